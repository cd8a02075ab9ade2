"""Speed of a 10-step I2V attack (depth 3) on a transformer surrogate of any family of `graphs.FAMILIES`, on b x 32 x 224^2 clips, in
adversarial frames/s: the end-to-end counterpart of the families' kernel benches (`tools/*_attention_bench.py` and kin).  `--arch` is any
served name; the family is the row of `graphs.FAMILIES` that serves it.  `--family WORD` alone picks that family's default model.

    python tools/family_speed.py engine --arch NAME [--clips 4] [--steps 10] [--reps 2]   # the product class on the HIP path
    python tools/family_speed.py eager  --arch NAME [--clips 4] [--steps 10] [--reps 2]   # the same loop in eager PyTorch fp32 on the same GPU
    python tools/family_speed.py shares --family WORD FILE                                 # kernel-time shares of a profiled engine run (or --arch NAME; --stats FILE)

Run each side in a process of its own; for BEiT and PiT `I2V_BEIT_ATTN=0` / `I2V_PIT_ATTN=0` in front of `engine` is the shared-launch
route, and the line names the route.  Synthetic weights (seed 0); the first call of each side warms up (planning, allocator) and is not
timed.  Prints one JSON line with every timed call and the rate of the fastest.  `shares` reads what `rocprofv3 --kernel-trace --stats`
wrote for an `engine` run, the results database or the kernel stats csv (`bench_util.kernel_rows`), and groups the device time by the
family's kernel names (`ROWS`); what matches no group is "the rest" (token assembly, loss, Adam step, copies).  Every family's line has
the form its own tool printed: {"file", "device_ms", "shares": {group: ms, launches, share}}, and for TNT {"kernel_ms", "share"}.  The
old tools knew their family from their name; here `shares` needs `--family` or `--arch`.

What a family brings is its row of `ROWS`: the default model, the module under tests/ whose `streams` the eager side runs, what its
hooks number, the kernel-name groups, and the environment variable of its second route if it has one."""
import argparse
import importlib
import json
import os
import time
from typing import NamedTuple, Optional

from bench_util import kernel_rows


class Row(NamedTuple):
    arch: str                       # the default model
    reference: str                  # tests/<reference>.py: its `streams(x, sd, spec, n)` is the eager side
    hooked: str                     # what the family's hooks number: the JSON key of the hook
    groups: tuple                   # (group, kernel-name substrings) of `shares`, the first match wins
    route_env: Optional[str] = None             # "0" there sends attention through the shared launches
    streams: str = "streams"
    split: Optional[str] = None                 # kernels with this substring are also listed forward / backward on their own
    flat: bool = False                          # `shares` prints TNT's form: {"kernel_ms": {group: ms}, "share": {group: share}}, remainder "rest"


GEMM, LN = ("linear GEMMs", ("vit_gemm_kernel",)), ("LayerNorm", ("vit_layernorm_",))
ROWS = {
    "vit": Row("vit_base_patch16_224", "vit_family_reference", "block", (GEMM, ("softmax", ("vit_softmax_",)), LN)),
    "swin": Row("swin_tiny_patch4_window7_224", "swin_reference", "stage", (GEMM, ("window attention", ("swin_attn_",)), LN, ("merging", ("swin_merge_kernel",))),
                split="swin_attn_"),
    "convnext": Row("convnext_tiny", "convnext_reference", "stage", (GEMM, ("depthwise 7x7", ("convnext_dw_kernel",)), LN, ("gather", ("swin_merge_kernel",)))),
    "mixer": Row("mixer_b16_224", "mixer_reference", "block", (GEMM, ("token mixing", ("mixer_tokens_kernel",)), LN)),
    "cait": Row("cait_s24_224", "cait_reference", "block", (GEMM, ("talking-heads attention", ("cait_attn_",)), LN)),
    "convit": Row("convit_small", "convit_reference", "block", (GEMM, ("gated positional attention", ("convit_attn_",)), LN)),
    "xcit": Row("xcit_small_12_p16_224", "xcit_reference", "block",
                (GEMM, ("cross-covariance attention", ("xcit_attn_",)), ("depthwise 3 x 3", ("xcit_dw3_",)),
                 ("stem gather / scatter", ("xcit_gather_", "xcit_scatter_")), LN)),
    "twins": Row("twins_pcpvt_small", "twins_reference", "stage",
                 (GEMM, ("sub-sampled attention", ("twins_attn_",)), ("window attention", ("swin_attn_",)),
                  ("gathers / scatters", ("twins_block_", "swin_merge_")), ("position encoding", ("xcit_dw3_",)), LN), streams="stages"),
    "beit": Row("beit_base_patch16_224", "beit_reference", "block",
                (("GEMMs", ("vit_gemm_kernel",)), ("biased attention", ("beit_attn_",)), ("bias add / softmax", ("beit_bias_add_", "vit_softmax_")), LN),
                route_env="I2V_BEIT_ATTN"),
    "pit": Row("pit_s_224", "pit_reference", "block",
               (("GEMMs", ("vit_gemm_kernel",)), ("streaming attention", ("pit_attn_",)), ("softmax", ("vit_softmax_",)), LN,
                ("pool / patches", ("pit_pool_", "pit_patch_"))), route_env="I2V_PIT_ATTN"),
    "coat": Row("coat_lite_tiny", "coat_reference", "stage", (GEMM, ("factorized attention", ("coat_",)), LN)),
    "tnt": Row("tnt_s_patch16_224", "tnt_reference", "block",
               (("shared_linear", ("vit_gemm",)), ("inner_attention", ("tnt_attn",)), ("outer_attention", ("beit_attn",))), flat=True),
}


def clips(b, f, seed=0):
    from tests.family_harness import video
    return video(b, f, 224, seed)


def eager_attack(vid, feat, steps, lr=0.005, eps=16 / 255):
    """image_attacks.py:294-364 (ImageGuidedFMDirection_Adam) in eager PyTorch over `feat`: frames (n, 3, h, w) -> the hooked feature (n, D)."""
    import torch
    from oracle import restate
    dev = vid.device
    b, c, f, h, w = vid.shape
    x = vid.permute(0, 2, 1, 3, 4).reshape(b * f, c, h, w)
    mean = torch.tensor(restate.MEAN, device=dev).view(1, 3, 1, 1)
    std = torch.tensor(restate.STD, device=dev).view(1, 3, 1, 1)
    u = x * std + mean
    with torch.no_grad():
        init = feat(x)
    delta = torch.full_like(x, 0.01 / 255).requires_grad_(True)
    opt = torch.optim.Adam([delta], lr=lr)
    for _ in range(steps):
        xn = (torch.clamp(u + torch.clamp(delta, -eps, eps), 0, 1) - mean) / std
        cost = torch.nn.functional.cosine_similarity(feat(xn), init, dim=1, eps=1e-8).sum()
        opt.zero_grad()
        cost.backward()
        opt.step()
    return delta.detach()


def patch_rows(x, sd, spec):
    """A patch embedding's strided convolution written as what it is, a reshape into patch rows and one matrix product: the eager side of
    ViT and Swin then runs on the BLAS library alone, whatever the patch size."""
    N, g, P = x.shape[0], spec.img // spec.patch, spec.patch
    rows = x.reshape(N, spec.in_chans, g, P, g, P).permute(0, 2, 4, 1, 3, 5).reshape(N, g * g, spec.in_chans * P * P)
    return rows @ sd["patch_embed.proj.weight"].reshape(spec.dim, -1).T + sd["patch_embed.proj.bias"]


def eager_feat(word, ref, sd, spec, hook):
    """The hooked feature of the eager side: the reference's streams up to the hook, except where a family's eager side was measured on
    another embedding than the reference's (ViT, Swin: `patch_rows`; ConvNeXt: channels-last planes)."""
    import torch
    if word == "vit":
        def tokens(x):
            prefix = [sd[k].reshape(1, 1, -1).expand(x.shape[0], 1, spec.dim) for k in ref.PREFIX_KEYS[:spec.n_prefix]]
            return torch.cat(prefix + [patch_rows(x, sd, spec)], 1) + sd["pos_embed"].reshape(1, spec.tokens, spec.dim)
        return lambda x: ref.run_blocks(tokens(x), sd, spec, [hook])[0].reshape(x.shape[0], -1)
    if word == "swin":
        norm = lambda e: ref.layer_norm(e, sd["patch_embed.norm.weight"], sd["patch_embed.norm.bias"], spec.ln_eps)      # noqa: E731
        return lambda x: ref.run_stages(norm(patch_rows(x, sd, spec)), sd, spec, [hook])[0].reshape(x.shape[0], -1)
    if word == "convnext":
        plane = lambda x: ref.stem(x, sd, spec).contiguous(memory_format=torch.channels_last)      # noqa: E731
        return lambda x: ref.run_stages(plane(x), sd, spec, [hook])[0].permute(0, 2, 3, 1).reshape(x.shape[0], -1)
    streams = getattr(ref, ROWS[word].streams)
    return lambda x: streams(x, sd, spec, hook + 1)[hook].reshape(x.shape[0], -1)


def time_calls(run, reps):
    """Seconds of each of `reps` calls after one that warms up."""
    import torch
    times = []
    for r in range(reps + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        run()
        torch.cuda.synchronize()
        if r:
            times.append(time.perf_counter() - t0)
    return times


def shares(path, groups, split=None, flat=False):
    rest = "rest" if flat else "the rest"
    tot = {name: [0, 0] for name, _ in tuple(groups) + ((rest, ()),)}
    per_kernel = {}
    for name, calls, ns in kernel_rows(path):
        fam = next((g for g, marks in groups if any(m in name for m in marks)), rest)
        tot[fam][0] += int(ns)
        tot[fam][1] += calls
        if split and split in name:
            per_kernel[split + ("bwd" if "bwd" in name else "fwd")] = int(ns)
            home = fam
    whole = sum(v[0] for v in tot.values())
    if flat:
        return print(json.dumps({"kernel_ms": {k: round(v[0] / 1e6, 2) for k, v in tot.items()}, "share": {k: round(v[0] / whole, 3) for k, v in tot.items()}}))
    out = {k: {"ms": round(v[0] / 1e6, 2), "launches": v[1], "share": round(v[0] / whole, 4)} for k, v in tot.items()}
    if per_kernel:
        out[home].update({k: round(v / whole, 4) for k, v in per_kernel.items()})
    print(json.dumps({"file": os.path.basename(path), "device_ms": round(whole / 1e6, 2), "shares": out}))


def main():
    from i2v_amd import graphs
    ap = argparse.ArgumentParser()
    ap.add_argument("side", choices=("engine", "eager", "shares"))
    ap.add_argument("file", nargs="?", default="", help="shares: the profiler's results database or kernel stats csv")
    ap.add_argument("--stats", default="", help="shares: the same file, by name")
    ap.add_argument("--family", choices=sorted(ROWS), help="the family, where no --arch is given: its default model")
    ap.add_argument("--arch", choices=sorted(n for f in graphs.FAMILIES for n in f.models))
    ap.add_argument("--depth", type=int, default=3)
    ap.add_argument("--clips", type=int, default=4)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--reps", type=int, default=2)
    a = ap.parse_intermixed_args()      # FILE may stand behind the options
    if not (a.arch or a.family):
        ap.error("one of --arch and --family is needed")
    word = next(f.word for f in graphs.FAMILIES if a.arch in f.models) if a.arch else a.family
    if a.family and a.family != word:
        ap.error(f"--arch {a.arch} is a model of the family {word}, not of --family {a.family}")
    row = ROWS[word]
    arch = a.arch or row.arch
    if a.side == "shares":
        if not (a.file or a.stats):
            ap.error("shares needs the profiler's results database or kernel stats csv: FILE or --stats FILE")
        return shares(a.file or a.stats, row.groups, row.split, row.flat)
    import torch
    from i2v_amd import attacks, weights
    vid = clips(a.clips, 32)
    spec = graphs.build_surrogate(arch)
    hook = spec.hook_for(a.depth)
    if a.side == "engine":
        atk = attacks.ImageGuidedFMDirection_Adam([arch], depth=a.depth, step_size=0.005, steps=a.steps, weight_seed=0)
        labels, names = torch.zeros(a.clips, dtype=torch.long), [f"c{i}" for i in range(a.clips)]
        run = lambda: atk(vid, labels, names)      # noqa: E731
    else:
        sd = {k: v.cuda() for k, v in weights.synthetic_state_dict(spec, 0).items()}
        vd = vid.cuda()
        feat = eager_feat(word, importlib.import_module("tests." + row.reference), sd, spec, hook)
        run = lambda: eager_attack(vd, feat, a.steps)      # noqa: E731
    times = time_calls(run, a.reps)
    line = {"side": a.side, "arch": arch, "depth": a.depth, row.hooked: hook, "clips": a.clips, "frames": 32, "steps": a.steps}
    if row.route_env:
        line["route"] = "eager" if a.side == "eager" else "shared launches" if os.environ.get(row.route_env) == "0" else "attention launch"
    line.update({"seconds": [round(t, 4) for t in times], "adv_frames_per_s": round(a.clips * 32 / min(times), 2)})
    print(json.dumps(line))


if __name__ == "__main__":
    main()
