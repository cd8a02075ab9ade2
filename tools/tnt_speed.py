"""Speed of a 10-step TNT I2V attack (depth 3) on b x 32 x 224^2 clips, in adversarial frames/s: the end-to-end counterpart of
tools/tnt_attention_bench.py.  `--arch` is any served name (`graphs.TNT_MODELS`).

    python tools/tnt_speed.py engine [--arch NAME] [--clips 4] [--steps 10] [--reps 2]   # the product class on the HIP path
    python tools/tnt_speed.py eager  [--arch NAME] [--clips 4] [--steps 10] [--reps 2]   # the same loop in eager PyTorch fp32 on the same GPU
    python tools/tnt_speed.py shares --stats FILE   # kernel-time shares from a `rocprofv3 --kernel-trace --stats` kernel stats csv or results database of an engine run

Run each side in a process of its own.  Synthetic weights (seed 0); the first call of each side warms up and is not timed.  Prints one
JSON line with every timed call and the rate of the fastest."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "image-to-video-i2v-attack_amd"), ROOT]


def clips(b, f, seed=0):
    import torch
    from oracle import restate
    gen = torch.Generator().manual_seed(seed)
    u8 = torch.randint(0, 256, (b, 3, f, 224, 224), generator=gen, dtype=torch.uint8)
    mean = torch.tensor(restate.MEAN).view(1, 3, 1, 1, 1)
    std = torch.tensor(restate.STD).view(1, 3, 1, 1, 1)
    return (u8.float() / 255 - mean) / std


def eager_attack(vid, sd, spec, block, steps, lr=0.005, eps=16 / 255):
    """image_attacks.py:294-364 (ImageGuidedFMDirection_Adam) in eager PyTorch over the reference's blocks."""
    import torch
    from oracle import restate
    from tests import tnt_reference as cr
    dev = vid.device
    b, c, f, h, w = vid.shape
    x = vid.permute(0, 2, 1, 3, 4).reshape(b * f, c, h, w)
    mean = torch.tensor(restate.MEAN, device=dev).view(1, 3, 1, 1)
    std = torch.tensor(restate.STD, device=dev).view(1, 3, 1, 1)
    u = x * std + mean

    def feat(inp):
        return cr.streams(inp, sd, spec, block + 1)[block].reshape(inp.shape[0], -1)
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


def shares(path):
    """Kernel-time shares of a profiled engine run: the shared linear launch, the inner attention, the outer attention, the rest."""
    import csv
    import sqlite3
    groups = {"shared_linear": 0.0, "inner_attention": 0.0, "outer_attention": 0.0, "rest": 0.0}
    if path.endswith(".db"):       # the profiler's database (its default output): the `kernels` view, one row per dispatch
        rows = sqlite3.connect(path).execute("select name, sum(duration) from kernels group by name").fetchall()
    else:                          # ... or its kernel stats csv (--output-format csv)
        rows = [(r["Name"], float(r["TotalDurationNs"])) for r in csv.DictReader(open(path))]
    for name, ns in rows:
        key = "shared_linear" if "vit_gemm" in name else "inner_attention" if "tnt_attn" in name else "outer_attention" if "beit_attn" in name else "rest"
        groups[key] += ns
    total = sum(groups.values())
    print(json.dumps({"kernel_ms": {k: round(v / 1e6, 2) for k, v in groups.items()}, "share": {k: round(v / total, 3) for k, v in groups.items()}}))


def main():
    import torch
    from i2v_amd import attacks, graphs, weights
    ap = argparse.ArgumentParser()
    ap.add_argument("side", choices=("engine", "eager", "shares"))
    ap.add_argument("--stats", default="")
    ap.add_argument("--arch", default="tnt_s_patch16_224", choices=sorted(graphs.TNT_MODELS))
    ap.add_argument("--depth", type=int, default=3)
    ap.add_argument("--clips", type=int, default=4)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--reps", type=int, default=2)
    a = ap.parse_args()
    if a.side == "shares":
        return shares(a.stats)
    vid = clips(a.clips, 32)
    spec = graphs.build_surrogate(a.arch)
    times = []
    if a.side == "engine":
        atk = attacks.ImageGuidedFMDirection_Adam([a.arch], depth=a.depth, step_size=0.005, steps=a.steps, weight_seed=0)
        labels, names = torch.zeros(a.clips, dtype=torch.long), [f"c{i}" for i in range(a.clips)]
        run = lambda: atk(vid, labels, names)      # noqa: E731
    else:
        sd = {k: v.cuda() for k, v in weights.synthetic_state_dict(spec, 0).items()}
        vd = vid.cuda()
        run = lambda: eager_attack(vd, sd, spec, spec.hook_for(a.depth), a.steps)      # noqa: E731
    for r in range(a.reps + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        run()
        torch.cuda.synchronize()
        if r:
            times.append(time.perf_counter() - t0)
    print(json.dumps({"side": a.side, "arch": a.arch, "depth": a.depth, "block": spec.hook_for(a.depth), "clips": a.clips, "frames": 32,
                      "steps": a.steps, "seconds": [round(t, 4) for t in times], "adv_frames_per_s": round(a.clips * 32 / min(times), 2)}))


if __name__ == "__main__":
    main()
