"""Writes the two BEiT fixtures under tests/golden/ (run on the CPU: `python -m tests.make_beit_fixtures`):

  timm_beit_keys.json        name -> {state_dict key: shape} of timm's `Beit` for the two served architectures, up to the last block, in
      timm's order, the int64 buffers `attn.relative_position_index` included.  Generated from the rule restated below -- on its own,
      not from i2v_amd.graphs -- and checked against timm wherever `import timm` works.  Where it does not, the contract is UNCHECKED
      against timm and the file says so ("checked_against").
  beit_fp32_cpu_errors.json  relative L2 error of the float32 CPU run of the references (tests/beit_reference.py) against their float64
      run on the inputs of tests/test_beit_cpu.py and tests/test_gpu_beit.py: what two correct float32 implementations may differ by.
      Never taken from the code under test.  "trajectory" records the float32 reference's own relative cost error after the 10-step I2V
      attack of the GPU test, per twin and depth.
"""
import json
import os

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")

#: name -> (patch, dim, heads, mlp, blocks), all at 224 x 224
TABLE = {"beit_base_patch16_224": (16, 768, 12, 3072, 12), "beit_large_patch16_224": (16, 1024, 16, 4096, 24)}
#: attention cases (frames, T, heads, dh, kind): a single key (P = 1, so dq and dk are exactly 0); one full tile; one key into the second
#: tile; a ragged T with a head width padded inside a 16-chunk; the workload's shape; the limit; kind "hot": scores and bias of magnitude
#: ~30 with the row maximum in the last key tile; kind "nobias": a null bias
ATTN_CASES = [(1, 1, 1, 4, ""), (2, 16, 2, 8, ""), (2, 17, 2, 32, ""), (3, 37, 4, 12, ""), (2, 197, 3, 64, ""), (1, 208, 1, 64, ""),
              (1, 197, 2, 64, "hot"), (2, 37, 2, 16, "nobias")]
#: the test-size twins: label -> (a served name that maps to it, frame side, frames)
TWINS = {"beit_test": ("beit_base_patch16_224", 64, 3), "beit_test_96": ("beit_large_patch16_224", 96, 3),
         "beit_test_224": ("beit_base_patch16_224", 224, 2)}
#: the full-size model of the GPU test, 2 frames
FULL = ("beit_base_patch16_224",)
#: the clips of the 10-step I2V trajectory whose float32 error is recorded: label -> (batch, frames, side, seed)
TRAJECTORY_CLIPS = {"beit_test": (2, 4, 64, 23), "beit_test_96": (2, 4, 96, 23)}
#: ... and the (twin, depth) the GPU test runs.  The float32 reference stays under 2e-4 at every depth on both twins (the errors file,
#: "trajectory": 4.8e-6 .. 1.3e-4), so the choice is free: the deepest hook, which runs all 8 blocks, on the twin where the float32
#: reference is closer there (2.8e-5 on beit_test_96 -- the ragged one, 37 tokens and heads of width 12 -- against 1.3e-4 on beit_test)
TRAJECTORY = ("beit_test_96", 4)


def rule(patch, dim, heads, mlp, blocks):
    """timm/models/beit.py (0.5.0), restated, without `norm.*` / `fc_norm.*` and `head.*`: `cls_token`, `patch_embed.proj` (a Conv2d with
    kernel = stride = patch and bias), no `pos_embed` and no shared `rel_pos_bias` (use_abs_pos_emb=False, use_shared_rel_pos_bias=False),
    then `blocks.{i}` (`Block`: the parameters gamma_1, gamma_2 first, then norm1, attn, norm2, mlp in the constructor's order;
    `Attention`: q_bias, v_bias, relative_position_bias_table ((2 g - 1)^2 + 3, heads), the buffer relative_position_index (T, T), then
    qkv (no bias key) and proj)."""
    g = 224 // patch
    T, rows = g * g + 1, (2 * g - 1) ** 2 + 3
    out = {"cls_token": [1, 1, dim], "patch_embed.proj.weight": [dim, 3, patch, patch], "patch_embed.proj.bias": [dim]}
    for i in range(blocks):
        p = f"blocks.{i}."
        out.update({p + "gamma_1": [dim], p + "gamma_2": [dim], p + "norm1.weight": [dim], p + "norm1.bias": [dim],
                    p + "attn.q_bias": [dim], p + "attn.v_bias": [dim], p + "attn.relative_position_bias_table": [rows, heads],
                    p + "attn.relative_position_index": [T, T], p + "attn.qkv.weight": [3 * dim, dim], p + "attn.proj.weight": [dim, dim],
                    p + "attn.proj.bias": [dim], p + "norm2.weight": [dim], p + "norm2.bias": [dim], p + "mlp.fc1.weight": [mlp, dim],
                    p + "mlp.fc1.bias": [mlp], p + "mlp.fc2.weight": [dim, mlp], p + "mlp.fc2.bias": [dim]})
    return out


def keys_fixture():
    names = {n: rule(*TABLE[n]) for n in TABLE}
    checked = "unchecked against timm"
    try:
        import timm
    except ImportError:
        timm = None
    if timm is not None:
        for n, want in names.items():
            sd = timm.create_model(n, pretrained=False).state_dict()
            got = {k: list(v.shape) for k, v in sd.items() if not k.startswith(("head.", "norm.", "fc_norm."))}
            assert got == want and list(got) == list(want), (n, sorted(set(got) ^ set(want))[:8])
        checked = f"timm {timm.__version__}"
    return {"checked_against": checked, "follows": "timm 0.5.0 beit.py key layout (restated)", "names": names}


def compact(fx):
    """One block per line: the file is the contract, read by eye, and stays under the size limit."""
    head = {k: v for k, v in fx.items() if k != "names"}
    out = ["{"] + [f" {json.dumps(k)}: {json.dumps(v)}," for k, v in head.items()] + [' "names": {']
    for i, (n, keys) in enumerate(fx["names"].items()):
        out.append(f"  {json.dumps(n)}: {{")
        lines, cur, tag = [], [], None
        for k, v in keys.items():
            t = ".".join(k.split(".")[:2 if k.startswith("blocks") else 1])
            if t != tag and cur:
                lines.append("   " + ", ".join(cur))
                cur = []
            tag = t
            cur.append(f"{json.dumps(k)}: {json.dumps(v)}")
        lines.append("   " + ", ".join(cur))
        out += [ln + ("," if j + 1 < len(lines) else "") for j, ln in enumerate(lines)]
        out.append("  }" + ("," if i + 1 < len(fx["names"]) else ""))
    return "\n".join(out + [" }", "}"]) + "\n"


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def _rand(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


def _cast(d, dtype):
    return {k: (v.to(dtype) if torch.is_tensor(v) else v) for k, v in d.items()}


# ---- biased global attention -------------------------------------------------------------------------------------------------------
def attn_case(F_, T, H, dh, kind=""):
    """The float64 inputs of one case: qkv, bias ~ N(0, 1), dout the output's gradient.  "hot": q times 40 / sqrt(dh) (scores of
    standard deviation 5) and the bias times 5, with 30 added to the keys of the last 16-key tile, so that the row maximum lies there,
    at about 30 to 45; "nobias": no bias."""
    d = {"qkv": _rand(F_, T, 3 * H * dh, seed=1), "bias": _rand(H, T, T, seed=2), "dout": _rand(F_, T, H * dh, seed=3), "heads": H}
    if kind == "hot":
        d["qkv"][:, :, :H * dh] *= 40.0 / dh ** 0.5
        d["bias"] = d["bias"] * 5.0
        d["bias"][:, :, (T - 1) // 16 * 16:] += 30.0
    if kind == "nobias":
        d["bias"] = None
    return d


def attn_reference(d, dtype=torch.float64):
    """(out, dq, dk, dv) of a case through tests/beit_reference.attn_core (timm's literal arithmetic) and autograd, in `dtype`."""
    from tests import beit_reference as br
    c = _cast(d, dtype)
    qkv = c["qkv"].clone().requires_grad_(True)
    out = br.attn_core(qkv, c["bias"], c["heads"])
    dqkv, = torch.autograd.grad(out, qkv, c["dout"])
    C = qkv.shape[2] // 3
    return out.detach(), dqkv[:, :, :C], dqkv[:, :, C:2 * C], dqkv[:, :, 2 * C:]


def case_key(F_, T, H, dh, kind=""):
    return f"{F_}x{T}x{H}x{dh}" + (f"-{kind}" if kind else "")


def twin_input(label):
    _, side, frames = TWINS[label]
    return _rand(frames, 3, side, side, seed=21)


def full_input():
    return _rand(2, 3, 224, 224, seed=22)


def video(b, f, hw, seed):
    from oracle import restate
    gen = torch.Generator().manual_seed(seed)
    u8 = torch.randint(0, 256, (b, 3, f, hw, hw), generator=gen, dtype=torch.uint8)
    mean = torch.tensor(restate.MEAN).view(1, 3, 1, 1, 1)
    std = torch.tensor(restate.STD).view(1, 3, 1, 1, 1)
    return (u8.float() / 255 - mean) / std


def fp32_errors():
    from i2v_amd import graphs, weights
    from oracle import restate
    from tests import beit_reference as br
    out = {"attention": {}}
    for case in ATTN_CASES:
        d = attn_case(*case)
        r64, r32 = attn_reference(d), attn_reference(d, torch.float32)
        rec = {"fwd": _rel(r32[0], r64[0]), "dv": _rel(r32[3], r64[3])}
        if case[1] > 1:                                                    # (a single key: dq and dk are identically 0, no relative error)
            rec.update({"dq": _rel(r32[1], r64[1]), "dk": _rel(r32[2], r64[2])})
        out["attention"][case_key(*case)] = rec
    cases = []
    for label, (name, side, _) in TWINS.items():
        spec = graphs.build_tiny(name, (side, side))
        assert spec.arch == label
        cases.append((label, spec, twin_input(label)))
    for n in FULL:
        cases.append((n, graphs.build(n), full_input()))
    for label, spec, x in cases:
        sd = weights.synthetic_state_dict(spec, 0)
        hooks = [spec.hook_for(d) for d in (1, 2, 3, 4)]
        r64, r32 = br.BeitReference(spec, sd, hooks), br.BeitReference(spec, sd, hooks, dtype=torch.float32)
        f64, f32 = r64.forward(x), r32.forward(x)
        hg = [_rand(*f.shape, seed=30 + i) for i, f in enumerate(f64)]
        out[label] = {"hooks": [_rel(a, b) for a, b in zip(f32, f64)], "grad": _rel(r32.backward(hg), r64.backward(hg)),
                      "hook_std": [float(f.std()) for f in f64]}
    out["trajectory"] = {}
    for label, clip in TRAJECTORY_CLIPS.items():
        name, side, _ = TWINS[label]
        spec = graphs.build_tiny(name, (side, side))
        sd, vid = weights.synthetic_state_dict(spec, 0), video(*clip)
        out["trajectory"][label] = {}
        for depth in (1, 2, 3, 4):
            runs = [restate.run_attack([br.BeitReference(spec, sd, [spec.hook_for(depth)], dtype=dt)], vid, steps=10, step_size=0.005)
                    for dt in (torch.float64, torch.float32)]
            c64, c32 = (torch.as_tensor(r["costs"], dtype=torch.float64) for r in runs)
            out["trajectory"][label][str(depth)] = float(((c32 - c64).abs() / c64.abs()).max())
    return out


def main():
    with open(os.path.join(GOLDEN, "timm_beit_keys.json"), "w") as f:
        f.write(compact(keys_fixture()))
    errs = fp32_errors()
    with open(os.path.join(GOLDEN, "beit_fp32_cpu_errors.json"), "w") as f:
        json.dump(errs, f, indent=1)
    print(json.dumps(errs, indent=1))


if __name__ == "__main__":
    main()
