"""Writes the two PiT fixtures under tests/golden/ (run on the CPU: `python -m tests.make_pit_fixtures`):

  timm_pit_keys.json        name -> {state_dict key: shape} of timm's `PoolingVisionTransformer` for the eight served names, up to the
      last block.  Generated from the rule restated below -- on its own, not from i2v_amd.graphs -- and checked against timm wherever
      `import timm` works.  Where it does not, the contract is UNCHECKED against timm and the file says so ("checked_against").
  pit_fp32_cpu_errors.json  relative L2 error of the float32 CPU run of the references (tests/pit_reference.py) against their float64
      run on the inputs of tests/test_pit_cpu.py and tests/test_gpu_pit.py: what two correct float32 implementations may differ by.
      Never taken from the code under test.  "trajectory" records the float32 reference's own relative cost error after the 10-step I2V
      attack of the GPU test, per twin and depth.
"""
import json
import os

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")

#: name -> (patch, stride, base dim, heads, depths), all at 224 x 224; each has a `_distilled_224` twin with two prefix tokens
TABLE = {"pit_ti_224": (16, 8, 32, (2, 4, 8), (2, 6, 4)), "pit_xs_224": (16, 8, 48, (2, 4, 8), (2, 6, 4)),
         "pit_s_224": (16, 8, 48, (3, 6, 12), (2, 6, 4)), "pit_b_224": (14, 7, 64, (4, 8, 16), (3, 6, 4))}
#: the kernel's own tile sizes (csrc/i2v_pit_kernels.h: PIT_QT queries a workgroup owns, PIT_KT keys staged at a time)
QUERY_TILE, KEY_TILE = 64, 64
#: attention cases (frames, T, heads, dh, kind): a single key (P = 1, so dq and dk are identically 0); exactly one MFMA tile; one token
#: over it; ragged across key tiles; PiT's dh 48 ragged across several tiles; pit_s_224's and pit_b_distilled_224's stage-0 shapes; T one
#: below, at and one above the query / key tile of 64 (65 is in the list already) and at two tiles (the staged side's second tile exactly
#: full); three cases that force the online rescale over T = 200 = four key tiles (`attn_case`)
ATTN_CASES = [(1, 1, 1, 4, ""), (2, 16, 2, 8, ""), (2, 17, 2, 32, ""), (2, 65, 2, 16, ""), (3, 130, 3, 48, ""), (1, 730, 1, 48, ""),
              (1, 963, 1, 64, ""), (2, QUERY_TILE - 1, 2, 32, ""), (2, QUERY_TILE, 2, 32, ""), (1, 2 * KEY_TILE, 2, 64, ""),
              (1, 200, 2, 32, "late"), (1, 200, 2, 32, "early"), (1, 200, 2, 32, "ramp")]
#: pool cases (frames, grid, C, prefix): degenerate, even and odd grids; C = 4 and C = 6 (no multiple of a lane group of 4); 0, 1, 2 prefix rows
POOL_CASES = [(2, 1, 4, 0), (2, 2, 4, 1), (2, 3, 6, 2), (3, 7, 6, 1), (2, 8, 4, 2), (1, 8, 6, 0)]
#: patch cases (frames, p, s, side)
PATCH_CASES = [(2, 16, 8, 64), (2, 14, 7, 70), (3, 4, 2, 10)]
#: the test-size twins: label -> (a served name that maps to it, frame side, frames)
TWINS = {"pit_test": ("pit_s_224", 64, 3), "pit_test_70": ("pit_b_distilled_224", 70, 3), "pit_test_224": ("pit_ti_224", 224, 2)}
#: the full-size model of the GPU test, 2 frames
FULL = ("pit_s_224",)
#: the clips of the 10-step I2V trajectory whose float32 error is recorded: label -> (batch, frames, side, seed)
TRAJECTORY_CLIPS = {"pit_test": (2, 4, 64, 23), "pit_test_70": (2, 4, 70, 23)}
#: ... and the (twin, depth) the GPU test runs: the ragged twin (two prefix tokens, heads of width 12) at depth 3, the last block of stage
#: 1, which passes one pooling -- where the errors file ("trajectory") shows the float32 reference itself well inside the 2e-4 the other
#: families hold their trajectories to
TRAJECTORY = ("pit_test_70", 3)


def rule(patch, stride, base, heads, depths, prefix):
    """timm/models/pit.py (0.5.0), restated, without `norm.*`, `head.*` and `head_dist.*`: `pos_embed` (1, C, g, g), `cls_token`
    (1, prefix, C), `patch_embed.conv` (a Conv2d with kernel patch, stride stride and bias), then `transformers.{s}`: `blocks.{j}` of
    plain ViT blocks (norm1, attn.qkv, attn.proj, norm2, mlp.fc1, mlp.fc2, all with bias) and, behind stages 0 and 1, `pool.conv`
    (Conv2d(C, 2 C, 3, groups = C): weight (2 C, 1, 3, 3)) and `pool.fc` (Linear(C, 2 C))."""
    g = (224 - patch) // stride + 1
    W = [base * h for h in heads]
    out = {"pos_embed": [1, W[0], g, g], "cls_token": [1, prefix, W[0]], "patch_embed.conv.weight": [W[0], 3, patch, patch],
           "patch_embed.conv.bias": [W[0]]}
    for s in range(3):
        D = W[s]
        for j in range(depths[s]):
            p = f"transformers.{s}.blocks.{j}."
            out.update({p + "norm1.weight": [D], p + "norm1.bias": [D], p + "attn.qkv.weight": [3 * D, D], p + "attn.qkv.bias": [3 * D],
                        p + "attn.proj.weight": [D, D], p + "attn.proj.bias": [D], p + "norm2.weight": [D], p + "norm2.bias": [D],
                        p + "mlp.fc1.weight": [4 * D, D], p + "mlp.fc1.bias": [4 * D], p + "mlp.fc2.weight": [D, 4 * D], p + "mlp.fc2.bias": [D]})
        if s < 2:
            p = f"transformers.{s}.pool."
            out.update({p + "conv.weight": [2 * D, 1, 3, 3], p + "conv.bias": [2 * D], p + "fc.weight": [2 * D, D], p + "fc.bias": [2 * D]})
    return out


def keys_fixture():
    names = {}
    for n, row in TABLE.items():
        names[n] = rule(*row, 1)
        names[n.replace("_224", "_distilled_224")] = rule(*row, 2)
    checked = "unchecked against timm"
    try:
        import timm
    except ImportError:
        timm = None
    if timm is not None:
        for n, want in names.items():
            sd = timm.create_model(n, pretrained=False).state_dict()
            got = {k: list(v.shape) for k, v in sd.items() if not k.startswith(("head.", "head_dist.", "norm."))}
            assert got == want, (n, sorted(set(got) ^ set(want))[:8])
        checked = f"timm {timm.__version__}"
    return {"checked_against": checked, "follows": "timm 0.5.0 pit.py key layout (restated)", "names": names}


def compact(fx):
    """One block per line: the file is the contract, read by eye, and stays under the size limit."""
    head = {k: v for k, v in fx.items() if k != "names"}
    out = ["{"] + [f" {json.dumps(k)}: {json.dumps(v)}," for k, v in head.items()] + [' "names": {']
    for i, (n, keys) in enumerate(fx["names"].items()):
        out.append(f"  {json.dumps(n)}: {{")
        lines, cur, tag = [], [], None
        for k, v in keys.items():
            t = ".".join(k.split(".")[:4 if ".blocks." in k else 1])
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


# ---- streaming attention -----------------------------------------------------------------------------------------------------------
def attn_case(F_, T, H, dh, kind=""):
    """The float64 inputs of one case: qkv ~ N(0, 1), dout the output's gradient.  The rescale cases (every frame and head):
    "late": k[T - 3] = 4 q[5], so row 5's maximum arrives in the last key tile; "early": the same spike at key 2, so every later tile
    is rescaled against an old maximum; "ramp": k scaled by a ramp 0.2 .. 3.0 along the keys, so the maximum moves in most tiles."""
    d = {"qkv": _rand(F_, T, 3 * H * dh, seed=1), "dout": _rand(F_, T, H * dh, seed=3), "heads": H}
    C = H * dh
    if kind in ("late", "early"):
        d["qkv"][:, T - 3 if kind == "late" else 2, C:2 * C] = 4.0 * d["qkv"][:, 5, :C]
    if kind == "ramp":
        d["qkv"][:, :, C:2 * C] *= torch.linspace(0.2, 3.0, T, dtype=torch.float64)[None, :, None]
    return d


def attn_reference(d, dtype=torch.float64):
    """(out, dq, dk, dv, lse) of a case through tests/pit_reference.attn_core and autograd, in `dtype`."""
    from tests import pit_reference as pr
    c = _cast(d, dtype)
    qkv = c["qkv"].clone().requires_grad_(True)
    out = pr.attn_core(qkv, c["heads"])
    dqkv, = torch.autograd.grad(out, qkv, c["dout"])
    n, T, C3 = qkv.shape
    C, H = C3 // 3, c["heads"]
    q, k = (qkv.detach()[:, :, i * C:(i + 1) * C].reshape(n, T, H, C // H).transpose(1, 2) for i in (0, 1))
    lse = torch.logsumexp((q @ k.transpose(-2, -1)) * (C // H) ** -0.5, dim=-1)
    return out.detach(), dqkv[:, :, :C], dqkv[:, :, C:2 * C], dqkv[:, :, 2 * C:], lse


def case_key(F_, T, H, dh, kind=""):
    return f"{F_}x{T}x{H}x{dh}" + (f"-{kind}" if kind else "")


# ---- pool and patches --------------------------------------------------------------------------------------------------------------
def pool_case(F_, g, C, prefix):
    go = (g - 1) // 2 + 1
    return {"x": _rand(F_, prefix + g * g, C, seed=5), "w": _rand(2 * C, 1, 3, 3, seed=6), "b": _rand(2 * C, seed=7),
            "dy": _rand(F_, go * go, 2 * C, seed=8), "g": g, "prefix": prefix}


def pool_reference(d, dtype=torch.float64):
    """(y grid rows, dx grid rows) through conv2d and autograd."""
    from tests import pit_reference as pr
    c = _cast(d, dtype)
    x = c["x"].clone().requires_grad_(True)
    y = pr.pool_tokens(x, c["w"], c["b"], c["g"], c["prefix"])
    dx, = torch.autograd.grad(y, x, c["dy"])
    return y.detach(), dx[:, c["prefix"]:]


def patch_case(F_, p, s, side):
    g = (side - p) // s + 1
    return {"img": _rand(F_, 3, side, side, seed=9), "drows": _rand(F_ * g * g, 3 * p * p, seed=10), "p": p, "s": s}


def patch_reference(d, dtype=torch.float64):
    """(rows, gimg): F.unfold and its adjoint by autograd."""
    from tests import pit_reference as pr
    c = _cast(d, dtype)
    img = c["img"].clone().requires_grad_(True)
    rows = pr.patch_rows(img, c["p"], c["s"])
    gimg, = torch.autograd.grad(rows, img, c["drows"])
    return rows.detach(), gimg


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


def net_cases():
    from i2v_amd import graphs
    cases = []
    for label, (name, side, _) in TWINS.items():
        spec = graphs.build_tiny(name, (side, side))
        assert spec.arch == label
        cases.append((label, spec, twin_input(label)))
    for n in FULL:
        cases.append((n, graphs.build_surrogate(n), full_input()))
    return cases


def fp32_errors():
    from i2v_amd import graphs, weights
    from oracle import restate
    from tests import pit_reference as pr
    out = {"attention": {}, "pool": {}, "patch": {}}
    for case in ATTN_CASES:
        d = attn_case(*case)
        r64, r32 = attn_reference(d), attn_reference(d, torch.float32)
        rec = {"fwd": _rel(r32[0], r64[0]), "dv": _rel(r32[3], r64[3]), "lse": _rel(r32[4], r64[4])}
        if case[1] > 1:                                                    # (a single key: dq and dk are identically 0, no relative error)
            rec.update({"dq": _rel(r32[1], r64[1]), "dk": _rel(r32[2], r64[2])})
        out["attention"][case_key(*case)] = rec
    for case in POOL_CASES:
        d = pool_case(*case)
        r64, r32 = pool_reference(d), pool_reference(d, torch.float32)
        out["pool"]["x".join(map(str, case))] = {"fwd": _rel(r32[0], r64[0]), "bwd": _rel(r32[1], r64[1])}
    for case in PATCH_CASES:
        d = patch_case(*case)
        r64, r32 = patch_reference(d), patch_reference(d, torch.float32)
        out["patch"]["x".join(map(str, case))] = {"scatter": _rel(r32[1], r64[1])}
    for label, spec, x in net_cases():
        sd = weights.synthetic_state_dict(spec, 0)
        hooks = [spec.hook_for(d) for d in (1, 2, 3, 4)]
        r64, r32 = pr.PitReference(spec, sd, hooks), pr.PitReference(spec, sd, hooks, dtype=torch.float32)
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
            runs = [restate.run_attack([pr.PitReference(spec, sd, [spec.hook_for(depth)], dtype=dt)], vid, steps=10, step_size=0.005)
                    for dt in (torch.float64, torch.float32)]
            c64, c32 = (torch.as_tensor(r["costs"], dtype=torch.float64) for r in runs)
            out["trajectory"][label][str(depth)] = float(((c32 - c64).abs() / c64.abs()).max())
    return out


def main():
    with open(os.path.join(GOLDEN, "timm_pit_keys.json"), "w") as f:
        f.write(compact(keys_fixture()))
    errs = fp32_errors()
    with open(os.path.join(GOLDEN, "pit_fp32_cpu_errors.json"), "w") as f:
        json.dump(errs, f, indent=1)
    print(json.dumps(errs, indent=1))


if __name__ == "__main__":
    main()
