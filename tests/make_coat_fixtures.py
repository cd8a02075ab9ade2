"""Writes the two CoaT fixtures under tests/golden/ (run on the CPU: `python -m tests.make_coat_fixtures`):

  timm_coat_keys.json        name -> {state_dict key: shape} of timm's serial `CoaT` for the three served names, up to the last block,
      the shared cpe / crpe under their stage-level keys.  Generated from the rule restated below -- on its own, not from
      i2v_amd.graphs -- and checked against timm wherever `import timm` works.  Where it does not, the contract is UNCHECKED against timm
      and the file says so ("checked_against").
  coat_fp32_cpu_errors.json  relative L2 error of the float32 CPU run of the references (tests/coat_reference.py) against their float64
      run on the inputs of tests/test_coat_cpu.py and tests/test_gpu_coat.py: what two correct float32 implementations may differ by.
      Never taken from the code under test.  "trajectory" records the float32 reference's own relative cost error after the 10-step I2V
      attack of the GPU test, per depth.
"""
import json
import os

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")

#: name -> (widths, depths, MLP ratios), all at 224 x 224 with 8 heads and crpe windows 3 / 5 / 7 on 2 / 3 / 3 heads
TABLE = {"coat_lite_tiny": ((64, 128, 256, 320), (2, 2, 2, 2), (8, 8, 4, 4)), "coat_lite_mini": ((64, 128, 320, 512), (2, 2, 2, 2), (8, 8, 4, 4)),
         "coat_lite_small": ((64, 128, 320, 512), (3, 4, 6, 3), (8, 8, 4, 4))}
HEADS, WINDOW_HEADS = 8, (2, 3, 3)
#: the kernel's token tile (csrc/i2v_coat_kernels.h: COAT_TT)
TOKEN_TILE = 64
#: attention cases (frames, T, heads, dh, kind): a single token (Ks = 1, G = v, dk = 0); a few tokens at the narrowest head; the last
#: stage's 50 tokens at dh 40 and 64; T around the token tile and at two tiles with dh 8; the stage shapes 197 x 32, 785 x 16 and
#: 3137 x 8; dh ragged against the MFMA chunk with fewer heads than a group holds; three cases at T = 200 that stress the column softmax
ATTN_CASES = [(1, 1, 8, 8, ""), (2, 5, 8, 4, ""), (1, 50, 8, 40, ""), (1, 50, 8, 64, ""), (1, TOKEN_TILE - 1, 8, 8, ""), (1, TOKEN_TILE, 8, 8, ""),
              (1, TOKEN_TILE + 1, 8, 8, ""), (1, 2 * TOKEN_TILE, 8, 8, ""), (2, 197, 8, 32, ""), (1, 785, 8, 16, ""), (1, 3137, 8, 8, ""),
              (1, 130, 4, 12, ""), (1, 130, 1, 20, ""), (1, 200, 8, 8, "peak"), (1, 200, 8, 8, "late"), (1, 200, 8, 8, "ramp")]
ATTN_PARTS = ("out", "gram", "dq", "dk", "dv", "dE")
#: dwmix cases (frames, grid, C, n3, n5, n7, prefix, form): "own" -- x an array of its own; "qkv" -- x is v, read in place out of a
#: (frames, T, 3 C) array at row stride 3 C, and the backward accumulates into such an array; "cpe" -- n3 = C with the residual on
DW_CASES = [(2, 1, 24, 8, 8, 8, 1, "own"), (2, 2, 24, 8, 8, 8, 1, "own"), (2, 3, 24, 8, 12, 4, 1, "qkv"), (2, 7, 32, 8, 12, 12, 1, "qkv"),
            (1, 14, 64, 16, 24, 24, 1, "qkv"), (2, 7, 16, 8, 0, 8, 1, "own"), (2, 3, 16, 0, 16, 0, 0, "own"), (2, 7, 20, 20, 0, 0, 1, "cpe"),
            (1, 14, 32, 32, 0, 0, 1, "cpe"), (2, 2, 8, 8, 0, 0, 0, "cpe")]
#: cell cases (frames, grid, C, s), one prefix row
CELL_CASES = [(2, 2, 8, 2), (2, 6, 12, 2), (1, 14, 16, 2), (2, 6, 12, 1)]
#: the test-size twins: label -> (a served name that maps to it, frame side, frames)
TWINS = {"coat_test": ("coat_lite_tiny", 64, 3), "coat_test_96": ("coat_lite_mini", 96, 2), "coat_test_224": ("coat_lite_small", 224, 1)}
#: the full-size model of the GPU test, one frame
FULL = ("coat_lite_tiny",)
#: the clip of the 10-step I2V trajectory on coat_test whose float32 error is recorded: (batch, frames, side, seed); the GPU test's depth
TRAJECTORY_CLIP, TRAJECTORY_DEPTH = (2, 4, 64, 23), 3


def rule(widths, depths, ratios):
    """timm/models/coat.py (0.5.0), serial models, restated from memory, without `norm*`, `head.*`, `aggregate.*` and the block-level
    duplicates of the shared modules: per stage s = 1..4 `patch_embed{s}.proj` (Conv2d, kernel 4 then 2) and `.norm`, `cls_token{s}`
    (1, 1, C), `cpe{s}.proj` (depthwise 3 x 3), `crpe{s}.conv_list.{0,1,2}` (depthwise 3 / 5 / 7 on 2 / 3 / 3 heads' channels), then
    `serial_blocks{s}.{j}`: norm1, factoratt_crpe.qkv, factoratt_crpe.proj, norm2, mlp.fc1, mlp.fc2, all with bias."""
    out = {}
    for k in range(4):
        D, Cin, p, s, dh = widths[k], widths[k - 1] if k else 3, 2 if k else 4, k + 1, widths[k] // HEADS
        out.update({f"patch_embed{s}.proj.weight": [D, Cin, p, p], f"patch_embed{s}.proj.bias": [D], f"patch_embed{s}.norm.weight": [D],
                    f"patch_embed{s}.norm.bias": [D], f"cls_token{s}": [1, 1, D], f"cpe{s}.proj.weight": [D, 1, 3, 3], f"cpe{s}.proj.bias": [D]})
        for i, (K, h) in enumerate(zip((3, 5, 7), WINDOW_HEADS)):
            out.update({f"crpe{s}.conv_list.{i}.weight": [h * dh, 1, K, K], f"crpe{s}.conv_list.{i}.bias": [h * dh]})
        M = ratios[k] * D
        for j in range(depths[k]):
            q = f"serial_blocks{s}.{j}."
            out.update({q + "norm1.weight": [D], q + "norm1.bias": [D], q + "factoratt_crpe.qkv.weight": [3 * D, D], q + "factoratt_crpe.qkv.bias": [3 * D],
                        q + "factoratt_crpe.proj.weight": [D, D], q + "factoratt_crpe.proj.bias": [D], q + "norm2.weight": [D], q + "norm2.bias": [D],
                        q + "mlp.fc1.weight": [M, D], q + "mlp.fc1.bias": [M], q + "mlp.fc2.weight": [D, M], q + "mlp.fc2.bias": [D]})
    return out


def keys_fixture():
    names = {n: rule(*row) for n, row in TABLE.items()}
    checked = "unchecked against timm"
    try:
        import timm
    except ImportError:
        timm = None
    if timm is not None:
        for n, want in names.items():
            sd = timm.create_model(n, pretrained=False).state_dict()
            got = {k: list(v.shape) for k, v in sd.items() if k in want or not k.startswith(("head.", "norm", "aggregate.", "serial_blocks"))}
            assert got == want, (n, sorted(set(got) ^ set(want))[:8])
        checked = f"timm {timm.__version__}"
    return {"checked_against": checked, "follows": "timm 0.5.0 coat.py key layout (restated from memory)", "names": names}


def compact(fx):
    """One stage module or block per line: the file is the contract, read by eye, and stays under the size limit."""
    head = {k: v for k, v in fx.items() if k != "names"}
    out = ["{"] + [f" {json.dumps(k)}: {json.dumps(v)}," for k, v in head.items()] + [' "names": {']
    for i, (n, keys) in enumerate(fx["names"].items()):
        out.append(f"  {json.dumps(n)}: {{")
        lines, cur, tag = [], [], None
        for k, v in keys.items():
            t = ".".join(k.split(".")[:2 if k.startswith("serial_blocks") else 1])
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


# ---- factorized attention ----------------------------------------------------------------------------------------------------------
def attn_case(F_, T, H, dh, kind=""):
    """The float64 inputs of one case: qkv and E ~ N(0, 1) (E's class row 0), dout the output's gradient.  The softmax cases, in every
    column of k: "peak": token 7 lies 30 above the column's maximum; "late": token T - 3, in the last tile, lies 3 above it; "ramp": k
    is 0.1 N(0, 1) plus a ramp 0 .. 8 along the tokens, so the running maximum moves in every tile."""
    C = H * dh
    d = {"qkv": _rand(F_, T, 3 * C, seed=1), "E": _rand(F_, T, C, seed=2), "dout": _rand(F_, T, C, seed=3), "heads": H}
    d["E"][:, 0] = 0.0
    k = d["qkv"][:, :, C:2 * C]
    if kind == "peak":
        k[:, 7] = k.max(dim=1).values + 30.0
    if kind == "late":
        k[:, T - 3] = k.max(dim=1).values + 3.0
    if kind == "ramp":
        k.mul_(0.1).add_(torch.linspace(0.0, 8.0, T, dtype=torch.float64)[None, :, None])
    return d


def attn_reference(d, dtype=torch.float64):
    """(out, gram, dq, dk, dv, dE) of a case through tests/coat_reference.factor_core and autograd, in `dtype`."""
    from tests import coat_reference as cr
    c = _cast(d, dtype)
    qkv, E = c["qkv"].clone().requires_grad_(True), c["E"].clone().requires_grad_(True)
    out = cr.factor_core(qkv, E, c["heads"])
    dqkv, dE = torch.autograd.grad(out, (qkv, E), c["dout"])
    C = qkv.shape[2] // 3
    gram = cr.factor_parts(qkv.detach(), c["heads"])[4]
    return out.detach(), gram, dqkv[:, :, :C], dqkv[:, :, C:2 * C], dqkv[:, :, 2 * C:], dE


def case_key(*case):
    return "x".join(str(v) for v in case if v != "")


# ---- dwmix and cells ---------------------------------------------------------------------------------------------------------------
def dw_case(F_, g, C, n3, n5, n7, prefix, form):
    R = prefix + g * g
    d = {"x": _rand(F_, R, 3 * C if form == "qkv" else C, seed=5), "dy": _rand(F_, R, C, seed=8), "b": _rand(C, seed=7), "g": g, "prefix": prefix,
         "form": form, "C": C}
    for i, (K, n) in enumerate(zip((3, 5, 7), (n3, n5, n7))):
        d[f"w{K}"] = _rand(n, 1, K, K, seed=60 + i) / K
    return d


def dw_reference(d, dtype=torch.float64):
    """(y, dx) through conv2d and autograd; dx is the gradient with respect to the C channels the launch reads."""
    from tests import coat_reference as cr
    c = _cast(d, dtype)
    C, g, pre = c["C"], c["g"], c["prefix"]
    x = (c["x"][:, :, 2 * C:] if c["form"] == "qkv" else c["x"]).clone().requires_grad_(True)
    if c["form"] == "cpe":
        y = cr.cpe(x, c["w3"], c["b"], g, pre)
    else:
        ws = [c["w3"], c["w5"], c["w7"]]
        at, bs = 0, []
        for w in ws:
            bs.append(c["b"][at:at + w.shape[0]])
            at += w.shape[0]
        y = cr.crpe(x, ws, bs, g, pre)
    dx, = torch.autograd.grad(y, x, c["dy"])
    return y.detach(), dx


def cell_case(F_, g, C, s):
    return {"x": _rand(F_, 1 + g * g, C, seed=9), "drows": _rand(F_ * (g // s) ** 2, s * s * C, seed=10), "g": g, "s": s}


def cell_reference(d, dtype=torch.float64):
    """(rows, dx): the cells and their adjoint by autograd (the prefix row's gradient is 0)."""
    from tests import coat_reference as cr
    c = _cast(d, dtype)
    x = c["x"].clone().requires_grad_(True)
    rows = cr.cells(x, c["g"], c["s"])
    dx, = torch.autograd.grad(rows, x, c["drows"])
    return rows.detach(), dx


def twin_input(label):
    _, side, frames = TWINS[label]
    return _rand(frames, 3, side, side, seed=21)


def full_input():
    return _rand(1, 3, 224, 224, seed=22)


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
    from tests import coat_reference as cr
    out = {"attention": {}, "dwmix": {}, "cells": {}}
    for case in ATTN_CASES:
        d = attn_case(*case)
        r64, r32 = attn_reference(d), attn_reference(d, torch.float32)
        out["attention"][case_key(*case)] = {k: _rel(a, b) for k, a, b in zip(ATTN_PARTS, r32, r64) if not (case[1] == 1 and k == "dk")}
    for case in DW_CASES:
        d = dw_case(*case)
        r64, r32 = dw_reference(d), dw_reference(d, torch.float32)
        out["dwmix"][case_key(*case)] = {"fwd": _rel(r32[0], r64[0]), "bwd": _rel(r32[1], r64[1])}
    for case in CELL_CASES:
        d = cell_case(*case)
        r64, r32 = cell_reference(d), cell_reference(d, torch.float32)
        out["cells"][case_key(*case)] = {"gather": _rel(r32[0], r64[0]), "scatter": _rel(r32[1], r64[1])}
    for label, spec, x in net_cases():
        sd = weights.synthetic_state_dict(spec, 0)
        hooks = [spec.hook_for(d) for d in (1, 2, 3, 4)]
        r64, r32 = cr.CoatReference(spec, sd, hooks), cr.CoatReference(spec, sd, hooks, dtype=torch.float32)
        f64, f32 = r64.forward(x), r32.forward(x)
        hg = [_rand(*f.shape, seed=30 + i) for i, f in enumerate(f64)]
        out[label] = {"hooks": [_rel(a, b) for a, b in zip(f32, f64)], "grad": _rel(r32.backward(hg), r64.backward(hg)),
                      "hook_std": [float(f.std()) for f in f64]}
    label = "coat_test"
    name, side, _ = TWINS[label]
    spec = graphs.build_tiny(name, (side, side))
    sd, vid = weights.synthetic_state_dict(spec, 0), video(*TRAJECTORY_CLIP)
    out["trajectory"] = {label: {}}
    for depth in (1, 2, 3, 4):
        runs = [restate.run_attack([cr.CoatReference(spec, sd, [spec.hook_for(depth)], dtype=dt)], vid, steps=10, step_size=0.005)
                for dt in (torch.float64, torch.float32)]
        c64, c32 = (torch.as_tensor(r["costs"], dtype=torch.float64) for r in runs)
        out["trajectory"][label][str(depth)] = float(((c32 - c64).abs() / c64.abs()).max())
    return out


def main():
    with open(os.path.join(GOLDEN, "timm_coat_keys.json"), "w") as f:
        f.write(compact(keys_fixture()))
    errs = fp32_errors()
    with open(os.path.join(GOLDEN, "coat_fp32_cpu_errors.json"), "w") as f:
        json.dump(errs, f, indent=1)
    print(json.dumps(errs, indent=1))


if __name__ == "__main__":
    main()
