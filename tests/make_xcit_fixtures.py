"""Writes the two XCiT fixtures under tests/golden/ (run on the CPU: `python -m tests.make_xcit_fixtures`):

  timm_xcit_keys.json        name -> {state_dict key: shape} of timm's `XCiT` for the seven served architectures, up to the last
      cross-covariance block, in timm's order (each `_dist` name has its base name's keys).  Generated from the rule restated below -- on
      its own, not from i2v_amd.graphs -- and checked against timm wherever `import timm` works.  Where it does not, the contract is
      UNCHECKED and the file says so ("checked_against").
  xcit_fp32_cpu_errors.json  relative L2 error of the float32 CPU run of the references (tests/xcit_reference.py and the entry
      definitions below) against their float64 run on the inputs of tests/test_xcit_cpu.py and tests/test_gpu_xcit.py: what two correct
      float32 implementations may differ by.  Never taken from the code under test.
"""
import json
import os

import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")

#: name -> (dim, blocks, heads)
TABLE = {"xcit_nano_12_p16_224": (128, 12, 4), "xcit_tiny_12_p16_224": (192, 12, 4), "xcit_tiny_24_p16_224": (192, 24, 4),
         "xcit_small_12_p16_224": (384, 12, 8), "xcit_small_24_p16_224": (384, 24, 8), "xcit_medium_24_p16_224": (512, 24, 8),
         "xcit_large_24_p16_224": (768, 24, 16)}
#: cross-covariance attention cases (frames, T, heads, dh, kind): the tiny / small / large shape; the medium shape (dh 64, the widest
#: served); the nano shape; one token tile and fewer tokens than an MFMA step's four; the odd twin's shape; a single token; dh no multiple
#: of 16; T beyond any whole-head staging.  kind "hot": every temperature 30, so the softmax needs its max; "zero": column 3 of q and
#: column 5 of k of head 0 are all zero -- row 3 of A is uniform, and the reference's own gradient is of order 1 / eps and is not compared
ATTN_CASES = [(2, 196, 4, 48, ""), (1, 196, 8, 64, ""), (1, 196, 4, 32, ""), (3, 16, 2, 8, ""), (2, 4, 2, 8, ""), (2, 25, 2, 24, ""),
              (1, 1, 2, 8, ""), (1, 17, 1, 20, ""), (1, 784, 4, 48, ""), (2, 25, 2, 24, "hot"), (1, 17, 1, 20, "zero")]
#: depthwise cases: plane side x channels x variant (which of the optional operands are given)
DW3_PLANES, DW3_CHANNELS = (1, 2, 5, 14), (4, 20, 192)
DW3_VARIANTS = {"plain": (), "transform": ("t",), "residual": ("r",), "multiply": ("m",), "all": ("t", "r", "m")}
DW3_CASES = [(p, c, v) for p in DW3_PLANES for c in DW3_CHANNELS for v in DW3_VARIANTS]
#: stem gather / scatter cases (plane side, channels, image layout): 5 -> 3 and 8 -> 4; 3 channels of an image, a width that is no
#: multiple of 4, one that is
STEM_CASES = [(p, c, nchw) for p in (5, 8) for c, nchw in ((3, True), (6, False), (8, False))]
#: the test-size twins: label -> (frame side, frames)
TWINS = {"xcit_test": (64, 3), "xcit_test_80": (80, 2)}
TWIN_HOOKS = [1, 3, 5, 7]
#: the full-size models of the GPU test: name -> hooked blocks (depths 1 .. 4), 2 frames
FULL = {"xcit_nano_12_p16_224": [2, 5, 8, 11], "xcit_tiny_12_p16_224": [2, 5, 8, 11]}
#: what the reference can leave out, one fold each (tests/xcit_reference.XcitReference `skip`)
FOLDS = ("stem_bn", "pos", "gamma1", "gamma2", "gamma3", "lpi_bn", "temperature")

#: `XcitSpec.workspace_bytes([8], 128)` of xcit_small_12_p16_224 (dim 384, 8 heads of 48, 9 blocks run), by hand: the stem weights and the
#: position table, 9 blocks of 12 dim^2 + 37 dim + heads + two mirrored filters; at 128 frames the stem's rows (stage 2: 56^2 x 9 x 48
#: is the largest) and the saved planes of its first three stages; 9 blocks of saves; the shared scratch; one hook
WORKSPACE_SMALL_D3 = 4 * ((48 * 27 + 48 + 96 * 432 + 96 + 192 * 864 + 192 + 384 * 1728 + 384) + 196 * 384
                          + 9 * (12 * 384 * 384 + 37 * 384 + 8 + 18 * 384)
                          + 128 * (56 * 56 * 9 * 48 + 2 * (112 * 112 * 48 + 56 * 56 * 96 + 28 * 28 * 192))
                          + 9 * 128 * (196 * (11 * 384 + 6) + 8 * 48 * 98)
                          + 128 * 196 * (6 * 384 + 1536) + 128 * 196 * 384)


def rule(dim, blocks, heads):
    """timm/models/xcit.py (0.5.0), restated, without `cls_token`, `cls_attn_blocks.*`, `norm.*`, `head.*` and the BatchNorms'
    `num_batches_tracked`: `patch_embed.proj` is a Sequential of conv3x3 (itself Sequential(Conv2d without bias, BatchNorm2d)) at 0, 2, 4,
    6 with GELUs between; `pos_embeder.token_projection` is a 1 x 1 Conv2d from 2 x 32 Fourier features; `blocks.{i}` is `XCABlock`: its
    own parameters gamma1, gamma3, gamma2 as its constructor makes them, then norm1, attn (`XCA`: its own `temperature` (heads, 1, 1), qkv
    with bias, proj), norm3, local_mp (`LPI`: conv1, bn, conv2), norm2, mlp."""
    D, H = dim, heads
    cs = [3, D // 8, D // 4, D // 2, D]
    out = {}
    for k in range(4):
        p = f"patch_embed.proj.{2 * k}."
        out[p + "0.weight"] = [cs[k + 1], cs[k], 3, 3]
        for n in ("weight", "bias", "running_mean", "running_var"):
            out[p + "1." + n] = [cs[k + 1]]
    out["pos_embeder.token_projection.weight"] = [D, 64, 1, 1]
    out["pos_embeder.token_projection.bias"] = [D]
    for i in range(blocks):
        p = f"blocks.{i}."
        out.update({p + "gamma1": [D], p + "gamma3": [D], p + "gamma2": [D], p + "norm1.weight": [D], p + "norm1.bias": [D],
                    p + "attn.temperature": [H, 1, 1], p + "attn.qkv.weight": [3 * D, D], p + "attn.qkv.bias": [3 * D],
                    p + "attn.proj.weight": [D, D], p + "attn.proj.bias": [D], p + "norm3.weight": [D], p + "norm3.bias": [D],
                    p + "local_mp.conv1.weight": [D, 1, 3, 3], p + "local_mp.conv1.bias": [D], p + "local_mp.bn.weight": [D],
                    p + "local_mp.bn.bias": [D], p + "local_mp.bn.running_mean": [D], p + "local_mp.bn.running_var": [D],
                    p + "local_mp.conv2.weight": [D, 1, 3, 3], p + "local_mp.conv2.bias": [D], p + "norm2.weight": [D], p + "norm2.bias": [D],
                    p + "mlp.fc1.weight": [4 * D, D], p + "mlp.fc1.bias": [4 * D], p + "mlp.fc2.weight": [D, 4 * D], p + "mlp.fc2.bias": [D]})
    return out


def keys_fixture():
    names = {n: rule(*TABLE[n]) for n in TABLE}
    checked = "unchecked: timm does not import here"
    try:
        import timm
    except ImportError:
        timm = None
    if timm is not None:
        for n, want in names.items():
            for name in (n, n + "_dist"):
                sd = timm.create_model(name, pretrained=False).state_dict()
                got = {k.replace("pos_embed.", "pos_embeder."): list(v.shape) for k, v in sd.items()
                       if not k.startswith(("cls_token", "cls_attn_blocks.", "head.", "norm.")) and not k.endswith("num_batches_tracked")}
                assert got == want and list(got) == list(want), (name, sorted(set(got) ^ set(want))[:8])
        checked = f"timm {timm.__version__}"
    return {"checked_against": checked, "follows": "timm 0.5.0 xcit.py key layout (restated)",
            "dist": "each name + '_dist' has the keys of the name", "names": names}


def compact(fx):
    """One block per line; the stem keys one module per line: the file is the contract, read by eye, and stays under the size limit."""
    head = {k: v for k, v in fx.items() if k != "names"}
    out = ["{"] + [f" {json.dumps(k)}: {json.dumps(v)}," for k, v in head.items()] + [' "names": {']
    for i, (n, keys) in enumerate(fx["names"].items()):
        out.append(f"  {json.dumps(n)}: {{")
        lines, cur, tag = [], [], None
        for k, v in keys.items():
            t = ".".join(k.split(".")[:3 if k.startswith("patch_embed") else 2])
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


def _unif(*shape, seed=0):
    return torch.rand(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


def _cast(d, dtype):
    return {k: (v.to(dtype) if torch.is_tensor(v) else v) for k, v in d.items()}


# ---- cross-covariance attention ------------------------------------------------------------------------------------------------------
def attn_case(F_, T, H, dh, kind=""):
    """The float64 inputs of one case: qkv ~ N(0, 1), dout the output's gradient, temperature uniform on (0.5, 4) (timm starts it at 1)."""
    d = {"qkv": _rand(F_, T, 3 * H * dh, seed=1), "dout": _rand(F_, T, H * dh, seed=2), "heads": H, "temperature": 0.5 + 3.5 * _unif(H, seed=3)}
    if kind == "hot":
        d["temperature"] = torch.full((H,), 30.0, dtype=torch.float64)
    if kind == "zero":
        d["qkv"][:, :, 3] = 0.0                     # q, head 0, column 3
        d["qkv"][:, :, H * dh + 5] = 0.0            # k, head 0, column 5
    return d


def attn_reference(d, dtype=torch.float64):
    """(out, A, dqkv) of a case through tests/xcit_reference.xca_core (timm's literal arithmetic) and autograd, in `dtype`."""
    from tests import xcit_reference as xr
    c = _cast(d, dtype)
    qkv = c["qkv"].clone().requires_grad_(True)
    out, a = xr.xca_core(qkv, c["heads"], c["temperature"])
    dqkv = torch.autograd.grad(out, qkv, c["dout"])[0]
    return out.detach(), a.detach(), dqkv


def case_key(F_, T, H, dh, kind=""):
    return f"{F_}x{T}x{H}x{dh}" + (f"-{kind}" if kind else "")


# ---- the depthwise launch ------------------------------------------------------------------------------------------------------------
def dw3_case(P, C, variant):
    on = DW3_VARIANTS[variant]
    d = {"x": _rand(2, P, P, C, seed=5), "w": _rand(9, C, seed=6) / 3.0, "b": 0.1 * _rand(C, seed=7), "ta": None, "ts": None, "add": None,
         "ma": None, "mu": None}
    if "t" in on:
        d["ta"], d["ts"] = 0.5 + _unif(C, seed=8), 0.5 * _rand(C, seed=9)
    if "r" in on:
        d["add"] = _rand(2, P, P, C, seed=10)
    if "m" in on:
        d["ma"], d["mu"] = 0.5 + _unif(C, seed=11), _rand(2, P, P, C, seed=12)
    return d


def gelu_grad(u):
    u = u.detach().clone().requires_grad_(True)
    return torch.autograd.grad(F.gelu(u).sum(), u)[0]


def dw3_reference(d, dtype=torch.float64):
    """The entry's definition through `conv2d`: the transform is applied before the zero padding."""
    c = _cast(d, dtype)
    C = c["x"].shape[-1]
    z = c["x"].permute(0, 3, 1, 2)
    if c["ta"] is not None:
        z = F.gelu(z) * c["ta"].view(1, C, 1, 1) + c["ts"].view(1, C, 1, 1)
    y = F.conv2d(z, c["w"].t().reshape(C, 1, 3, 3), c["b"], padding=1, groups=C).permute(0, 2, 3, 1)
    if c["add"] is not None:
        y = y + c["add"]
    if c["ma"] is not None:
        y = y * (c["ma"] * gelu_grad(c["mu"]))
    return y.contiguous()


def dw3_key(P, C, variant):
    return f"{P}x{P}x{C}-{variant}"


# ---- the stem pair -------------------------------------------------------------------------------------------------------------------
def stem_case(P, C, nchw):
    Po = (P + 1) // 2
    return {"src": _rand(2, C, P, P, seed=13) if nchw else _rand(2, P, P, C, seed=13), "drows": _rand(2 * Po * Po, 9 * C, seed=14),
            "pre": None if nchw else _rand(2, P, P, C, seed=15), "nchw": nchw}


def gather_reference(src, nchw):
    """rows (n Ho Wo, 9 C), column (3 ky + kx) C + c, through `unfold` (whose columns are c 9 + tap)."""
    x = src if nchw else src.permute(0, 3, 1, 2)
    n, C = x.shape[:2]
    u = F.unfold(x, 3, padding=1, stride=2)
    return u.reshape(n, C, 9, -1).permute(0, 3, 2, 1).reshape(-1, 9 * C)


def scatter_reference(d, dtype=torch.float64):
    """The transpose of the gather by autograd, times gelu'(pre) where the case has one."""
    c = _cast(d, dtype)
    src = torch.zeros_like(c["src"]).requires_grad_(True)
    g = torch.autograd.grad(gather_reference(src, c["nchw"]), src, c["drows"])[0]
    return g if c["pre"] is None else g * gelu_grad(c["pre"])


def stem_key(P, C, nchw):
    return f"{P}x{P}x{C}" + ("-image" if nchw else "")


def twin_input(label):
    side, frames = TWINS[label]
    return _rand(frames, 3, side, side, seed=21)


def fp32_errors():
    from i2v_amd import graphs, weights
    from tests import xcit_reference as xr
    out = {"attention": {}, "dw3": {}, "scatter": {}}
    for case in ATTN_CASES:
        d = attn_case(*case)
        o64, p64, g64 = attn_reference(d)
        o32, p32, g32 = attn_reference(d, torch.float32)
        out["attention"][case_key(*case)] = {"fwd": _rel(o32, o64), "probs": _rel(p32, p64), "bwd": _rel(g32, g64)}
    for case in DW3_CASES:
        d = dw3_case(*case)
        out["dw3"][dw3_key(*case)] = _rel(dw3_reference(d, torch.float32), dw3_reference(d))
    for case in STEM_CASES:
        d = stem_case(*case)
        out["scatter"][stem_key(*case)] = _rel(scatter_reference(d, torch.float32), scatter_reference(d))
    cases = []
    for label, (side, _) in TWINS.items():
        spec = graphs.build_tiny("xcit_tiny_12_p16_224", (side, side))
        cases.append((label, spec, weights.synthetic_state_dict(spec, 0), twin_input(label), TWIN_HOOKS))
    for n, hooks in FULL.items():
        spec = graphs.build(n)
        cases.append((n, spec, weights.synthetic_state_dict(spec, 0), _rand(2, 3, 224, 224, seed=22), hooks))
    for label, spec, sd, x, hooks in cases:
        r64, r32 = xr.XcitReference(spec, sd, hooks), xr.XcitReference(spec, sd, hooks, dtype=torch.float32)
        f64, f32 = r64.forward(x), r32.forward(x)
        hg = [_rand(*f.shape, seed=30 + i) for i, f in enumerate(f64)]
        out[label] = {"hooks": [_rel(a, b) for a, b in zip(f32, f64)], "grad": _rel(r32.backward(hg), r64.backward(hg)),
                      "hook_std": [float(f.std()) for f in f64]}
    return out


def main():
    with open(os.path.join(GOLDEN, "timm_xcit_keys.json"), "w") as f:
        f.write(compact(keys_fixture()))
    errs = fp32_errors()
    with open(os.path.join(GOLDEN, "xcit_fp32_cpu_errors.json"), "w") as f:
        json.dump(errs, f, indent=1)
    print(json.dumps(errs, indent=1))


if __name__ == "__main__":
    main()
