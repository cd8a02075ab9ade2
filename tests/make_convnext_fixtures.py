"""Writes the two ConvNeXt fixtures under tests/golden/ (run on the CPU: `python -m tests.make_convnext_fixtures`):

  timm_convnext_keys.json        name -> {state_dict key: shape} of timm's `ConvNeXt` for the four served names, up to the last block.
      Generated from the rule restated below -- on its own, not from i2v_amd.graphs -- and checked against timm wherever `import timm`
      works.  Where it does not, the contract is UNCHECKED and the file says so ("checked_against").
  convnext_fp32_cpu_errors.json  relative L2 error of the float32 CPU run of tests/convnext_reference.py against its float64 run on the
      inputs of tests/test_gpu_convnext.py: what two correct float32 implementations may differ by.  Never taken from the code under test.
"""
import json
import os

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")

TABLE = {"convnext_tiny": (96, (3, 3, 9, 3)), "convnext_small": (96, (3, 3, 27, 3)), "convnext_base": (128, (3, 3, 27, 3)),
         "convnext_large": (192, (3, 3, 27, 3))}
#: node cases of the GPU test: (C, H, W)
NODE_CASES = [(96, 7, 7), (8, 2, 2), (20, 5, 9), (6, 14, 14), (192, 14, 14)]


def rule(dim, depths):
    """timm/models/convnext.py (0.6.x key layout: `stem`, `stages.{i}.downsample`, `stages.{i}.blocks.{j}` with `conv_dw`, `norm`, `mlp.fc1`,
    `mlp.fc2`, `gamma`), restated."""
    out = {"stem.0.weight": [dim, 3, 4, 4], "stem.0.bias": [dim], "stem.1.weight": [dim], "stem.1.bias": [dim]}
    for i, d in enumerate(depths):
        C = dim << i
        if i > 0:
            p = f"stages.{i}.downsample."
            out.update({p + "0.weight": [C // 2], p + "0.bias": [C // 2], p + "1.weight": [C, C // 2, 2, 2], p + "1.bias": [C]})
        for j in range(d):
            p = f"stages.{i}.blocks.{j}."
            out.update({p + "conv_dw.weight": [C, 1, 7, 7], p + "conv_dw.bias": [C], p + "norm.weight": [C], p + "norm.bias": [C],
                        p + "mlp.fc1.weight": [4 * C, C], p + "mlp.fc1.bias": [4 * C], p + "mlp.fc2.weight": [C, 4 * C],
                        p + "mlp.fc2.bias": [C], p + "gamma": [C]})
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
            sd = timm.create_model(n, pretrained=False).state_dict()
            got = {k: list(v.shape) for k, v in sd.items() if not k.startswith(("head.", "norm_pre."))}
            assert got == want, (n, sorted(set(got) ^ set(want))[:8])
        checked = f"timm {timm.__version__}"
    return {"checked_against": checked, "follows": "timm 0.6.x convnext.py key layout (restated)", "names": names}


def compact(fx):
    """One key per line; runs of blocks that differ only in their index stay written out: the file is the contract, read by eye."""
    head = {k: v for k, v in fx.items() if k != "names"}
    out = ["{"] + [f" {json.dumps(k)}: {json.dumps(v)}," for k, v in head.items()] + [' "names": {']
    for i, (n, keys) in enumerate(fx["names"].items()):
        out.append(f"  {json.dumps(n)}: {{")
        out += [f"   {json.dumps(k)}: {json.dumps(v)}" + ("," if j + 1 < len(keys) else "") for j, (k, v) in enumerate(keys.items())]
        out.append("  }" + ("," if i + 1 < len(fx["names"]) else ""))
    return "\n".join(out + [" }", "}"]) + "\n"


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def _rand(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


def fp32_errors():
    from i2v_amd import graphs, weights
    from tests import convnext_reference as cr
    out = {"nodes": {}}
    for C, H, W in NODE_CASES:
        for N in (1, 3):
            x, w, b, dy = _rand(N, H, W, C, seed=1), _rand(49, C, seed=2) / 7, _rand(C, seed=3), _rand(N, H, W, C, seed=4)
            xr = x.clone().requires_grad_(True)
            y = cr.dwconv_token_major(xr, w, b)
            gx = torch.autograd.grad(y, xr, dy)[0]
            xf = x.float().requires_grad_(True)
            yf = cr.dwconv_token_major(xf, w.float(), b.float())
            gf = torch.autograd.grad(yf, xf, dy.float())[0]
            out["nodes"][f"{C}x{H}x{W}x{N}"] = {"fwd": _rel(yf.detach(), y.detach()), "bwd": _rel(gf, gx)}
    for label, spec, x, stages in (("convnext_test", graphs.build_tiny("convnext_tiny", (64, 64)), _rand(3, 3, 64, 64, seed=21), [0, 1, 2, 3]),
                                   ("convnext_tiny", graphs.build("convnext_tiny"), _rand(2, 3, 224, 224, seed=22), [2])):
        sd = weights.synthetic_state_dict(spec, 0)
        r64, r32 = cr.ConvNextReference(spec, sd, stages), cr.ConvNextReference(spec, sd, stages, dtype=torch.float32)
        f64, f32 = r64.forward(x), r32.forward(x)
        hg = [_rand(*f.shape, seed=30 + i) for i, f in enumerate(f64)]
        out[label] = {"hooks": [_rel(a, b) for a, b in zip(f32, f64)], "grad": _rel(r32.backward(hg), r64.backward(hg)),
                      "hook_std": [float(f.std()) for f in f64]}
    return out


def main():
    with open(os.path.join(GOLDEN, "timm_convnext_keys.json"), "w") as f:
        f.write(compact(keys_fixture()))
    errs = fp32_errors()
    with open(os.path.join(GOLDEN, "convnext_fp32_cpu_errors.json"), "w") as f:
        json.dump(errs, f, indent=1)
    print(json.dumps({k: v for k, v in errs.items() if k != "nodes"}, indent=1))
    print("nodes: max fwd", max(v["fwd"] for v in errs["nodes"].values()), "max bwd", max(v["bwd"] for v in errs["nodes"].values()))


if __name__ == "__main__":
    main()
