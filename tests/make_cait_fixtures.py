"""Writes the two CaiT fixtures under tests/golden/ (run on the CPU: `python -m tests.make_cait_fixtures`):

  timm_cait_keys.json        name -> {state_dict key: shape} of timm's `Cait` for the three served names, up to the last self-attention
      block, in timm's order.  Generated from the rule restated below -- on its own, not from i2v_amd.graphs -- and checked against timm
      wherever `import timm` works.  Where it does not, the contract is UNCHECKED and the file says so ("checked_against").
  cait_fp32_cpu_errors.json  relative L2 error of the float32 CPU run of tests/cait_reference.py against its float64 run on the inputs of
      tests/test_cait_cpu.py and tests/test_gpu_cait.py: what two correct float32 implementations may differ by.  Never taken from the
      code under test.
"""
import json
import os

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")

#: name -> (dim, self-attention blocks, heads)
TABLE = {"cait_xxs24_224": (192, 24, 4), "cait_xxs36_224": (192, 36, 4), "cait_s24_224": (384, 24, 8)}
#: attention cases (frames, T, heads, dh): the xxs shape with its 4-row tail; the s24 shape, the largest LDS tile; exactly one tile; fewer
#: rows than a tile; odd T, so padded probability rows; one tile plus four rows
ATTN_CASES = [(2, 196, 4, 48), (1, 196, 8, 48), (3, 16, 2, 8), (2, 4, 2, 8), (2, 49, 4, 48), (1, 20, 8, 16)]
#: the test-size twin: label -> (frame side, frames); 64 gives 16 tokens (one tile), 80 gives 25 (a tile and a tail)
TWINS = {"cait_test": (64, 3), "cait_test_80": (80, 2)}
TWIN_HOOKS = [1, 3, 5, 7]
#: the full-size models of the GPU test: name -> hooked blocks (depths 1 .. 4), 2 frames
FULL = {"cait_xxs24_224": [5, 11, 17, 23], "cait_s24_224": [5, 11, 17, 23]}


def rule(dim, blocks, heads):
    """timm/models/cait.py (0.5.0), restated: the model's own parameters first (`cls_token`, not listed here, and `pos_embed`), then
    `patch_embed.proj`, then `blocks.{i}` as `LayerScale_Block` -- its own parameters gamma_1, gamma_2 first, then norm1, attn
    (`TalkingHeadAttn`: qkv, proj, proj_l, proj_w in the order its constructor makes them), norm2, mlp."""
    D, H = dim, heads
    out = {"pos_embed": [1, 196, D], "patch_embed.proj.weight": [D, 3, 16, 16], "patch_embed.proj.bias": [D]}
    for i in range(blocks):
        p = f"blocks.{i}."
        out.update({p + "gamma_1": [D], p + "gamma_2": [D], p + "norm1.weight": [D], p + "norm1.bias": [D],
                    p + "attn.qkv.weight": [3 * D, D], p + "attn.qkv.bias": [3 * D], p + "attn.proj.weight": [D, D], p + "attn.proj.bias": [D],
                    p + "attn.proj_l.weight": [H, H], p + "attn.proj_l.bias": [H], p + "attn.proj_w.weight": [H, H], p + "attn.proj_w.bias": [H],
                    p + "norm2.weight": [D], p + "norm2.bias": [D], p + "mlp.fc1.weight": [4 * D, D], p + "mlp.fc1.bias": [4 * D],
                    p + "mlp.fc2.weight": [D, 4 * D], p + "mlp.fc2.bias": [D]})
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
            got = {k: list(v.shape) for k, v in sd.items() if k != "cls_token" and not k.startswith(("blocks_token_only.", "head.", "norm."))}
            assert got == want and list(got) == list(want), (n, sorted(set(got) ^ set(want))[:8])
        checked = f"timm {timm.__version__}"
    return {"checked_against": checked, "follows": "timm 0.5.0 cait.py key layout (restated)", "names": names}


def compact(fx):
    """One block per line; the stem keys one per line: the file is the contract, read by eye, and stays well under the size limit."""
    head = {k: v for k, v in fx.items() if k != "names"}
    out = ["{"] + [f" {json.dumps(k)}: {json.dumps(v)}," for k, v in head.items()] + [' "names": {']
    for i, (n, keys) in enumerate(fx["names"].items()):
        out.append(f"  {json.dumps(n)}: {{")
        lines, cur, tag = [], [], None
        for k, v in keys.items():
            t = k.split(".")[1] if k.startswith("blocks.") else k
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


def attn_case(F, T, H, dh):
    """The float64 inputs of one attention case: qkv ~ N(0, 1) (logits of O(1) at scale dh^-0.5), dout the output's gradient, the two
    head mixes as identity + 0.25 N(0, 1) with biases 0.5 N(0, 1) and 0.02 N(0, 1)."""
    return {"qkv": _rand(F, T, 3 * H * dh, seed=1), "dout": _rand(F, T, H * dh, seed=2), "wl": torch.eye(H, dtype=torch.float64) + 0.25 * _rand(H, H, seed=3),
            "bl": 0.5 * _rand(H, seed=4), "ww": torch.eye(H, dtype=torch.float64) + 0.25 * _rand(H, H, seed=5), "bw": 0.02 * _rand(H, seed=6),
            "heads": H, "scale": dh ** -0.5}


def attn_reference(d, dtype=torch.float64):
    """(out, probs, dqkv) of a case through tests/cait_reference.talking_heads and autograd, in `dtype`."""
    from tests import cait_reference as cr
    c = {k: (v.to(dtype) if torch.is_tensor(v) else v) for k, v in d.items()}
    qkv = c["qkv"].clone().requires_grad_(True)
    out, p = cr.talking_heads(qkv, c["heads"], c["scale"], c["wl"], c["bl"], c["ww"], c["bw"])
    dqkv = torch.autograd.grad(out, qkv, c["dout"])[0]
    return out.detach(), p.detach(), dqkv


def case_key(F, T, H, dh):
    return f"{F}x{T}x{H}x{dh}"


def twin_input(label):
    side, frames = TWINS[label]
    return _rand(frames, 3, side, side, seed=21)


def fp32_errors():
    from i2v_amd import graphs, weights
    from tests import cait_reference as cr
    out = {"attention": {}}
    for case in ATTN_CASES:
        d = attn_case(*case)
        o64, p64, g64 = attn_reference(d)
        o32, p32, g32 = attn_reference(d, torch.float32)
        out["attention"][case_key(*case)] = {"fwd": _rel(o32, o64), "probs": _rel(p32, p64), "bwd": _rel(g32, g64)}
    cases = [(label, graphs.build_tiny("cait_s24_224", (side, side)), twin_input(label), TWIN_HOOKS) for label, (side, _) in TWINS.items()]
    cases += [(n, graphs.build(n), _rand(2, 3, 224, 224, seed=22), hooks) for n, hooks in FULL.items()]
    for label, spec, x, hooks in cases:
        sd = weights.synthetic_state_dict(spec, 0)
        r64, r32 = cr.CaitReference(spec, sd, hooks), cr.CaitReference(spec, sd, hooks, dtype=torch.float32)
        f64, f32 = r64.forward(x), r32.forward(x)
        hg = [_rand(*f.shape, seed=30 + i) for i, f in enumerate(f64)]
        out[label] = {"hooks": [_rel(a, b) for a, b in zip(f32, f64)], "grad": _rel(r32.backward(hg), r64.backward(hg)),
                      "hook_std": [float(f.std()) for f in f64]}
    return out


def main():
    with open(os.path.join(GOLDEN, "timm_cait_keys.json"), "w") as f:
        f.write(compact(keys_fixture()))
    errs = fp32_errors()
    with open(os.path.join(GOLDEN, "cait_fp32_cpu_errors.json"), "w") as f:
        json.dump(errs, f, indent=1)
    print(json.dumps(errs, indent=1))


if __name__ == "__main__":
    main()
