"""Writes the two ConViT fixtures under tests/golden/ (run on the CPU: `python -m tests.make_convit_fixtures`):

  timm_convit_keys.json        name -> {state_dict key: shape} of timm's `ConViT` for the three served names, up to the last block, in
      timm's order.  Generated from the rule restated below -- on its own, not from i2v_amd.graphs -- and checked against timm wherever
      `import timm` works.  Where it does not, the contract is UNCHECKED and the file says so ("checked_against").
  convit_fp32_cpu_errors.json  relative L2 error of the float32 CPU run of tests/convit_reference.py against its float64 run on the inputs
      of tests/test_convit_cpu.py and tests/test_gpu_convit.py: what two correct float32 implementations may differ by.  Never taken
      from the code under test.
"""
import dataclasses
import json
import os

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")

#: name -> (dim, heads); 12 blocks, the first 10 GPSA
TABLE = {"convit_tiny": (192, 4), "convit_small": (432, 9), "convit_base": (768, 16)}
#: attention cases (frames, T, heads, dh, gated): convit_tiny's shape; an odd head count; convit_base's shape; behind the join, without a
#: table; exactly one tile; fewer rows than a tile; three tiles and a one-row tail; dh below the 16-chunk -- and one tile without a table
ATTN_CASES = [(2, 196, 4, 48, True), (1, 196, 9, 48, True), (1, 196, 16, 48, True), (1, 197, 4, 48, False), (3, 16, 2, 8, True),
              (2, 4, 2, 8, True), (2, 49, 4, 48, True), (1, 20, 8, 16, True), (3, 17, 2, 8, False)]
#: the test-size twin: label -> (frame side, frames); 64 gives 16 tokens (one tile), 80 gives 25 (a tile and a tail); 17 / 26 behind the join
TWINS = {"convit_test": (64, 3), "convit_test_80": (80, 2)}
TWIN_HOOKS = [1, 3, 5, 7]
#: the twin with the class token joining one block early (the sensitivity check): its label here
EARLY = "convit_test_early"
#: the full-size models of the GPU test: name -> hooked blocks (depths 1 .. 4), 2 frames
FULL = {"convit_tiny": [2, 5, 8, 11], "convit_small": [2, 5, 8, 11]}

#: `ConvitSpec.workspace_bytes([8], 128)` of convit_base, by hand: weights 4 (768 * 768 + 768 + 196 * 768 + 768 + 9 (4 * 768^2 + 2 * 768 *
#: 3072 + 9 * 768 + 3072) + 9 (16 + 16 * 196 * 196)), saves 9 blocks, scratch and one hook at 196 tokens
WORKSPACE_BASE_D3 = 4 * ((768 * 768 + 768 + 196 * 768 + 768 + 9 * (4 * 768 * 768 + 2 * 768 * 3072 + 9 * 768 + 3072) + 9 * (16 + 16 * 196 * 196))
                         + 9 * 128 * (196 * (5 * 768 + 3072 + 4) + 16 * 196 * 196)
                         + 128 * (196 * (6 * 768 + 3072) + 16 * 196 * 196 + 196 * 768) + 128 * 196 * 768)


def rule(dim, heads):
    """timm/models/convit.py (0.5.0), restated: the model's own parameters first (`cls_token`, `pos_embed`), then `patch_embed.proj`,
    then `blocks.{i}` as `Block` -- norm1, attn, norm2, mlp.  `GPSA` (blocks 0 .. 9): its own parameter gating_param first, then qk, v
    (no bias), proj, pos_proj in the order its constructor makes them; `MHSA` (blocks 10, 11): qkv (no bias), proj."""
    D, H = dim, heads
    out = {"cls_token": [1, 1, D], "pos_embed": [1, 196, D], "patch_embed.proj.weight": [D, 3, 16, 16], "patch_embed.proj.bias": [D]}
    for i in range(12):
        p = f"blocks.{i}."
        out.update({p + "norm1.weight": [D], p + "norm1.bias": [D]})
        if i < 10:
            out.update({p + "attn.gating_param": [H], p + "attn.qk.weight": [2 * D, D], p + "attn.v.weight": [D, D],
                        p + "attn.proj.weight": [D, D], p + "attn.proj.bias": [D], p + "attn.pos_proj.weight": [H, 3], p + "attn.pos_proj.bias": [H]})
        else:
            out.update({p + "attn.qkv.weight": [3 * D, D], p + "attn.proj.weight": [D, D], p + "attn.proj.bias": [D]})
        out.update({p + "norm2.weight": [D], p + "norm2.bias": [D], p + "mlp.fc1.weight": [4 * D, D], p + "mlp.fc1.bias": [4 * D],
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
            got = {k: list(v.shape) for k, v in sd.items() if not k.startswith(("head.", "norm."))}
            assert got == want and list(got) == list(want), (n, sorted(set(got) ^ set(want))[:8])
        checked = f"timm {timm.__version__}"
    return {"checked_against": checked, "follows": "timm 0.5.0 convit.py key layout (restated)", "names": names}


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


def _unif(*shape, seed=0):
    return torch.rand(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


def attn_case(F, T, H, dh, gated=True):
    """The float64 inputs of one attention case: qkv ~ N(0, 1) (logits of O(1) at scale dh^-0.5), dout the output's gradient; gated: c
    uniform on (0.1, 0.9) and a random non-negative table (H, T, T), uniform on (0, 2 / T) so that its rows sum to about one -- not a
    square grid's table, and not normalised: the entry takes any."""
    d = {"qkv": _rand(F, T, 3 * H * dh, seed=1), "dout": _rand(F, T, H * dh, seed=2), "heads": H, "scale": dh ** -0.5, "c": None, "table": None}
    if gated:
        d["c"] = 0.1 + 0.8 * _unif(H, seed=3)
        d["table"] = _unif(H, T, T, seed=4) * (2.0 / T)
    return d


def attn_reference(d, dtype=torch.float64):
    """(out, Ppatch, dqkv) of a case through tests/convit_reference.blend_attention and autograd, in `dtype`."""
    from tests import convit_reference as cr
    c = {k: (v.to(dtype) if torch.is_tensor(v) else v) for k, v in d.items()}
    qkv = c["qkv"].clone().requires_grad_(True)
    out, p = cr.blend_attention(qkv, c["heads"], c["scale"], c["c"], c["table"])
    dqkv = torch.autograd.grad(out, qkv, c["dout"])[0]
    return out.detach(), p.detach(), dqkv


def case_key(F, T, H, dh, gated=True):
    return f"{F}x{T}x{H}x{dh}" + ("" if gated else "-plain")


def twin_input(label):
    side, frames = TWINS[label]
    return _rand(frames, 3, side, side, seed=21)


def early_join(spec, sd):
    """The twin with the class token joining one block early: (spec with local_blocks - 1, its state dict).  The block that moves behind
    the join keeps its weights -- `attn.qk.weight` and `attn.v.weight` stacked are its `attn.qkv.weight` -- and loses its gate."""
    b = spec.local_blocks - 1
    p = f"blocks.{b}.attn."
    out = {k: v for k, v in sd.items() if not k.startswith(p) or k.startswith(p + "proj.")}
    out[p + "qkv.weight"] = torch.cat([sd[p + "qk.weight"], sd[p + "v.weight"]], 0)
    s2 = dataclasses.replace(spec, local_blocks=b, hooks=dict(spec.hooks))
    return s2, {k: out[k] for k in s2.param_shapes()}


def fp32_errors():
    from i2v_amd import graphs, weights
    from tests import convit_reference as cr
    out = {"attention": {}}
    for case in ATTN_CASES:
        d = attn_case(*case)
        o64, p64, g64 = attn_reference(d)
        o32, p32, g32 = attn_reference(d, torch.float32)
        out["attention"][case_key(*case)] = {"fwd": _rel(o32, o64), "probs": _rel(p32, p64), "bwd": _rel(g32, g64)}
    cases = []
    for label, (side, _) in TWINS.items():
        spec = graphs.build_tiny("convit_tiny", (side, side))
        cases.append((label, spec, weights.synthetic_state_dict(spec, 0), twin_input(label), TWIN_HOOKS))
    spec = graphs.build_tiny("convit_tiny", (64, 64))
    cases.append((EARLY, *early_join(spec, weights.synthetic_state_dict(spec, 0)), twin_input("convit_test"), TWIN_HOOKS))
    for n, hooks in FULL.items():
        spec = graphs.build(n)
        cases.append((n, spec, weights.synthetic_state_dict(spec, 0), _rand(2, 3, 224, 224, seed=22), hooks))
    for label, spec, sd, x, hooks in cases:
        r64, r32 = cr.ConvitReference(spec, sd, hooks), cr.ConvitReference(spec, sd, hooks, dtype=torch.float32)
        f64, f32 = r64.forward(x), r32.forward(x)
        hg = [_rand(*f.shape, seed=30 + i) for i, f in enumerate(f64)]
        out[label] = {"hooks": [_rel(a, b) for a, b in zip(f32, f64)], "grad": _rel(r32.backward(hg), r64.backward(hg)),
                      "hook_std": [float(f.std()) for f in f64]}
    return out


def main():
    with open(os.path.join(GOLDEN, "timm_convit_keys.json"), "w") as f:
        f.write(compact(keys_fixture()))
    errs = fp32_errors()
    with open(os.path.join(GOLDEN, "convit_fp32_cpu_errors.json"), "w") as f:
        json.dump(errs, f, indent=1)
    print(json.dumps(errs, indent=1))


if __name__ == "__main__":
    main()
