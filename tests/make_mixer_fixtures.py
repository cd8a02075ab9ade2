"""Writes the two MLP-Mixer / ResMLP fixtures under tests/golden/ (run on the CPU: `python -m tests.make_mixer_fixtures`):

  timm_mixer_keys.json        name -> {state_dict key: shape} of timm's `MlpMixer` for the twelve served names, up to the last block, in
      timm's order.  Generated from the rule restated below -- on its own, not from i2v_amd.graphs -- and checked against timm wherever
      `import timm` works.  Where it does not, the contract is UNCHECKED and the file says so ("checked_against").
  mixer_fp32_cpu_errors.json  relative L2 error of the float32 CPU run of tests/mixer_reference.py against its float64 run on the inputs
      of tests/test_mixer_cpu.py and tests/test_gpu_mixer.py: what two correct float32 implementations may differ by.  Never taken from
      the code under test.
"""
import json
import os

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")

#: name -> (kind, patch, dim, blocks)
TABLE = {"mixer_s32_224": ("mixer", 32, 512, 8), "mixer_s16_224": ("mixer", 16, 512, 8), "mixer_b32_224": ("mixer", 32, 768, 12),
         "mixer_b16_224": ("mixer", 16, 768, 12), "mixer_l32_224": ("mixer", 32, 1024, 24), "mixer_l16_224": ("mixer", 16, 1024, 24),
         "resmlp_12_224": ("resmlp", 16, 384, 12), "resmlp_24_224": ("resmlp", 16, 384, 24), "resmlp_36_224": ("resmlp", 16, 384, 36),
         "resmlp_12_distilled_224": ("resmlp", 16, 384, 12), "resmlp_24_distilled_224": ("resmlp", 16, 384, 24),
         "resmlp_36_distilled_224": ("resmlp", 16, 384, 36)}
#: token-launch cases with a hidden layer, (S, Sh, C): the smallest shapes that reach each tail (the issue's list)
HIDDEN_CASES = [(4, 2, 4), (9, 5, 12), (16, 16, 32), (49, 24, 68), (196, 98, 36), (196, 384, 64), (196, 512, 32)]
#: ... and without one, (S, C), run with in_scale / in_shift / out_scale
LINEAR_CASES = [(16, 8), (196, 388)]
#: the full-size models of the GPU test: name -> hooked blocks (depths 2 and 4), 2 frames
FULL = {"mixer_b16_224": [5, 11], "resmlp_12_224": [5, 11]}


def rule(kind, patch, dim, blocks):
    """timm/models/mlp_mixer.py (0.5.0: `stem.proj`, `blocks.{i}` as `MixerBlock` -- norm1, mlp_tokens, norm2, mlp_channels -- or `ResBlock`
    -- the parameters ls1, ls2 first, then norm1 (Affine: alpha, beta), linear_tokens, norm2, mlp_channels), restated."""
    D, S = dim, (224 // patch) ** 2
    out = {"stem.proj.weight": [D, 3, patch, patch], "stem.proj.bias": [D]}
    for i in range(blocks):
        p = f"blocks.{i}."
        if kind == "mixer":
            Sh = D // 2
            out.update({p + "norm1.weight": [D], p + "norm1.bias": [D], p + "mlp_tokens.fc1.weight": [Sh, S], p + "mlp_tokens.fc1.bias": [Sh],
                        p + "mlp_tokens.fc2.weight": [S, Sh], p + "mlp_tokens.fc2.bias": [S], p + "norm2.weight": [D], p + "norm2.bias": [D]})
        else:
            out.update({p + "ls1": [D], p + "ls2": [D], p + "norm1.alpha": [1, 1, D], p + "norm1.beta": [1, 1, D],
                        p + "linear_tokens.weight": [S, S], p + "linear_tokens.bias": [S], p + "norm2.alpha": [1, 1, D],
                        p + "norm2.beta": [1, 1, D]})
        out.update({p + "mlp_channels.fc1.weight": [4 * D, D], p + "mlp_channels.fc1.bias": [4 * D], p + "mlp_channels.fc2.weight": [D, 4 * D],
                    p + "mlp_channels.fc2.bias": [D]})
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
    return {"checked_against": checked, "follows": "timm 0.5.0 mlp_mixer.py key layout (restated)", "names": names}


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


def token_case(S, Sh, C, F):
    """The float64 inputs of one token-launch case: dict of z, residual, g (the output's gradient), add (an addend of the input
    gradient), the weights at fan_in^-0.5, and -- without a hidden layer -- the three per-channel arrays, well away from 1 and 0."""
    d = {"z": _rand(F, S, C, seed=1), "residual": _rand(F, S, C, seed=2), "g": _rand(F, S, C, seed=3), "add": _rand(F, S, C, seed=4)}
    if Sh:
        d.update(w1=_rand(Sh, S, seed=5) * S ** -0.5, b1=0.5 * _rand(Sh, seed=6), w2=_rand(S, Sh, seed=7) * Sh ** -0.5, b2=0.5 * _rand(S, seed=8),
                 in_scale=None, in_shift=None, out_scale=None)
    else:
        d.update(w1=_rand(S, S, seed=5) * S ** -0.5, b1=0.5 * _rand(S, seed=6), w2=None, b2=None,
                 in_scale=0.5 + torch.rand(C, generator=torch.Generator().manual_seed(9), dtype=torch.float64),
                 in_shift=0.3 * _rand(C, seed=10), out_scale=0.4 * _rand(C, seed=11))
    return d


def token_reference(d, dtype=torch.float64):
    """(out, dz + add) of a case through tests/mixer_reference.token_mix and autograd, in `dtype`."""
    from tests import mixer_reference as mr
    c = {k: (None if v is None else v.to(dtype)) for k, v in d.items()}
    z = c["z"].clone().requires_grad_(True)
    out = mr.token_mix(z, c["residual"], c["w1"], c["b1"], c["w2"], c["b2"], c["in_scale"], c["in_shift"], c["out_scale"])
    dz = torch.autograd.grad(out, z, c["g"])[0] + c["add"]
    return out.detach(), dz


def case_key(S, Sh, C, F):
    return f"{S}x{Sh}x{C}x{F}"


def fp32_errors():
    from i2v_amd import graphs, weights
    from tests import mixer_reference as mr
    out = {"tokens": {}}
    for S, Sh, C in HIDDEN_CASES + [(S, 0, C) for S, C in LINEAR_CASES]:
        for F in (1, 3):
            d = token_case(S, Sh, C, F)
            o64, g64 = token_reference(d)
            o32, g32 = token_reference(d, torch.float32)
            out["tokens"][case_key(S, Sh, C, F)] = {"fwd": _rel(o32, o64), "bwd": _rel(g32, g64)}
    cases = [("mixer_test", graphs.build_tiny("mixer_b16_224", (64, 64)), _rand(3, 3, 64, 64, seed=21), [1, 3, 5, 7]),
             ("mixer_test_patch32", graphs.build_tiny("mixer_b32_224", (64, 64)), _rand(3, 3, 64, 64, seed=21), [1, 3, 5, 7]),
             ("resmlp_test", graphs.build_tiny("resmlp_12_224", (64, 64)), _rand(3, 3, 64, 64, seed=21), [1, 3, 5, 7])]
    cases += [(n, graphs.build(n), _rand(2, 3, 224, 224, seed=22), hooks) for n, hooks in FULL.items()]
    for label, spec, x, hooks in cases:
        sd = weights.synthetic_state_dict(spec, 0)
        r64, r32 = mr.MixerReference(spec, sd, hooks), mr.MixerReference(spec, sd, hooks, dtype=torch.float32)
        f64, f32 = r64.forward(x), r32.forward(x)
        hg = [_rand(*f.shape, seed=30 + i) for i, f in enumerate(f64)]
        out[label] = {"hooks": [_rel(a, b) for a, b in zip(f32, f64)], "grad": _rel(r32.backward(hg), r64.backward(hg)),
                      "hook_std": [float(f.std()) for f in f64]}
    return out


def main():
    with open(os.path.join(GOLDEN, "timm_mixer_keys.json"), "w") as f:
        f.write(compact(keys_fixture()))
    errs = fp32_errors()
    with open(os.path.join(GOLDEN, "mixer_fp32_cpu_errors.json"), "w") as f:
        json.dump(errs, f, indent=1)
    print(json.dumps({k: v for k, v in errs.items() if k != "tokens"}, indent=1))
    print("tokens: max fwd", max(v["fwd"] for v in errs["tokens"].values()), "max bwd", max(v["bwd"] for v in errs["tokens"].values()))


if __name__ == "__main__":
    main()
