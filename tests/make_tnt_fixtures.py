"""Writes the two TNT fixtures under tests/golden/ (run on the CPU: `python -m tests.make_tnt_fixtures`):

  timm_tnt_keys.json        name -> {state_dict key: shape} of timm's `TNT` for the two served names, up to the last block.  Generated
      from the rule restated below -- on its own, not from i2v_amd.graphs -- and checked against timm wherever `import timm` works.
      Where it does not, the contract is UNCHECKED against timm and the file says so ("checked_against").
  tnt_fp32_cpu_errors.json  relative L2 error of the float32 CPU run of the references (tests/tnt_reference.py) against their float64
      run on the inputs of tests/test_tnt_cpu.py and tests/test_gpu_tnt.py: what two correct float32 implementations may differ by.
      Never taken from the code under test.  "trajectory" records the float32 reference's own relative cost error after the 10-step I2V
      attack of the tests, per depth.
"""
import json
import os

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")

#: name -> (dim, in_dim, blocks, heads, in_heads), all at 224 x 224 with patch 16 and MLP ratio 4 on both levels
TABLE = {"tnt_s_patch16_224": (384, 24, 12, 6, 4), "tnt_b_patch16_224": (640, 40, 12, 10, 4)}
#: sequences a workgroup of the attention launches owns at (T 16, 4 heads, dh 6): the tests assert that the library says the same
#: (`i2v_tnt_attention_group`), so the two cases around it below do bracket a workgroup's worth
GROUP = 4
#: attention cases (sequences, T, heads, dh, kind): one sequence; one fewer and one more than a workgroup's worth; 197 sequences at
#: tnt_b's width; a single token; T 9 under 2 heads; the narrowest and the widest head; the most heads at an odd width; one head; one
#: full frame of tnt_s; two cases that stress the softmax
ATTN_CASES = [(1, 16, 4, 6, ""), (GROUP - 1, 16, 4, 6, ""), (GROUP + 1, 16, 4, 6, ""), (197, 16, 4, 10, ""), (5, 1, 4, 6, ""), (7, 9, 2, 6, ""),
              (3, 16, 4, 1, ""), (3, 16, 4, 16, ""), (3, 16, 8, 3, ""), (3, 16, 1, 4, ""), (196, 16, 4, 6, ""), (6, 16, 4, 6, "wide"),
              (6, 16, 4, 6, "onehot")]
ATTN_PARTS = ("out", "dq", "dk", "dv")
#: the one-hot case: row ONEHOT_ROW of every sequence and head attends to key ONEHOT_KEY alone
ONEHOT_ROW, ONEHOT_KEY = 5, 3
#: pixel cases (frames, channels, side): one 16 x 16 frame (one patch, every window over the border) with one channel (3 padding
#: columns); 48 x 48 with 3 channels (an odd patch grid, 1 padding column); 3 frames of 32 x 32 with 2 channels
PIXEL_CASES = [(1, 1, 16), (1, 3, 48), (3, 2, 32)]
#: the test-size twins: label -> (a served name that maps to it, frame side, frames)
TWINS = {"tnt_test": ("tnt_s_patch16_224", 64, 3), "tnt_test_48": ("tnt_b_patch16_224", 48, 2)}
#: the full-size model of the GPU test, two frames
FULL = ("tnt_s_patch16_224",)
#: the clip of the 10-step I2V trajectory on tnt_test whose float32 error is recorded: (batch, frames, side, seed); the tests' depth
TRAJECTORY_CLIP, TRAJECTORY_DEPTH = (2, 4, 64, 23), 3


def rule(dim, in_dim, blocks, heads, in_heads):
    """timm/models/tnt.py (0.5.0), restated from memory, without `norm.*` and `head.*`: `cls_token`, `patch_pos`, `pixel_pos`,
    `pixel_embed.proj` (Conv2d(3, in_dim, 7, stride 4, padding 3)), `norm1_proj` over 16 in_dim, `proj`, `norm2_proj`; per block
    `norm_in`, `attn_in` (qk and v without bias, proj with), `norm_mlp_in`, `mlp_in`, `norm1_proj` over in_dim, `proj`, `norm_out`,
    `attn_out`, `norm_mlp`, `mlp`."""
    D, d = dim, in_dim
    out = {"cls_token": [1, 1, D], "patch_pos": [1, 197, D], "pixel_pos": [1, d, 4, 4], "pixel_embed.proj.weight": [d, 3, 7, 7],
           "pixel_embed.proj.bias": [d], "norm1_proj.weight": [16 * d], "norm1_proj.bias": [16 * d], "proj.weight": [D, 16 * d], "proj.bias": [D],
           "norm2_proj.weight": [D], "norm2_proj.bias": [D]}

    def level(p, w, norm, attn, norm_mlp, mlp):
        return {p + norm + ".weight": [w], p + norm + ".bias": [w], p + attn + ".qk.weight": [2 * w, w], p + attn + ".v.weight": [w, w],
                p + attn + ".proj.weight": [w, w], p + attn + ".proj.bias": [w], p + norm_mlp + ".weight": [w], p + norm_mlp + ".bias": [w],
                p + mlp + ".fc1.weight": [4 * w, w], p + mlp + ".fc1.bias": [4 * w], p + mlp + ".fc2.weight": [w, 4 * w], p + mlp + ".fc2.bias": [w]}
    for i in range(blocks):
        p = f"blocks.{i}."
        out.update(level(p, d, "norm_in", "attn_in", "norm_mlp_in", "mlp_in"))
        out.update({p + "norm1_proj.weight": [d], p + "norm1_proj.bias": [d], p + "proj.weight": [D, 16 * d], p + "proj.bias": [D]})
        out.update(level(p, D, "norm_out", "attn_out", "norm_mlp", "mlp"))
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
            got = {k: list(v.shape) for k, v in sd.items() if not k.startswith(("head.", "norm."))}
            assert got == want, (n, sorted(set(got) ^ set(want))[:8])
        checked = f"timm {timm.__version__}"
    return {"checked_against": checked, "follows": "timm 0.5.0 tnt.py key layout (restated from memory)", "names": names}


def compact(fx):
    """One level of a block per line: the file is the contract, read by eye, and stays under the size limit."""
    head = {k: v for k, v in fx.items() if k != "names"}
    out = ["{"] + [f" {json.dumps(k)}: {json.dumps(v)}," for k, v in head.items()] + [' "names": {']
    for i, (n, keys) in enumerate(fx["names"].items()):
        out.append(f"  {json.dumps(n)}: {{")
        lines, cur, tag = [], [], None
        for k, v in keys.items():
            parts = k.split(".")
            t = ".".join(parts[:2]) + ("in" if parts[0] == "blocks" and parts[2].endswith("_in") else "") if parts[0] == "blocks" else "top"
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


# ---- attention ---------------------------------------------------------------------------------------------------------------------
def attn_case(S, T, H, dh, kind=""):
    """The float64 inputs of one case: qkv ~ N(0, 1), dout the output's gradient.  The softmax cases: "wide": q is 30 x larger, so the
    scaled scores have a standard deviation of about 30 and span about +-80 -- without the row maximum subtracted exp overflows;
    "onehot": every key ONEHOT_KEY is 3 in every column and q of row ONEHOT_ROW is 60 x that key, so that row's score for that key
    lies hundreds above the others, its probabilities are one-hot in float32 and in float64, and its dS and dq are 0."""
    C = H * dh
    d = {"qkv": _rand(S, T, 3 * C, seed=1), "dout": _rand(S, T, C, seed=3), "heads": H}
    if kind == "wide":
        d["qkv"][:, :, :C] *= 30.0
    if kind == "onehot":
        d["qkv"][:, ONEHOT_KEY, C:2 * C] = 3.0
        d["qkv"][:, ONEHOT_ROW, :C] = 180.0
    return d


def attn_reference(d, dtype=torch.float64):
    """(out, dq, dk, dv) of a case through tests/tnt_reference.attention_core and autograd, in `dtype`."""
    from tests import tnt_reference as tr
    c = _cast(d, dtype)
    qkv = c["qkv"].clone().requires_grad_(True)
    out = tr.attention_core(qkv, c["heads"])
    dqkv, = torch.autograd.grad(out, qkv, c["dout"])
    C = qkv.shape[2] // 3
    return out.detach(), dqkv[:, :, :C], dqkv[:, :, C:2 * C], dqkv[:, :, 2 * C:]


def case_key(*case):
    return "x".join(str(v) for v in case if v != "")


# ---- the pixel pair ----------------------------------------------------------------------------------------------------------------
def pixel_case(F_, Cin, side):
    rows = F_ * (side // 4) ** 2
    return {"x": _rand(F_, Cin, side, side, seed=5), "drows": _rand(rows, Cin * 49, seed=6)}


def pixel_reference(d, dtype=torch.float64):
    """(rows, dx): the convolution's rows without the padding columns, and their adjoint by autograd."""
    from tests import tnt_reference as tr
    c = _cast(d, dtype)
    x = c["x"].clone().requires_grad_(True)
    rows = tr.pixel_rows(x)
    dx, = torch.autograd.grad(rows, x, c["drows"])
    return rows.detach(), dx


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
    from tests import tnt_reference as tr
    out = {"attention": {}, "pixels": {}}
    for case in ATTN_CASES:
        d = attn_case(*case)
        r64, r32 = attn_reference(d), attn_reference(d, torch.float32)
        # (a single token: P = 1, so dq and dk are identically 0 and have no relative error: the tests hold them absolutely)
        out["attention"][case_key(*case)] = {k: _rel(a, b) for k, a, b in zip(ATTN_PARTS, r32, r64) if not (case[1] == 1 and k in ("dq", "dk"))}
    for case in PIXEL_CASES:
        d = pixel_case(*case)
        r64, r32 = pixel_reference(d), pixel_reference(d, torch.float32)
        out["pixels"][case_key(*case)] = {"gather": _rel(r32[0], r64[0]), "scatter": _rel(r32[1], r64[1])}
    for label, spec, x in net_cases():
        sd = weights.synthetic_state_dict(spec, 0)
        hooks = [spec.hook_for(d) for d in (1, 2, 3, 4)]
        r64, r32 = tr.TntReference(spec, sd, hooks), tr.TntReference(spec, sd, hooks, dtype=torch.float32)
        f64, f32 = r64.forward(x), r32.forward(x)
        hg = [_rand(*f.shape, seed=30 + i) for i, f in enumerate(f64)]
        out[label] = {"hooks": [_rel(a, b) for a, b in zip(f32, f64)], "grad": _rel(r32.backward(hg), r64.backward(hg)),
                      "hook_std": [float(f.std()) for f in f64]}
    label = "tnt_test"
    name, side, _ = TWINS[label]
    spec = graphs.build_tiny(name, (side, side))
    sd, vid = weights.synthetic_state_dict(spec, 0), video(*TRAJECTORY_CLIP)
    out["trajectory"] = {label: {}}
    for depth in (1, 2, 3, 4):
        runs = [restate.run_attack([tr.TntReference(spec, sd, [spec.hook_for(depth)], dtype=dt)], vid, steps=10, step_size=0.005)
                for dt in (torch.float64, torch.float32)]
        c64, c32 = (torch.as_tensor(r["costs"], dtype=torch.float64) for r in runs)
        out["trajectory"][label][str(depth)] = float(((c32 - c64).abs() / c64.abs()).max())
    return out


def main():
    with open(os.path.join(GOLDEN, "timm_tnt_keys.json"), "w") as f:
        f.write(compact(keys_fixture()))
    errs = fp32_errors()
    with open(os.path.join(GOLDEN, "tnt_fp32_cpu_errors.json"), "w") as f:
        json.dump(errs, f, indent=1)
    print(json.dumps(errs, indent=1))


if __name__ == "__main__":
    main()
