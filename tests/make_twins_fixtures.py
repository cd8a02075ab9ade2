"""Writes the two Twins fixtures under tests/golden/ (run on the CPU: `python -m tests.make_twins_fixtures`):

  timm_twins_keys.json        name -> {state_dict key: shape} of timm's `Twins` for the six served architectures, up to the last block, in
      timm's order.  Generated from the rule restated below -- on its own, not from i2v_amd.graphs -- and checked against timm wherever
      `import timm` works.  Where it does not, the contract is UNCHECKED against timm and the file says so ("checked_against").
  twins_fp32_cpu_errors.json  relative L2 error of the float32 CPU run of the references (tests/twins_reference.py and the entry
      definitions below) against their float64 run on the inputs of tests/test_twins_cpu.py and tests/test_gpu_twins.py: what two
      correct float32 implementations may differ by.  Never taken from the code under test.  "trajectory" records the float32
      reference's own relative cost error after the 10-step I2V attack of the GPU test, per depth.
"""
import json
import os

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")

#: name -> (dims, heads, MLP ratios, depths, window); patch sizes (4, 2, 2, 2) and sr_ratios (8, 4, 2, 1) for all
TABLE = {"twins_pcpvt_small": ((64, 128, 320, 512), (1, 2, 5, 8), (8, 8, 4, 4), (3, 4, 6, 3), 0),
         "twins_pcpvt_base": ((64, 128, 320, 512), (1, 2, 5, 8), (8, 8, 4, 4), (3, 4, 18, 3), 0),
         "twins_pcpvt_large": ((64, 128, 320, 512), (1, 2, 5, 8), (8, 8, 4, 4), (3, 8, 27, 3), 0),
         "twins_svt_small": ((64, 128, 256, 512), (2, 4, 8, 16), (4, 4, 4, 4), (2, 2, 10, 4), 7),
         "twins_svt_base": ((96, 192, 384, 768), (3, 6, 12, 24), (4, 4, 4, 4), (2, 2, 18, 2), 7),
         "twins_svt_large": ((128, 256, 512, 1024), (4, 8, 16, 32), (4, 4, 4, 4), (2, 2, 18, 2), 7)}
SR = (8, 4, 2, 1)
#: sub-sampled attention cases (frames, Tq, Tk, heads, dh, kind): the smallest twin's shape; odd keys with a query count that is no
#: multiple of the 64-row step; the full-size stage 2 and stage 3 shapes of PCPVT; one frame of the real stage-0 shape (13 query tiles);
#: SVT-small's stage 1; Tk at the limit with dh no multiple of 16; a single key (P = 1, dq = 0); kind "hot": q times 30, scores of
#: magnitude ~30, so the softmax needs its row maximum
ATTN_CASES = [(1, 16, 4, 1, 16, ""), (3, 100, 9, 2, 32, ""), (2, 196, 49, 5, 64, ""), (2, 49, 49, 8, 64, ""), (1, 3136, 49, 1, 64, ""),
              (2, 784, 49, 4, 32, ""), (1, 70, 64, 1, 12, ""), (2, 33, 1, 2, 8, ""), (3, 100, 9, 2, 32, "hot")]
#: the window attention case (frames, grid, window, heads, dh)
WINDOW_CASE = (2, 8, 4, 2, 16)
#: block gather / scatter cases (s, H, W): a plane of one block, and one of 3 x 2 blocks; 8 channels
BLOCK_CASES = [(s, h * s, w * s) for s in (2, 4, 8) for h, w in ((1, 1), (3, 2))]
#: the test-size twins: label -> (a served name that maps to it, frame side, frames)
TWINS = {"twins_pcpvt_test": ("twins_pcpvt_small", 64, 3), "twins_pcpvt_test_96": ("twins_pcpvt_base", 96, 3),
         "twins_svt_test": ("twins_svt_small", 128, 3)}
HOOKS = [0, 1, 2, 3]
#: the window-7 twin that SVT names map to at 224 x 224 (the size the attack classes probe a builder with): label -> (name, side, frames)
PROBE = {"twins_svt_test_224": ("twins_svt_small", 224, 1)}
#: the full-size models of the GPU test, 2 frames
FULL = ("twins_pcpvt_small", "twins_svt_small")
#: the 10-step I2V trajectory of the GPU test: the twin (the SVT one: on the two PCPVT twins the float32 reference itself misses the 2e-4
#: bound at depth 3 -- 1.1e-3 at 64 x 64 and 2.2e-3 at 96 x 96 on this clip's seed --, on the SVT twin it is within 1.2e-5), the clip
#: (batch, frames, side, seed)
TRAJECTORY = ("twins_svt_small", (2, 4, 128, 23))


def rule(dims, heads, ratios, depths, window):
    """timm/models/twins.py (0.5.0), restated, without `norm.*` and `head.*`: the module lists in the constructor's order -- `patch_embeds`
    (`proj` a Conv2d with kernel = stride = 4, 2, 2, 2 and bias, `norm` a LayerNorm), `blocks.{k}.{j}` (`Block`: norm1, attn, norm2, mlp;
    `GlobalSubSampleAttn`: q, kv, proj, then sr (Conv2d, kernel = stride = sr) and norm where sr > 1; `LocallyGroupedAttn`: qkv, proj; a
    block is LSA where the model has a window and j is even), `pos_block.{k}.proj.0` (a depthwise 3 x 3 Conv2d with bias)."""
    out = {}
    for k in range(4):
        p, cin, ps = f"patch_embeds.{k}.", dims[k - 1] if k else 3, 2 if k else 4
        out.update({p + "proj.weight": [dims[k], cin, ps, ps], p + "proj.bias": [dims[k]], p + "norm.weight": [dims[k]], p + "norm.bias": [dims[k]]})
    for k in range(4):
        D, M = dims[k], ratios[k] * dims[k]
        for j in range(depths[k]):
            p = f"blocks.{k}.{j}."
            out.update({p + "norm1.weight": [D], p + "norm1.bias": [D]})
            if window and j % 2 == 0:
                out.update({p + "attn.qkv.weight": [3 * D, D], p + "attn.qkv.bias": [3 * D]})
            else:
                out.update({p + "attn.q.weight": [D, D], p + "attn.q.bias": [D], p + "attn.kv.weight": [2 * D, D], p + "attn.kv.bias": [2 * D]})
            out.update({p + "attn.proj.weight": [D, D], p + "attn.proj.bias": [D]})
            if not (window and j % 2 == 0) and SR[k] > 1:
                out.update({p + "attn.sr.weight": [D, D, SR[k], SR[k]], p + "attn.sr.bias": [D], p + "attn.norm.weight": [D], p + "attn.norm.bias": [D]})
            out.update({p + "norm2.weight": [D], p + "norm2.bias": [D], p + "mlp.fc1.weight": [M, D], p + "mlp.fc1.bias": [M],
                        p + "mlp.fc2.weight": [D, M], p + "mlp.fc2.bias": [D]})
    for k in range(4):
        out.update({f"pos_block.{k}.proj.0.weight": [dims[k], 1, 3, 3], f"pos_block.{k}.proj.0.bias": [dims[k]]})
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
            got = {k: list(v.shape) for k, v in sd.items() if not k.startswith(("head.", "norm."))}
            assert got == want and list(got) == list(want), (n, sorted(set(got) ^ set(want))[:8])
        checked = f"timm {timm.__version__}"
    return {"checked_against": checked, "follows": "timm 0.5.0 twins.py key layout (restated)", "names": names}


def compact(fx):
    """One module per line: the file is the contract, read by eye, and stays under the size limit."""
    head = {k: v for k, v in fx.items() if k != "names"}
    out = ["{"] + [f" {json.dumps(k)}: {json.dumps(v)}," for k, v in head.items()] + [' "names": {']
    for i, (n, keys) in enumerate(fx["names"].items()):
        out.append(f"  {json.dumps(n)}: {{")
        lines, cur, tag = [], [], None
        for k, v in keys.items():
            t = ".".join(k.split(".")[:3 if k.startswith("blocks") else 2])
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


# ---- sub-sampled attention ---------------------------------------------------------------------------------------------------------
def attn_case(F_, Tq, Tk, H, dh, kind=""):
    """The float64 inputs of one case: q, kv ~ N(0, 1) (q times 30 for "hot"), dout the output's gradient."""
    d = {"q": _rand(F_, Tq, H * dh, seed=1), "kv": _rand(F_, Tk, 2 * H * dh, seed=2), "dout": _rand(F_, Tq, H * dh, seed=3), "heads": H}
    if kind == "hot":
        d["q"] = d["q"] * 30.0
    return d


def attn_reference(d, dtype=torch.float64):
    """(out, dq, dkv) of a case through tests/twins_reference.gsa_core (timm's literal arithmetic) and autograd, in `dtype`."""
    from tests import twins_reference as tr
    c = _cast(d, dtype)
    q, kv = c["q"].clone().requires_grad_(True), c["kv"].clone().requires_grad_(True)
    out = tr.gsa_core(q, kv, c["heads"])
    dq, dkv = torch.autograd.grad(out, (q, kv), c["dout"])
    return out.detach(), dq, dkv


def case_key(F_, Tq, Tk, H, dh, kind=""):
    return f"{F_}x{Tq}x{Tk}x{H}x{dh}" + (f"-{kind}" if kind else "")


def window_case():
    F_, g, ws, H, dh = WINDOW_CASE
    return {"qkv": _rand(F_, g * g, 3 * H * dh, seed=4), "dout": _rand(F_, g * g, H * dh, seed=5), "heads": H, "grid": g, "window": ws}


def window_reference(d, dtype=torch.float64):
    from tests import twins_reference as tr
    c = _cast(d, dtype)
    qkv = c["qkv"].clone().requires_grad_(True)
    out = tr.lsa_core(qkv, c["heads"], c["grid"], c["window"])
    return out.detach(), torch.autograd.grad(out, qkv, c["dout"])[0]


# ---- the block gather --------------------------------------------------------------------------------------------------------------
def block_case(s, H, W, C=8):
    return {"x": _rand(2, H, W, C, seed=6).float(), "drows": _rand(2 * (H // s) * (W // s), s * s * C, seed=7).float(),
            "base": _rand(2, H, W, C, seed=8).float()}


def gather_reference(x, s):
    """rows (n H/s W/s, s s C) with column (dy s + dx) C + c, by reshape."""
    n, H, W, C = x.shape
    return x.reshape(n, H // s, s, W // s, s, C).permute(0, 1, 3, 2, 4, 5).reshape(n * (H // s) * (W // s), s * s * C).contiguous()


def scatter_reference(drows, shape, s):
    n, H, W, C = shape
    return drows.reshape(n, H // s, W // s, s, s, C).permute(0, 1, 3, 2, 4, 5).reshape(n, H, W, C).contiguous()


def twin_input(label):
    _, side, frames = {**TWINS, **PROBE}[label]
    return _rand(frames, 3, side, side, seed=21)


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
    from tests import twins_reference as tr
    out = {"attention": {}}
    for case in ATTN_CASES:
        d = attn_case(*case)
        r64, r32 = attn_reference(d), attn_reference(d, torch.float32)
        out["attention"][case_key(*case)] = {"fwd": _rel(r32[0], r64[0]), "dkv": _rel(r32[2], r64[2])}
        if case[2] > 1:                                                    # (a single key: dq is identically 0, there is no relative error)
            out["attention"][case_key(*case)]["dq"] = _rel(r32[1], r64[1])
    d = window_case()
    r64, r32 = window_reference(d), window_reference(d, torch.float32)
    out["window"] = {"fwd": _rel(r32[0], r64[0]), "bwd": _rel(r32[1], r64[1])}
    cases = []
    for label, (name, side, _) in {**TWINS, **PROBE}.items():
        spec = graphs.build_tiny(name, (side, side))
        assert spec.arch == label
        cases.append((label, spec, weights.synthetic_state_dict(spec, 0), twin_input(label)))
    for n in FULL:
        spec = graphs.build(n)
        cases.append((n, spec, weights.synthetic_state_dict(spec, 0), _rand(2, 3, 224, 224, seed=22)))
    for label, spec, sd, x in cases:
        r64, r32 = tr.TwinsReference(spec, sd, HOOKS), tr.TwinsReference(spec, sd, HOOKS, dtype=torch.float32)
        f64, f32 = r64.forward(x), r32.forward(x)
        hg = [_rand(*f.shape, seed=30 + i) for i, f in enumerate(f64)]
        out[label] = {"hooks": [_rel(a, b) for a, b in zip(f32, f64)], "grad": _rel(r32.backward(hg), r64.backward(hg)),
                      "hook_std": [float(f.std()) for f in f64]}
    name, clip = TRAJECTORY
    spec = graphs.build_tiny(name, (clip[2], clip[2]))
    sd, vid = weights.synthetic_state_dict(spec, 0), video(*clip)
    out["trajectory"] = {}
    for depth in (1, 2, 3, 4):
        runs = [restate.run_attack([tr.TwinsReference(spec, sd, [spec.hook_for(depth)], dtype=dt)], vid, steps=10, step_size=0.005)
                for dt in (torch.float64, torch.float32)]
        c64, c32 = (torch.as_tensor(r["costs"], dtype=torch.float64) for r in runs)
        out["trajectory"][str(depth)] = float(((c32 - c64).abs() / c64.abs()).max())
    return out


def main():
    with open(os.path.join(GOLDEN, "timm_twins_keys.json"), "w") as f:
        f.write(compact(keys_fixture()))
    errs = fp32_errors()
    with open(os.path.join(GOLDEN, "twins_fp32_cpu_errors.json"), "w") as f:
        json.dump(errs, f, indent=1)
    print(json.dumps(errs, indent=1))


if __name__ == "__main__":
    main()
