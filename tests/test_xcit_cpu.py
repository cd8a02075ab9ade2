"""CPU: timm's XCiT family as image surrogates on the transformer stack -- for every served name the spec and the key /
shape contract against tests/golden/timm_xcit_keys.json; the refusals; checkpoint loading with both spellings of the position keys; every
fold of the native packing (the stem BatchNorms, the position table, the three LayerScales, the LPI BatchNorm pair, the temperature)
against timm's literal arithmetic, and that leaving a fold out is seen; the three kernel entries (cross-covariance attention, the depthwise
3 x 3, the stem gather / scatter) on the host simulation, which runs them as scalar code (csrc/i2v_xcit_host.h); and the planner itself
(csrc/i2v_xcit.cpp) on the host simulation: both twins against float64, a 4-step I2V attack and an AENS ensemble against the oracle.

The bound is relative L2 against float64: the larger of the floor for that kind of case (entries 1e-6 forward and on probs, 1e-5 backward;
nets 1e-5) and 4 x the error of the float32 CPU run of the same reference on the same inputs, read from
tests/golden/xcit_fp32_cpu_errors.json (tests/make_xcit_fixtures.py).  A case without a recorded error fails (KeyError)."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from i2v_amd import attacks, graphs, weights
from i2v_amd import lib as _lib
from oracle import restate
from tests import make_xcit_fixtures as mk
from tests import xcit_reference as xr
from tests.family_harness import bound, check_trajectory, rand as _rand, rel as _rel, run_twin as _run_twin
from tests.hostsim_util import hostsim_engine
from tests.xcit_reference import XcitReference

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = json.load(open(os.path.join(ROOT, "tests", "golden", "timm_xcit_keys.json")))
FP32 = json.load(open(os.path.join(ROOT, "tests", "golden", "xcit_fp32_cpu_errors.json")))
BASE = {"xcit_nano_12_p16_224": (128, 12, 4), "xcit_tiny_12_p16_224": (192, 12, 4), "xcit_tiny_24_p16_224": (192, 24, 4),
        "xcit_small_12_p16_224": (384, 12, 8), "xcit_small_24_p16_224": (384, 24, 8), "xcit_medium_24_p16_224": (512, 24, 8),
        "xcit_large_24_p16_224": (768, 24, 16)}
TABLE = {**BASE, **{k + "_dist": v for k, v in BASE.items()}}
NAMES = sorted(TABLE)
NANO, TINY, SMALL = "xcit_nano_12_p16_224", "xcit_tiny_12_p16_224", "xcit_small_12_p16_224"
NET_FLOOR, FWD_FLOOR, BWD_FLOOR = 1e-5, 1e-6, 1e-5


# ---- the specs ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_param_shapes_equal_the_key_fixture(name):
    base = name[:-5] if name.endswith("_dist") else name
    want = {k: tuple(v) for k, v in KEYS["names"][base].items()}
    shapes = graphs.build(name).param_shapes()
    assert shapes == want and list(shapes) == list(want)
    assert KEYS["checked_against"].startswith(("timm ", "unchecked"))
    if name != base:                                                      # the _dist twin builds to the same shapes, under its own name
        assert shapes == graphs.build(base).param_shapes() and graphs.build(name).arch == name != graphs.build(base).arch


@pytest.mark.parametrize("name", NAMES)
def test_spec_tokens_widths_and_hooks_of_every_name(name):
    dim, blocks, heads = TABLE[name]
    spec = graphs.build(name)
    assert isinstance(spec, graphs.XcitSpec) and spec.arch == name and spec.video is False and spec.in_hw == (224, 224)
    assert (spec.img, spec.patch, spec.in_chans, spec.dim, spec.heads, spec.blocks, spec.ln_eps) == (224, 16, 3, dim, heads, blocks, 1e-6)
    assert spec.tokens == 196 and spec.grid == 14 and spec.mlp == 4 * dim and dim // heads in (32, 48, 64)
    assert spec.stem_widths == [3, dim // 8, dim // 4, dim // 2, dim]
    hooks = [spec.hook_for(d) for d in (1, 2, 3, 4)]
    assert hooks == ([2, 5, 8, 11] if blocks == 12 else [5, 11, 17, 23])
    assert all(spec.hook_dim(b) == 196 * dim for b in hooks)
    with pytest.raises(KeyError):
        spec.hook_for(5)
    assert graphs.xcit_named(name) == spec and graphs.is_xcit_name(name)
    assert not any(f(name) for f in (graphs.is_swin_name, graphs.is_vit_name, graphs.is_convnext_name, graphs.is_mixer_name, graphs.is_cait_name,
                                     graphs.is_convit_name))
    shapes = spec.param_shapes()
    assert shapes["patch_embed.proj.0.0.weight"] == (dim // 8, 3, 3, 3) and shapes["patch_embed.proj.6.1.running_var"] == (dim,)
    assert shapes["pos_embeder.token_projection.weight"] == (dim, 64, 1, 1) and shapes["blocks.0.attn.temperature"] == (heads, 1, 1)
    assert shapes[f"blocks.{blocks - 1}.local_mp.conv2.weight"] == (dim, 1, 3, 3) and f"blocks.{blocks}.gamma1" not in shapes
    assert not any(k.startswith(("head.", "norm.", "cls_token", "cls_attn_blocks.")) or k.endswith("num_batches_tracked") for k in shapes)
    for hw in ((384, 384), (112, 112), (224, 192)):
        with pytest.raises(ValueError, match="224 x 224") as ei:
            graphs.build(name, hw)
        assert all(n in str(ei.value) for n in TABLE)


def test_refusals_name_the_reason_and_list_the_served_names():
    for name, why in (("xcit", "not a model"), ("xcit_huge_24_p16_224", "not a model"), ("xcit_small_12_p8_224", "three-convolution stem"),
                      ("xcit_tiny_24_p8_224_dist", "784 tokens"), ("xcit_small_12_p16_384_dist", "384 x 384"),
                      ("xcit_large_24_p8_384_dist", "three-convolution stem")):
        assert graphs.is_xcit_name(name)
        with pytest.raises(ValueError, match=why) as ei:
            graphs.build(name)
        assert all(n in str(ei.value) for n in TABLE) and "not a model of this table" in str(ei.value)
        with pytest.raises(ValueError, match="not a model of this table"):
            graphs.build_tiny(name)


def test_existing_names_behave_as_before():
    with pytest.raises(UnboundLocalError):
        graphs.build("transformer")
    with pytest.raises(UnboundLocalError):
        graphs.build("pit_s_224")
    with pytest.raises(ValueError, match="not served"):
        graphs.build("mobilenet_v2")
    assert not any(graphs.is_xcit_name(n) for n in ("convnext_tiny", "vit_base_patch16_224", "cait_s24_224", "convit_tiny", "resnet", "conv"))
    assert isinstance(graphs.build("convit_tiny"), graphs.ConvitSpec) and isinstance(graphs.build("cait_s24_224"), graphs.CaitSpec)
    assert isinstance(graphs.build("vit_base_patch16_224"), graphs.VitSpec) and graphs.build("resnet").arch == "resnet101"
    others = (set(graphs.SWIN_MODELS) | set(graphs.VIT_MODELS) | set(graphs.CONVNEXT_MODELS) | set(graphs.MIXER_MODELS) | set(graphs.CAIT_MODELS)
              | set(graphs.CONVIT_MODELS))
    assert not set(graphs.XCIT_MODELS) & others and graphs.XCIT_MODELS == TABLE


# ---- checkpoints -------------------------------------------------------------------------------------------------------------------
def _checkpoint(spec):
    """A timm-shaped checkpoint with the keys behind every hook as well."""
    D = spec.dim
    sd = {k: torch.zeros(1).expand(shp) for k, shp in spec.param_shapes().items()}
    sd.update({"cls_token": torch.zeros(1, 1, D), "norm.weight": torch.ones(D), "norm.bias": torch.zeros(D), "head.weight": torch.zeros(1).expand(1000, D),
               "head.bias": torch.zeros(1000), "cls_attn_blocks.0.gamma1": torch.ones(D), "blocks.0.local_mp.bn.num_batches_tracked": torch.tensor(0)})
    return sd


@pytest.mark.parametrize("name", [NANO, SMALL + "_dist"])
def test_checkpoint_loads_from_its_own_file_with_either_spelling_of_the_position_keys(name, tmp_path, monkeypatch):
    spec = graphs.build(name)
    monkeypatch.delenv("I2V_SYNTHETIC_WEIGHTS", raising=False)
    monkeypatch.setenv("I2V_WEIGHTS_DIR", str(tmp_path))
    with pytest.raises(weights.MissingWeights, match=name):
        weights.load_state_dict(spec)
    sd = _checkpoint(spec)
    sd["pos_embeder.token_projection.bias"] = torch.full((spec.dim,), 0.25)
    for later in (False, True):
        ck = {k.replace("pos_embeder.", "pos_embed.") if later else k: v for k, v in sd.items()}
        assert ("pos_embed.token_projection.bias" in ck) == later
        torch.save(ck, tmp_path / f"{name}.pth")
        got = weights.load_state_dict(spec)
        assert list(got) == list(spec.param_shapes())
        assert all(tuple(got[k].shape) == shp and got[k].is_contiguous() for k, shp in spec.param_shapes().items())
        assert float(got["pos_embeder.token_projection.bias"].mean()) == 0.25
    if name.endswith("_dist"):                                            # the twin reads its own file, not the base name's
        with pytest.raises(weights.MissingWeights):
            weights.load_state_dict(graphs.build(name[:-5]))


def test_misshaped_and_missing_keys_are_refused_by_key(tmp_path, monkeypatch):
    monkeypatch.setenv("I2V_WEIGHTS_DIR", str(tmp_path))
    for name, bad, shape, gone in ((NANO, "blocks.3.attn.temperature", (4,), "blocks.9.gamma3"),
                                   (TINY, "patch_embed.proj.2.0.weight", (48, 24, 1, 1), "pos_embeder.token_projection.weight")):
        spec = graphs.build(name)
        sd = _checkpoint(spec)
        path = tmp_path / f"{name}.pth"
        torch.save(dict(sd, **{bad: torch.zeros(*shape)}), path)
        with pytest.raises(ValueError, match=bad.replace(".", r"\.")):
            weights.load_state_dict(spec)
        short = dict(sd)
        del short[gone]
        torch.save(short, path)
        with pytest.raises(KeyError, match=gone.replace(".", r"\.")):
            weights.load_state_dict(spec)


def test_synthetic_weights_let_the_new_arithmetic_show():
    spec = graphs.build(NANO)
    sd = weights.load_state_dict(spec, seed=3)
    assert {k: tuple(v.shape) for k, v in sd.items()} == spec.param_shapes()
    for i in (0, 11):
        g = [sd[f"blocks.{i}.gamma{j}"] for j in (1, 2, 3)]
        assert all(0.5 <= float(v.min()) and float(v.max()) <= 1.5 and float(v.std()) > 0.2 for v in g)
        assert not torch.equal(g[0], g[1]) and not torch.equal(g[1], g[2])
        t = sd[f"blocks.{i}.attn.temperature"]
        assert 0.5 <= float(t.min()) and float(t.max()) <= 4.0 and float(t.max() - t.min()) > 0.2
        assert float(sd[f"blocks.{i}.local_mp.bn.running_var"].min()) >= 0.5 and float(sd[f"blocks.{i}.local_mp.conv2.bias"].abs().mean()) > 0.03
    assert float(sd["patch_embed.proj.0.1.running_var"].min()) >= 0.5 and float(sd["patch_embed.proj.4.1.running_mean"].abs().mean()) > 0.02


def test_test_size_twins():
    t = graphs.build_tiny(SMALL, (64, 64))
    assert t == graphs.build_tiny(NANO, (64, 64)) == graphs.build_tiny(TINY + "_dist", (64, 64)) == graphs.xcit_tiny_twin()
    assert t.arch == "xcit_test" and t.arch not in graphs.XCIT_MODELS
    assert (t.dim, t.heads, t.blocks, t.tokens, t.grid, t.mlp) == (32, 4, 8, 16, 4, 128) and t.hooks == {1: 1, 2: 3, 3: 5, 4: 7}
    t80 = graphs.build_tiny(SMALL, (80, 80))
    assert t80.arch == "xcit_test_80" and (t80.dim, t80.heads, t80.blocks, t80.tokens, t80.grid) == (48, 4, 8, 25, 5)
    assert [9 * c for c in t80.stem_widths[:4]] == [27, 54, 108, 216]
    with pytest.raises(ValueError):
        graphs.build_tiny(SMALL, (72, 72))
    ref = XcitReference(t, weights.synthetic_state_dict(t, 0), [1, 7])
    f = ref.forward(torch.randn(2, 3, 64, 64))
    assert [tuple(a.shape) for a in f] == [(2, 16 * 32)] * 2
    assert ref.backward([torch.ones_like(a) for a in f]).shape == (2, 3, 64, 64)


# ---- the packer against timm's literal arithmetic ----------------------------------------------------------------------------------
def test_position_table_against_the_literal_fourier_code():
    for side in (64, 80, 224):
        spec = graphs.xcit_named(NANO) if side == 224 else graphs.xcit_tiny_twin((side, side))
        lit = xr.fourier(spec.grid).flatten(2).transpose(1, 2)[0]          # (tokens, 64)
        assert tuple(lit.shape) == (spec.tokens, 64) and float((spec.fourier_features() - lit).abs().max()) < 1e-14
        sd = weights.synthetic_state_dict(spec, 0)
        pos = F.conv2d(xr.fourier(spec.grid), sd["pos_embeder.token_projection.weight"].double(), sd["pos_embeder.token_projection.bias"].double())
        table = spec.native_arrays(sd, 1)[8]
        assert tuple(table.shape) == (spec.tokens, spec.dim) and _rel(table, pos.flatten(2).transpose(1, 2)[0]) < 1e-7
    g = xr.fourier(5)[0]                                                   # y features first; sin on even and cos on odd feature indices
    y1 = 1.0 / (5 + 1e-6) * 2 * np.pi
    assert abs(float(g[0, 0, 3]) - np.sin(y1)) < 1e-12 and abs(float(g[1, 0, 3]) - np.cos(y1)) < 1e-12 and abs(float(g[32, 3, 0]) - np.sin(y1)) < 1e-12


def test_native_packing_against_the_literal_reference():
    spec = graphs.build_tiny(SMALL, (80, 80))
    sd = weights.synthetic_state_dict(spec, 0)
    sd64 = {k: v.double() for k, v in sd.items()}
    a = spec.native_arrays(sd, 8)
    D, H, T = 48, 4, 25
    assert len(a) == 9 + 21 * 8 and all(t.dtype == torch.float32 and t.is_contiguous() for t in a) and len(spec.native_arrays(sd, 3)) == 9 + 21 * 3
    assert [tuple(t.shape) for t in a[:9]] == [(6, 27), (6,), (12, 54), (12,), (24, 108), (24,), (48, 216), (48,), (T, D)]
    # the stem: gather rows (column = tap * C_in + c) times the folded weight, plus the folded bias, is conv + BatchNorm
    x = _rand(2, 3, 80, 80, seed=7)
    lit = xr._bn(F.conv2d(x, sd64["patch_embed.proj.0.0.weight"], None, stride=2, padding=1), sd64, "patch_embed.proj.0.1.")
    prod = mk.gather_reference(x, True) @ a[0].double().t()
    fold = lambda v: v.reshape(2, 40, 40, 6).permute(0, 3, 1, 2)      # noqa: E731
    assert _rel(fold(prod + a[1].double()), lit) < 1e-7
    assert _rel(fold(prod), lit) > 0.05                                   # ... and without the bias it is not
    b = 9 + 21 * 2                                                         # block 2
    blk = a[b:b + 21]
    assert [tuple(t.shape) for t in blk] == [(D,), (D,), (3 * D, D), (3 * D,), (H,), (D, D), (D,), (D,), (D,), (4 * D, D), (4 * D,), (D, 4 * D), (D,),
                                             (D,), (D,), (9, D), (D,), (D,), (D,), (9, D), (D,)]
    p = "blocks.2."
    assert torch.equal(blk[2], sd[p + "attn.qkv.weight"]) and torch.equal(blk[4], sd[p + "attn.temperature"].reshape(H))
    assert torch.equal(blk[7], sd[p + "norm2.weight"]) and torch.equal(blk[13], sd[p + "norm3.weight"])
    t = _rand(2, T, D, seed=8)
    lit = sd64[p + "gamma1"] * F.linear(t, sd64[p + "attn.proj.weight"], sd64[p + "attn.proj.bias"])
    assert _rel(F.linear(t, blk[5].double(), blk[6].double()), lit) < 1e-7
    h = _rand(2, T, 4 * D, seed=9)
    lit = sd64[p + "gamma2"] * F.linear(h, sd64[p + "mlp.fc2.weight"], sd64[p + "mlp.fc2.bias"])
    assert _rel(F.linear(h, blk[11].double(), blk[12].double()), lit) < 1e-7
    # the LPI: two launches of the depthwise definition against conv, GELU, BatchNorm, conv, LayerScale
    lit = sd64[p + "gamma3"] * xr.lpi(t, sd64, p + "local_mp.", 5)
    plane = t.reshape(2, 5, 5, D)
    u = mk.dw3_reference({"x": plane, "w": blk[15].double(), "b": blk[16].double(), "ta": None, "ts": None, "add": None, "ma": None, "mu": None})
    y = mk.dw3_reference({"x": u, "w": blk[19].double(), "b": blk[20].double(), "ta": blk[17].double(), "ts": blk[18].double(), "add": None,
                          "ma": None, "mu": None})
    assert _rel(y.reshape(2, T, D), lit) < 1e-7
    # the BatchNorm's shift folded into conv2's bias instead (s times the filter's sum) is wrong at the plane's edge: the padding is of its output
    w2 = blk[19].double()
    shifted = mk.dw3_reference({"x": u, "w": w2, "b": blk[20].double() + blk[18].double() * w2.sum(0), "ta": blk[17].double(),
                                "ts": torch.zeros(D, dtype=torch.float64), "add": None, "ma": None, "mu": None})
    assert _rel(shifted.reshape(2, T, D), lit) > 1e-3
    assert _rel(shifted[:, 1:4, 1:4], y[:, 1:4, 1:4]) < 1e-12             # (the interior agrees)


@pytest.fixture(scope="module")
def eng():
    e = hostsim_engine()
    _lib.bind(e.capi, _lib._XCIT_PROTOS)
    return e


# ---- the three entries on the host simulation --------------------------------------------------------------------------------------
def _f(v):
    return None if v is None else v.float().contiguous()


def run_attn(eng, d):
    qkv, temp = _f(d["qkv"]), _f(d["temperature"])
    out, probs, gram = eng.xcit_attention(qkv, d["heads"], temp)
    return out, probs, eng.xcit_attention_bwd(qkv, gram, probs, _f(d["dout"]), d["heads"], temp), gram


@pytest.mark.parametrize("F_,T,H,dh,kind", [c for c in mk.ATTN_CASES if c[0] * c[1] * c[2] * c[3] * c[3] < 4e6])
def test_attention_host_twin_against_float64_autograd(eng, F_, T, H, dh, kind):
    d = mk.attn_case(F_, T, H, dh, kind)
    out, probs, dqkv, gram = run_attn(eng, d)
    want, want_p, want_g = mk.attn_reference(d)
    fp = FP32["attention"][mk.case_key(F_, T, H, dh, kind)]
    e_f, e_p = _rel(out, want), _rel(probs, want_p)
    print(f"xca F {F_} T {T} H {H} dh {dh} {kind}: out {e_f:.3e} (fp32 CPU {fp['fwd']:.3e}) probs {e_p:.3e} ({fp['probs']:.3e})")
    assert e_f < bound(fp["fwd"], FWD_FLOOR) and e_p < bound(fp["probs"], FWD_FLOOR)
    q, k = d["qkv"].reshape(F_, T, 3, H, dh).permute(2, 0, 3, 1, 4)[:2]
    assert _rel(gram[:, :, dh], q.norm(dim=2).clamp_min(1e-12)) < 1e-6 and _rel(gram[:, :, dh + 1], k.norm(dim=2).clamp_min(1e-12)) < 1e-6
    if kind == "zero":
        assert float((probs[:, 0, 3] - 1.0 / dh).abs().max()) < 1e-7 and bool(torch.isfinite(dqkv).all())
        assert float(gram[0, 0, dh, 3]) == float(gram[0, 0, dh + 1, 5]) == float(torch.tensor(1e-12, dtype=torch.float32))
    else:
        e_b = _rel(dqkv, want_g)
        print(f"    dqkv {e_b:.3e} ({fp['bwd']:.3e})")
        assert e_b < bound(fp["bwd"], BWD_FLOOR)
    if F_ > 1:                                                            # frame 0 of the F-frame call: the bits of a 1-frame call
        o1, p1, g1, _ = run_attn(eng, dict(d, qkv=d["qkv"][:1], dout=d["dout"][:1]))
        assert torch.equal(out[:1], o1) and torch.equal(probs[:1], p1) and torch.equal(dqkv[:1], g1)


def test_the_shortcut_for_the_column_dot_products_is_algebra():
    """r_i = sum_t qh[t][i] dqh[t][i] = sum_j dG[i][j] Gh[i][j] and c_j likewise, in float64 on a random case."""
    T, dh = 25, 12
    qh, kh, dG = F.normalize(_rand(T, dh, seed=1), dim=0), F.normalize(_rand(T, dh, seed=2), dim=0), _rand(dh, dh, seed=3)
    Gh = qh.t() @ kh
    assert float(((qh * (kh @ dG.t())).sum(0) - (dG * Gh).sum(1)).abs().max()) < 1e-13
    assert float(((kh * (qh @ dG)).sum(0) - (dG * Gh).sum(0)).abs().max()) < 1e-13


@pytest.mark.parametrize("P,Cn,variant", mk.DW3_CASES)
def test_depthwise_host_twin_against_float64(eng, P, Cn, variant):
    d = mk.dw3_case(P, Cn, variant)
    y = eng.xcit_dw3(*[_f(d[k]) for k in ("x", "w", "b", "ta", "ts", "add", "ma", "mu")])
    assert _rel(y, mk.dw3_reference(d)) < bound(FP32["dw3"][mk.dw3_key(P, Cn, variant)], FWD_FLOOR)


@pytest.mark.parametrize("P,Cn,nchw", mk.STEM_CASES)
def test_stem_gather_and_scatter_host_twin(eng, P, Cn, nchw):
    d = mk.stem_case(P, Cn, nchw)
    assert torch.equal(eng.xcit_stem_gather(_f(d["src"]), nchw), mk.gather_reference(d["src"].float(), nchw))
    got = eng.xcit_stem_scatter(_f(d["drows"]), tuple(d["src"].shape), _f(d["pre"]), nchw)
    assert _rel(got, mk.scatter_reference(d)) < bound(FP32["scatter"][mk.stem_key(P, Cn, nchw)], BWD_FLOOR)
    if nchw:
        base = _rand(*d["src"].shape, seed=16).float()
        assert torch.equal(eng.xcit_stem_scatter(_f(d["drows"]), tuple(d["src"].shape), None, True, into=base.clone()), base + got)


def test_the_entries_refuse_with_the_reason(eng):
    z = torch.zeros(8192)
    p = lambda t: C.c_void_p(t.data_ptr())      # noqa: E731
    capi = eng.capi
    fwd = lambda *, q=p(z), frames=1, T=4, H=2, dh=8, t=p(z): capi.i2v_xcit_attention_f32(q, frames, T, H, dh, t, p(z), p(z), p(z), None)      # noqa: E731
    assert fwd() == 0 and fwd(H=1, dh=64) == 0                            # 64 is served
    off = C.c_void_p(z.data_ptr() + 4)
    for kw, why in ((dict(q=None), b"null"), (dict(t=None), b"null"), (dict(frames=0), b"positive"), (dict(dh=6), b"multiple of 4"),
                    (dict(H=1, dh=68), b"wider than 64"), (dict(frames=70000), b"65535"), (dict(frames=40000, T=196, H=8, dh=48), b"2^31"),
                    (dict(q=off), b"alignment")):
        assert fwd(**kw) != 0
        err = capi.i2v_last_error()
        assert b"xcit_attention" in err and b"hipErrorInvalidValue" in err and why in err, err
    bwd = lambda *, dh=8, g=p(z): capi.i2v_xcit_attention_bwd_f32(p(z), g, p(z), p(z), 1, 4, 2, dh, p(z), p(z), None)      # noqa: E731
    assert bwd() == 0
    for kw, why in ((dict(dh=6), b"multiple of 4"), (dict(g=None), b"null")):
        assert bwd(**kw) != 0
        assert b"xcit_attention_bwd" in capi.i2v_last_error() and why in capi.i2v_last_error()
    dw = lambda *, Cn=8, ts=p(z), y=C.c_void_p(z.data_ptr() + 4096): capi.i2v_xcit_dw3_f32(p(z), 1, 2, 2, Cn, p(z), None, p(z), ts, None, None, None, y, None)      # noqa: E731
    assert dw() == 0
    for kw, why in ((dict(Cn=6), b"multiple of 4"), (dict(ts=None), b"both of its arrays"), (dict(y=p(z)), b"overlap"), (dict(y=None), b"null")):
        assert dw(**kw) != 0
        assert b"xcit_dw3" in capi.i2v_last_error() and why in capi.i2v_last_error(), capi.i2v_last_error()
    assert capi.i2v_xcit_stem_gather_f32(p(z), None, 1, 5, 5, 3, 1, None) != 0 and b"null" in capi.i2v_last_error()
    assert capi.i2v_xcit_stem_scatter_f32(p(z), p(z), p(z), 1, 5, 5, 3, 1, 0, None) != 0 and b"pre-activation" in capi.i2v_last_error()
    assert capi.i2v_xcit_stem_scatter_f32(p(z), None, C.c_void_p(z.data_ptr() + 8192), 1, 5, 5, 4, 0, 1, None) != 0 and b"accumulates" in capi.i2v_last_error()


# ---- the attack classes, the CLI, the symbols --------------------------------------------------------------------------------------
def test_attack_classes_and_the_cli_take_the_names(tmp_path, monkeypatch):
    for name in NAMES:
        atk = attacks.ImageGuidedFMDirection_Adam([name], depth=4, step_size=0.005, steps=2, weight_seed=0)
        assert atk.model_names == [name]
    attacks.ImageGuidedStd_Adam([TINY], depth=1, step_size=0.005, weight_seed=0)
    attacks.AENS_I2V_MF([SMALL, "vgg", "convit_tiny"], depths={SMALL: [2, 4], "vgg": [2, 3], "convit_tiny": [1]}, step_size=0.005, weight_seed=0)
    with pytest.raises(KeyError):
        attacks.ImageGuidedFMDirection_Adam([SMALL], depth=5, step_size=0.005, weight_seed=0)
    with pytest.raises(ValueError, match="not a model of this table"):
        attacks.ImageGuidedFMDirection_Adam(["xcit_small_12_p8_224"], depth=2, step_size=0.005, weight_seed=0)
    import image_main
    monkeypatch.setattr(image_main, "OPT_PATH", str(tmp_path))
    base = ["--attack_method", "ImageGuidedFMDirection_Adam", "--step", "2"]
    for name in NAMES:
        for depth in ("1", "2", "3", "4"):
            a = image_main.arg_parse(base + ["--direction_image_model", name, "--depth", depth])
            assert image_main.build_attack(a).model_names == [name]
    for bad in (["--direction_image_model", "xcit_small_12_p8_224"], ["--direction_image_model", SMALL, "--depth", "5"],
                ["--direction_image_model", TINY, "--hw", "112"]):
        with pytest.raises(SystemExit):
            image_main.arg_parse(base + bad)


def test_new_native_symbols_are_exported_by_the_library_and_the_host_simulation():
    import __graft_entry__ as ge
    cd = C.CDLL(ge.LIB)
    assert all(hasattr(cd, n) for n in _lib.XCIT_EXPORTS)
    assert {"i2v_xcit_attention_f32", "i2v_xcit_attention_bwd_f32", "i2v_xcit_dw3_f32", "i2v_xcit_stem_gather_f32", "i2v_xcit_stem_scatter_f32",
            "i2v_xcit_create", "i2v_xcit_destroy", "i2v_xcit_workspace_bytes", "i2v_xcit_forward", "i2v_xcit_backward", "i2v_xcit_hook_info",
            "i2v_xcit_read_hook"} == set(_lib.XCIT_EXPORTS)
    assert not set(_lib.XCIT_EXPORTS) & (set(_lib.EXPORTS) | set(_lib.VIT_EXPORTS) | set(_lib.SWIN_EXPORTS) | set(_lib.LOADER_EXPORTS)
                                         | set(_lib.CONVNEXT_EXPORTS) | set(_lib.MIXER_EXPORTS) | set(_lib.CAIT_EXPORTS) | set(_lib.CONVIT_EXPORTS))
    assert {"i2v_xcit.hip", "i2v_xcit.cpp"} <= set(ge.UNITS) and "-DI2V_HAVE_XCIT" in ge.FLAGS
    assert {"i2v_xcit_host.h", "i2v_xcit_kernels.h"} <= set(ge.HEADERS)
    hs = C.CDLL(os.path.join(ROOT, "tests", "hostsim", "libi2v_hostsim.so"))
    assert all(hasattr(hs, n) for n in _lib.XCIT_EXPORTS) and not hasattr(hs, "i2v_swin_create") and not hasattr(hs, "i2v_vit_create")
    assert "I2V_HAVE_XCIT" not in open(os.path.join(ROOT, "tests", "hostsim", "build.sh")).read()
    header = open(os.path.join(ROOT, "include", "i2v_xcit.h")).read()
    assert all(n + "(" in header for n in _lib.XCIT_EXPORTS)


def test_planned_bytes_are_counted_in_64_bits_and_grow_as_the_saves_do():
    t = graphs.build("xcit_large_24_p16_224")
    assert 2 ** 33 < t.workspace_bytes([23], 128) < 2 ** 38               # past 32 bits
    T, D, H, dh = t.tokens, t.dim, t.heads, t.dim // t.heads
    per = lambda blocks: t.workspace_bytes(blocks, 3) - t.workspace_bytes(blocks, 2)       # noqa: E731
    # one more frame costs per further block: x, qkv, y1, u, y2 (7 D per token), h (4 D), six statistics, and per head the (dh + 2, dh) Gram
    # with its norms and the (dh, dh) probabilities
    assert per([7]) - per([6]) == 4 * (T * (11 * D + 6) + H * dh * (2 * dh + 2))
    assert graphs.build(SMALL).workspace_bytes([8], 128) == mk.WORKSPACE_SMALL_D3      # the figure of DESIGN.md section 23


# ---- the planner (csrc/i2v_xcit.cpp) on the host simulation ------------------------------------------------------------------------
@pytest.fixture(scope="module")
def twin_refs():
    """The float64 reference of each twin case, computed once: label -> (spec, sd, x, features, hook gradients, input gradient)."""
    out = {}
    for label, (side, _) in mk.TWINS.items():
        spec = graphs.build_tiny(SMALL, (side, side))
        sd = weights.synthetic_state_dict(spec, 0)
        x = mk.twin_input(label)
        ref = XcitReference(spec, sd, mk.TWIN_HOOKS)
        rf = ref.forward(x)
        hg = [_rand(*f.shape, seed=30 + i) for i, f in enumerate(rf)]
        out[label] = (spec, sd, x, rf, hg, ref.backward(hg))
    return out


@pytest.mark.parametrize("label", sorted(mk.TWINS))
def test_twin_on_the_host_simulation_against_float64(eng, twin_refs, label):
    """Features at all four depths and the input gradient with all four hook gradients flowing; a net planned for 5 frames gives the same
    bits, frame 0 the bits of a 1-frame run; hooks in another order; a single hook gives the same features and its own gradient."""
    spec, sd, x, rf, hg, want_gx = twin_refs[label]
    blocks = [spec.hook_for(d) for d in (1, 2, 3, 4)]
    assert blocks == mk.TWIN_HOOKS
    feats, gx = _run_twin(eng, spec, sd, blocks, x, hg)
    fp = FP32[label]
    errs, gerr = [_rel(a, b) for a, b in zip(feats, rf)], _rel(gx, want_gx)
    print(f"{label} on the host simulation vs float64: hooks {errs} grad {gerr}; fp32 CPU: {fp['hooks']} {fp['grad']}")
    for e, cpu in zip(errs, fp["hooks"]):
        assert e < bound(cpu, NET_FLOOR)
    assert gerr < bound(fp["grad"], NET_FLOOR)
    feats2, gx2 = _run_twin(eng, spec, sd, blocks, x, hg, max_frames=5)
    assert all(torch.equal(a, b) for a, b in zip(feats, feats2)) and torch.equal(gx, gx2)
    f1, g1 = _run_twin(eng, spec, sd, blocks, x[:1], [h[:1] for h in hg])
    assert all(torch.equal(a[:1], b) for a, b in zip(feats, f1)) and torch.equal(gx[:1], g1)
    fo, go = _run_twin(eng, spec, sd, blocks[::-1], x, hg[::-1])          # hooks in another order
    assert all(torch.equal(a, b) for a, b in zip(feats, fo[::-1])) and torch.equal(gx, go)
    fa, ga = _run_twin(eng, spec, sd, [blocks[1]], x, [hg[1]])            # one hook: the net is truncated there
    assert torch.equal(fa[0], feats[1])
    ref1 = XcitReference(spec, sd, [blocks[1]])
    ref1.forward(x)
    assert _rel(ga, ref1.backward([hg[1]])) < bound(fp["grad"], NET_FLOOR)


@pytest.mark.parametrize("fold", mk.FOLDS)
def test_leaving_a_fold_out_is_seen(eng, twin_refs, fold):
    """Each fold of `native_arrays` carries arithmetic: the reference without it (a BatchNorm skipped, a LayerScale or temperature of
    one, no position table) misses every hooked feature of the twin by more than 100 x the bound, and so does the library's result."""
    spec, sd, x, rf, hg, _ = twin_refs["xcit_test_80"]
    feats, _ = _run_twin(eng, spec, sd, mk.TWIN_HOOKS, x, hg)
    without = XcitReference(spec, sd, mk.TWIN_HOOKS, skip=(fold,)).forward(x)
    for got, want, wo, cpu in zip(feats, rf, without, FP32["xcit_test_80"]["hooks"]):
        assert _rel(wo, want) > 100 * bound(cpu, NET_FLOOR) and _rel(got, wo) > 100 * bound(cpu, NET_FLOOR)


def test_planner_refusals_on_the_host_simulation(eng):
    spec = graphs.build_tiny(SMALL, (64, 64))
    sd = weights.synthetic_state_dict(spec, 0)
    with pytest.raises(_lib.I2VError, match="hooked twice"):
        eng.build_xcit_net(spec, sd, [1, 1], 2)
    with pytest.raises(_lib.I2VError, match="outside"):
        eng.build_xcit_net(spec, sd, [8], 2)
    net = eng.build_xcit_net(spec, sd, [0], 2)
    with pytest.raises(_lib.I2VError, match="planned for"):
        net.forward(torch.zeros(3, 3, 64, 64))
    with pytest.raises(_lib.I2VError):
        net.forward(torch.zeros(2, 3, 32, 32))
    net.close()
    cfg = _lib.XcitConfig(64, 3, 136, 2, 544, 8, 1e-6)                     # heads of width 68
    h, one = C.c_void_p(), (C.c_int32 * 1)(0)
    assert eng.capi.i2v_xcit_create(0, C.byref(cfg), (C.c_void_p * 30)(), 30, one, 1, 1, C.byref(h)) != 0
    assert b"width 68" in eng.capi.i2v_last_error()


def test_i2v_trajectory_on_the_twin_matches_the_reference(eng):
    """4 steps of the I2V attack at depth 4 against `restate.run_attack` on the float32 reference net (costs at rtol 2e-4, as
    tests/test_convit_cpu.py)."""
    torch.manual_seed(5)
    vid = torch.randn(1, 3, 2, 64, 64)
    atk = attacks.ImageGuidedFMDirection_Adam([SMALL], depth=4, step_size=0.005, steps=4, engine=eng, graph_builder=graphs.build_tiny,
                                              weight_seed=0)
    adv = atk(vid, torch.zeros(1, dtype=torch.long), ["t"])
    g = graphs.build_tiny(SMALL, (64, 64))
    check_trajectory(atk, adv, XcitReference(g, weights.synthetic_state_dict(g, 0), [g.hook_for(4)], dtype=torch.float32), vid, rtol=2e-4, steps=4)


def test_aens_of_the_twin_with_tiny_resnet_matches_the_oracle(eng):
    torch.manual_seed(6)
    vid = torch.randn(1, 3, 2, 80, 80)
    depths = {SMALL: [1, 4], "resnet": [2, 3]}
    atk = attacks.AENS_I2V_MF([SMALL, "resnet"], depths=depths, step_size=0.005, steps=3, momentum=0.5, engine=eng,
                              graph_builder=graphs.build_tiny, weight_seed=0)
    _, _, costs = atk(vid, torch.zeros(1, dtype=torch.long), ["a"])
    cs, rs = (graphs.build_tiny(n, (80, 80)) for n in (SMALL, "resnet"))
    nets = [XcitReference(cs, weights.synthetic_state_dict(cs, 0), [cs.hook_for(d) for d in depths[SMALL]], dtype=torch.float32),
            restate.OracleNet(rs, weights.synthetic_state_dict(rs, 0), [rs.hook_for(d, True) for d in depths["resnet"]], dtype=torch.float32)]
    ref = restate.run_attack(nets, vid, steps=3, step_size=0.005, mode="aens", coeffs=torch.ones(4), momentum=0.5)
    np.testing.assert_allclose(costs, ref["costs"], rtol=2e-4)
