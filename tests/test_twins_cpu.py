"""CPU: timm's Twins family (PCPVT and SVT) as image surrogates on the transformer stack -- for every served name
the spec, the hooks and the key / shape contract against tests/golden/timm_twins_keys.json; the refusals; checkpoint loading; the repacks
of the native packing (the later patch embeddings, the sr convolution, the position encoding) against timm's literal arithmetic, and
that leaving the new arithmetic out is seen; the kernel entries (sub-sampled attention, the block gather / scatter, window attention at
shift 0) on the host simulation, which runs them as scalar code (csrc/i2v_twins_host.h); and the planner itself (csrc/i2v_twins.cpp) on
the host simulation: all three twins against float64, a 4-step I2V attack and an AENS ensemble against the oracle.

The bound is relative L2 against float64: the larger of the floor for that kind of case (entries 1e-6 forward, 1e-5 backward; nets 1e-5)
and 4 x the error of the float32 CPU run of the same reference on the same inputs, read from tests/golden/twins_fp32_cpu_errors.json
(tests/make_twins_fixtures.py).  A case without a recorded error fails (KeyError)."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from i2v_amd import attacks, graphs, weights
from i2v_amd import lib as _lib
from oracle import restate
from tests import make_twins_fixtures as mk
from tests.family_harness import bound, check_trajectory, rand as _rand, rel as _rel, run_twin as _run_twin
from tests.hostsim_util import hostsim_engine
from tests.twins_reference import TwinsReference

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = json.load(open(os.path.join(ROOT, "tests", "golden", "timm_twins_keys.json")))
FP32 = json.load(open(os.path.join(ROOT, "tests", "golden", "twins_fp32_cpu_errors.json")))
TABLE = {"twins_pcpvt_small": ((64, 128, 320, 512), (1, 2, 5, 8), (8, 8, 4, 4), (3, 4, 6, 3), 0),
         "twins_pcpvt_base": ((64, 128, 320, 512), (1, 2, 5, 8), (8, 8, 4, 4), (3, 4, 18, 3), 0),
         "twins_pcpvt_large": ((64, 128, 320, 512), (1, 2, 5, 8), (8, 8, 4, 4), (3, 8, 27, 3), 0),
         "twins_svt_small": ((64, 128, 256, 512), (2, 4, 8, 16), (4, 4, 4, 4), (2, 2, 10, 4), 7),
         "twins_svt_base": ((96, 192, 384, 768), (3, 6, 12, 24), (4, 4, 4, 4), (2, 2, 18, 2), 7),
         "twins_svt_large": ((128, 256, 512, 1024), (4, 8, 16, 32), (4, 4, 4, 4), (2, 2, 18, 2), 7)}
NAMES = sorted(TABLE)
PCPVT, SVT = "twins_pcpvt_small", "twins_svt_small"
NET_FLOOR, FWD_FLOOR, BWD_FLOOR = 1e-5, 1e-6, 1e-5


# ---- the specs ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_param_shapes_equal_the_key_fixture(name):
    want = {k: tuple(v) for k, v in KEYS["names"][name].items()}
    shapes = graphs.build(name).param_shapes()
    assert shapes == want and list(shapes) == list(want)
    assert KEYS["checked_against"].startswith(("timm ", "unchecked"))


@pytest.mark.parametrize("name", NAMES)
def test_spec_grids_widths_and_hooks_of_every_name(name):
    dims, heads, ratios, depths, window = TABLE[name]
    spec = graphs.build(name)
    assert isinstance(spec, graphs.TwinsSpec) and spec.arch == name and spec.video is False and spec.in_hw == (224, 224)
    assert (spec.img, spec.patch, spec.in_chans, spec.dims, spec.heads, spec.mlp_ratios, spec.depths, spec.window) == \
           (224, 4, 3, dims, heads, ratios, depths, window)
    assert (spec.sr_ratios, spec.ln_eps, spec.pe_eps, spec.stages) == ((8, 4, 2, 1), 1e-6, 1e-5, 4)
    assert [spec.grid(k) for k in range(4)] == [56, 28, 14, 7] and [spec.tokens(k) for k in range(4)] == [3136, 784, 196, 49]
    assert [spec.keys_per_frame(k) for k in range(4)] == [49] * 4                      # 49 keys at every stage
    assert all(d // h == (32 if window else 64) for d, h in zip(dims, heads))
    hooks = [spec.hook_for(d) for d in (1, 2, 3, 4)]
    assert hooks == [0, 1, 2, 3] and [spec.hook_dim(s) for s in hooks] == [3136 * dims[0], 784 * dims[1], 196 * dims[2], 49 * dims[3]]
    if name == PCPVT:
        assert [spec.hook_dim(s) for s in hooks] == [200704, 100352, 62720, 25088]
    with pytest.raises(KeyError):
        spec.hook_for(5)
    assert graphs.twins_named(name) == spec and graphs.is_twins_name(name)
    assert not any(f(name) for f in (graphs.is_swin_name, graphs.is_vit_name, graphs.is_convnext_name, graphs.is_mixer_name, graphs.is_cait_name,
                                     graphs.is_convit_name, graphs.is_xcit_name))
    assert [spec.is_lsa(2, j) for j in range(4)] == ([True, False, True, False] if window else [False] * 4)
    shapes = spec.param_shapes()
    assert shapes["patch_embeds.0.proj.weight"] == (dims[0], 3, 4, 4) and shapes["patch_embeds.3.proj.weight"] == (dims[3], dims[2], 2, 2)
    assert shapes["pos_block.2.proj.0.weight"] == (dims[2], 1, 3, 3)
    gsa = 1 if window else 0                                                           # a GSA block of each stage
    assert shapes[f"blocks.0.{gsa}.attn.sr.weight"] == (dims[0], dims[0], 8, 8) and shapes[f"blocks.2.{gsa}.attn.kv.weight"] == (2 * dims[2], dims[2])
    assert f"blocks.3.{gsa}.attn.sr.weight" not in shapes and f"blocks.3.{gsa}.attn.norm.weight" not in shapes      # sr = 1: neither key
    assert ("blocks.1.0.attn.qkv.weight" in shapes) == bool(window) and ("blocks.1.0.attn.q.weight" in shapes) == (not window)
    assert not any(k.startswith(("head.", "norm.")) for k in shapes)
    for hw in ((384, 384), (112, 112), (224, 192)):
        with pytest.raises(ValueError, match="224 x 224") as ei:
            graphs.build(name, hw)
        assert all(n in str(ei.value) for n in TABLE)


def test_refusals_name_the_reason_and_list_the_served_names():
    for name in ("twins_", "twins_pcpvt_tiny", "twins_svt_huge", "twins_pcpvt_small_384"):
        assert graphs.is_twins_name(name)
        with pytest.raises(ValueError, match="not a model of this table") as ei:
            graphs.build(name)
        assert all(n in str(ei.value) for n in TABLE)
        with pytest.raises(ValueError, match="not a model of this table"):
            graphs.build_tiny(name)


def test_existing_names_behave_as_before():
    with pytest.raises(UnboundLocalError):
        graphs.build("transformer")
    with pytest.raises(UnboundLocalError):
        graphs.build("pit_s_224")
    with pytest.raises(UnboundLocalError):
        graphs.build("twin_pcpvt_small")
    with pytest.raises(ValueError, match="not served"):
        graphs.build("mobilenet_v2")
    assert not any(graphs.is_twins_name(n) for n in ("convnext_tiny", "vit_base_patch16_224", "swin_tiny_patch4_window7_224", "xcit_nano_12_p16_224",
                                                     "resnet", "conv"))
    assert isinstance(graphs.build("xcit_nano_12_p16_224"), graphs.XcitSpec) and isinstance(graphs.build("convit_tiny"), graphs.ConvitSpec)
    assert isinstance(graphs.build("swin_tiny_patch4_window7_224"), graphs.SwinSpec) and graphs.build("resnet").arch == "resnet101"
    others = (set(graphs.SWIN_MODELS) | set(graphs.VIT_MODELS) | set(graphs.CONVNEXT_MODELS) | set(graphs.MIXER_MODELS) | set(graphs.CAIT_MODELS)
              | set(graphs.CONVIT_MODELS) | set(graphs.XCIT_MODELS))
    assert not set(graphs.TWINS_MODELS) & others and graphs.TWINS_MODELS == TABLE


# ---- checkpoints -------------------------------------------------------------------------------------------------------------------
def _checkpoint(spec):
    """A timm-shaped checkpoint with the keys behind every hook as well."""
    D = spec.dims[3]
    sd = {k: torch.zeros(1).expand(shp) for k, shp in spec.param_shapes().items()}
    sd.update({"norm.weight": torch.ones(D), "norm.bias": torch.zeros(D), "head.weight": torch.zeros(1).expand(1000, D), "head.bias": torch.zeros(1000)})
    return sd


@pytest.mark.parametrize("name", [PCPVT, "twins_svt_base"])
def test_checkpoint_loads_from_its_own_file(name, tmp_path, monkeypatch):
    spec = graphs.build(name)
    monkeypatch.delenv("I2V_SYNTHETIC_WEIGHTS", raising=False)
    monkeypatch.setenv("I2V_WEIGHTS_DIR", str(tmp_path))
    with pytest.raises(weights.MissingWeights, match=name):
        weights.load_state_dict(spec)
    sd = _checkpoint(spec)
    sd["pos_block.1.proj.0.bias"] = torch.full((spec.dims[1],), 0.25)
    torch.save(sd, tmp_path / f"{name}.pth")
    got = weights.load_state_dict(spec)
    assert list(got) == list(spec.param_shapes()) and "head.weight" not in got
    assert all(tuple(got[k].shape) == shp and got[k].is_contiguous() for k, shp in spec.param_shapes().items())
    assert float(got["pos_block.1.proj.0.bias"].mean()) == 0.25
    with pytest.raises(weights.MissingWeights):                             # every name reads its own file
        weights.load_state_dict(graphs.build("twins_pcpvt_base" if name == PCPVT else SVT))


def test_misshaped_and_missing_keys_are_refused_by_key(tmp_path, monkeypatch):
    monkeypatch.setenv("I2V_WEIGHTS_DIR", str(tmp_path))
    for name, bad, shape, gone in ((PCPVT, "blocks.1.2.attn.sr.weight", (128, 128, 2, 2), "pos_block.3.proj.0.weight"),
                                   (SVT, "blocks.2.1.attn.kv.weight", (256, 256), "blocks.0.0.attn.qkv.bias")):
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
    spec = graphs.build(PCPVT)
    sd = weights.load_state_dict(spec, seed=3)
    assert {k: tuple(v.shape) for k, v in sd.items()} == spec.param_shapes()
    for k in range(4):
        w, b = sd[f"pos_block.{k}.proj.0.weight"], sd[f"pos_block.{k}.proj.0.bias"]
        assert float(w.std()) > 0.2 and float(b.abs().mean()) > 0.03
        g = sd[f"patch_embeds.{k}.norm.weight"]
        assert 0.5 <= float(g.min()) and float(g.max()) <= 1.5 and float(g.std()) > 0.2
    for k in range(3):
        g, s = sd[f"blocks.{k}.1.attn.norm.weight"], sd[f"blocks.{k}.1.attn.norm.bias"]
        assert 0.5 <= float(g.min()) and float(g.max()) <= 1.5 and float(g.std()) > 0.2 and float(s.abs().mean()) > 0.03
        assert float(sd[f"blocks.{k}.1.attn.sr.weight"].std()) > 0 and float(sd[f"blocks.{k}.1.attn.sr.bias"].abs().mean()) > 0.03


def test_test_size_twins():
    t = graphs.build_tiny(PCPVT, (64, 64))
    assert t == graphs.build_tiny("twins_pcpvt_large", (64, 64)) == graphs.twins_tiny_twin()
    assert t.arch == "twins_pcpvt_test" and [t.grid(k) for k in range(4)] == [16, 8, 4, 2] and [t.keys_per_frame(k) for k in range(4)] == [4] * 4
    t96 = graphs.build_tiny("twins_pcpvt_base", (96, 96))
    assert t96.arch == "twins_pcpvt_test_96" and [t96.grid(k) for k in range(4)] == [24, 12, 6, 3]
    assert [t96.tokens(k) for k in range(4)] == [576, 144, 36, 9] and [t96.keys_per_frame(k) for k in range(4)] == [9] * 4
    assert any(t96.tokens(k) % 64 for k in range(4)) and all(d // h == 12 for d, h in zip(t96.dims, t96.heads))
    ts = graphs.build_tiny("twins_svt_large", (128, 128))
    assert ts == graphs.build_tiny(SVT, (128, 128)) and ts.arch == "twins_svt_test" and ts.window == 4
    assert [ts.grid(k) for k in range(4)] == [32, 16, 8, 4] and [ts.keys_per_frame(k) for k in range(4)] == [16] * 4
    assert all(d // h == 16 for d, h in zip(ts.dims, ts.heads))
    for tw in (t, t96, ts, graphs.build_tiny(SVT, (224, 224))):
        assert tw.arch not in graphs.TWINS_MODELS and all(d >= 2 for d in tw.depths) and tw.sr_ratios == (8, 4, 2, 1)
        assert tw.hooks == {1: 0, 2: 1, 3: 2, 4: 3}
    for name, hw in ((PCPVT, (72, 72)), (SVT, (64, 64)), (SVT, (96, 96)), (PCPVT, (64, 96))):
        with pytest.raises(ValueError):
            graphs.build_tiny(name, hw)
    ref = TwinsReference(ts, weights.synthetic_state_dict(ts, 0), [0, 3])
    f = ref.forward(torch.randn(2, 3, 128, 128))
    assert [tuple(a.shape) for a in f] == [(2, 1024 * 16), (2, 16 * 128)]
    assert ref.backward([torch.ones_like(a) for a in f]).shape == (2, 3, 128, 128)


def test_native_arrays_repack_to_the_gathers_column_orders():
    """The sr convolution and the later patch embeddings as a gather and a Linear on the repacked weight equal `conv2d`, in float64."""
    import torch.nn.functional as F
    spec = graphs.build_tiny(PCPVT, (64, 64))
    sd = {k: v.double() for k, v in weights.synthetic_state_dict(spec, 0).items()}
    arrays = spec.native_arrays(sd, 2)
    x = _rand(2, 16, 16, 16, seed=1)                                       # stage 0's plane, token-major
    srw = arrays[4 + 2 + 4 + 0]                                             # embedding (4), norm1 (2), q and kv (4): then attn.sr
    assert srw.shape == (16, 8 * 8 * 16)
    want = F.conv2d(x.permute(0, 3, 1, 2), sd["blocks.0.0.attn.sr.weight"], None, stride=8).permute(0, 2, 3, 1).reshape(-1, 16)
    assert _rel(mk.gather_reference(x, 8) @ srw.double().t(), want) < 1e-6
    n0 = 4 + len(spec.block_keys(0, 0)) + 2 + len(spec.block_keys(0, 1))
    pew = arrays[n0]
    assert pew.shape == (32, 4 * 16)
    merged = x.reshape(2, 8, 2, 8, 2, 16).permute(0, 1, 3, 4, 2, 5).reshape(-1, 64)          # quarter dy + 2 dx: the merge gather's order
    want = F.conv2d(x.permute(0, 3, 1, 2), sd["patch_embeds.1.proj.weight"], None, stride=2).permute(0, 2, 3, 1).reshape(-1, 32)
    assert _rel(merged @ pew.double().t(), want) < 1e-6
    peg = arrays[4 + len(spec.block_keys(0, 0))]
    assert peg.shape == (9, 16) and torch.equal(peg[5], sd["pos_block.0.proj.0.weight"][:, 0, 1, 2].float())


# ---- the entries on the host simulation --------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def eng():
    e = hostsim_engine()
    _lib.bind(e.capi, _lib._TWINS_PROTOS)
    return e


def _f(v):
    return None if v is None else v.float().contiguous()


def run_attn(eng, d):
    q, kv = _f(d["q"]), _f(d["kv"])
    out = eng.twins_attention(q, kv, d["heads"])
    dq, dkv = eng.twins_attention_bwd(q, kv, _f(d["dout"]), d["heads"])
    return out, dq, dkv


@pytest.mark.parametrize("F_,Tq,Tk,H,dh,kind", mk.ATTN_CASES)
def test_attention_host_twin_against_float64_autograd(eng, F_, Tq, Tk, H, dh, kind):
    d = mk.attn_case(F_, Tq, Tk, H, dh, kind)
    out, dq, dkv = run_attn(eng, d)
    want, want_q, want_kv = mk.attn_reference(d)
    fp = FP32["attention"][mk.case_key(F_, Tq, Tk, H, dh, kind)]
    e_f = _rel(out, want)
    print(f"gsa F {F_} Tq {Tq} Tk {Tk} H {H} dh {dh} {kind}: out {e_f:.3e} (fp32 CPU {fp['fwd']:.3e})")
    assert e_f < bound(fp["fwd"], FWD_FLOOR)
    e_kv = _rel(dkv, want_kv)
    assert e_kv < bound(fp["dkv"], BWD_FLOOR)
    if Tk == 1:                                                            # a single key: P = 1, dS = 0, dq = 0
        assert float(dq.abs().max()) == 0.0 and float(want_q.abs().max()) < 1e-12
        assert _rel(out, d["kv"][:, :, H * dh:].expand(F_, Tq, H * dh)) < 1e-7
    else:
        assert _rel(dq, want_q) < bound(fp["dq"], BWD_FLOOR)
    if F_ > 1:                                                             # frame 0 of the F-frame call: the bits of a 1-frame call
        o1, q1, k1 = run_attn(eng, dict(d, q=d["q"][:1], kv=d["kv"][:1], dout=d["dout"][:1]))
        assert torch.equal(out[:1], o1) and torch.equal(dq[:1], q1) and torch.equal(dkv[:1], k1)


def test_window_host_twin_against_float64_autograd(eng):
    d = mk.window_case()
    out = eng.twins_window_attention(_f(d["qkv"]), d["grid"], d["window"], d["heads"])
    dqkv = eng.twins_window_attention(_f(d["qkv"]), d["grid"], d["window"], d["heads"], dout=_f(d["dout"]))
    want, want_g = mk.window_reference(d)
    assert _rel(out, want) < bound(FP32["window"]["fwd"], FWD_FLOOR) and _rel(dqkv, want_g) < bound(FP32["window"]["bwd"], BWD_FLOOR)


@pytest.mark.parametrize("s,H,W", mk.BLOCK_CASES)
def test_block_gather_and_scatter_host_twin_are_exact(eng, s, H, W):
    d = mk.block_case(s, H, W)
    assert torch.equal(eng.twins_block_gather(d["x"], s), mk.gather_reference(d["x"], s))
    want = mk.scatter_reference(d["drows"], tuple(d["x"].shape), s)
    assert torch.equal(eng.twins_block_scatter(d["drows"], tuple(d["x"].shape), s), want)
    assert torch.equal(eng.twins_block_scatter(d["drows"], tuple(d["x"].shape), s, into=d["base"].clone()), d["base"] + want)
    assert torch.equal(mk.scatter_reference(mk.gather_reference(d["x"], s), tuple(d["x"].shape), s), d["x"])      # a permutation


def test_the_entries_refuse_with_the_reason(eng):
    z = torch.zeros(16384)
    p = lambda t: C.c_void_p(t.data_ptr())      # noqa: E731
    capi = eng.capi
    fwd = lambda *, q=p(z), kv=p(z), frames=1, Tq=4, Tk=4, H=2, dh=8: capi.i2v_twins_attention_f32(q, kv, frames, Tq, Tk, H, dh, 0.5, p(z), None)      # noqa: E731
    assert fwd() == 0 and fwd(H=1, dh=64, Tk=64) == 0                      # the limits are served
    off = C.c_void_p(z.data_ptr() + 4)
    for kw, why in ((dict(q=None), b"null"), (dict(kv=None), b"null"), (dict(frames=0), b"positive"), (dict(dh=6), b"multiple of 4"),
                    (dict(H=1, dh=68), b"wider than 64"), (dict(Tk=65), b"more than 64 keys"), (dict(frames=70000), b"65535"),
                    (dict(frames=40000, Tq=3136, H=1, dh=64), b"2^31"), (dict(q=off), b"alignment"), (dict(kv=off), b"alignment")):
        assert fwd(**kw) != 0
        err = capi.i2v_last_error()
        assert b"twins_attention" in err and b"hipErrorInvalidValue" in err and why in err, err
    bwd = lambda *, dh=8, Tk=4, g=p(z): capi.i2v_twins_attention_bwd_f32(p(z), p(z), g, 1, 4, Tk, 2, dh, 0.5, p(z), p(z), None)      # noqa: E731
    assert bwd() == 0
    for kw, why in ((dict(dh=6), b"multiple of 4"), (dict(Tk=65), b"more than 64 keys"), (dict(g=None), b"null")):
        assert bwd(**kw) != 0
        assert b"twins_attention_bwd" in capi.i2v_last_error() and why in capi.i2v_last_error()
    y = C.c_void_p(z.data_ptr() + 32768)
    ga = lambda *, s=2, H=4, Cn=8, out=y: capi.i2v_twins_block_gather_f32(p(z), out, 1, H, 4, Cn, s, None)      # noqa: E731
    assert ga() == 0
    for kw, why in ((dict(s=3), b"2, 4 or 8"), (dict(H=6, s=4), b"whole number of blocks"), (dict(Cn=6), b"multiple of 4"), (dict(out=None), b"null"),
                    (dict(out=p(z)), b"overlap")):
        assert ga(**kw) != 0
        assert b"twins_block_gather" in capi.i2v_last_error() and why in capi.i2v_last_error(), capi.i2v_last_error()
    assert capi.i2v_twins_block_scatter_f32(p(z), y, 1, 4, 4, 8, 16, 0, None) != 0 and b"twins_block_scatter" in capi.i2v_last_error()
    assert capi.i2v_twins_window_attention_f32(p(z), 1, 8, 8, 4, 2, 32, None, y, None) != 0 and b"head width 16" in capi.i2v_last_error()


# ---- the attack classes, the CLI, the symbols --------------------------------------------------------------------------------------
def test_attack_classes_and_the_cli_take_the_names(tmp_path, monkeypatch):
    for name in NAMES:
        atk = attacks.ImageGuidedFMDirection_Adam([name], depth=4, step_size=0.005, steps=2, weight_seed=0)
        assert atk.model_names == [name]
    attacks.ImageGuidedStd_Adam([SVT], depth=1, step_size=0.005, weight_seed=0)
    attacks.ImageGuidedFML2_Adam_MultiModels([PCPVT, "resnet"], depths={PCPVT: 2, "resnet": 3}, weight_seed=0)
    attacks.AENS_I2V_MF([PCPVT, "vgg", "xcit_nano_12_p16_224"], depths={PCPVT: [2, 4], "vgg": [2, 3], "xcit_nano_12_p16_224": [1]}, step_size=0.005,
                        weight_seed=0)
    with pytest.raises(KeyError):
        attacks.ImageGuidedFMDirection_Adam([SVT], depth=5, step_size=0.005, weight_seed=0)
    with pytest.raises(ValueError, match="not a model of this table"):
        attacks.ImageGuidedFMDirection_Adam(["twins_svt_tiny"], depth=2, step_size=0.005, weight_seed=0)
    import image_main
    monkeypatch.setattr(image_main, "OPT_PATH", str(tmp_path))
    base = ["--attack_method", "ImageGuidedFMDirection_Adam", "--step", "2"]
    for name in NAMES:
        for depth in ("1", "2", "3", "4"):
            a = image_main.arg_parse(base + ["--direction_image_model", name, "--depth", depth])
            assert image_main.build_attack(a).model_names == [name]
    for bad in (["--direction_image_model", "twins_svt_tiny"], ["--direction_image_model", SVT, "--depth", "5"],
                ["--direction_image_model", PCPVT, "--hw", "112"]):
        with pytest.raises(SystemExit):
            image_main.arg_parse(base + bad)


def test_new_native_symbols_are_exported_by_the_library_and_the_host_simulation():
    import __graft_entry__ as ge
    cd = C.CDLL(ge.LIB)
    assert all(hasattr(cd, n) for n in _lib.TWINS_EXPORTS)
    assert {"i2v_twins_create", "i2v_twins_destroy", "i2v_twins_workspace_bytes", "i2v_twins_forward", "i2v_twins_backward", "i2v_twins_hook_info",
            "i2v_twins_read_hook", "i2v_twins_attention_f32", "i2v_twins_attention_bwd_f32", "i2v_twins_block_gather_f32",
            "i2v_twins_block_scatter_f32", "i2v_twins_window_attention_f32", "i2v_twins_window_attention_bwd_f32"} == set(_lib.TWINS_EXPORTS)
    assert not set(_lib.TWINS_EXPORTS) & (set(_lib.EXPORTS) | set(_lib.VIT_EXPORTS) | set(_lib.SWIN_EXPORTS) | set(_lib.LOADER_EXPORTS)
                                          | set(_lib.CONVNEXT_EXPORTS) | set(_lib.MIXER_EXPORTS) | set(_lib.CAIT_EXPORTS) | set(_lib.CONVIT_EXPORTS)
                                          | set(_lib.XCIT_EXPORTS))
    assert {"i2v_twins.hip", "i2v_twins.cpp"} <= set(ge.UNITS) and "-DI2V_HAVE_TWINS" in ge.FLAGS
    assert {"i2v_twins_host.h", "i2v_twins_kernels.h"} <= set(ge.HEADERS)
    hs = C.CDLL(os.path.join(ROOT, "tests", "hostsim", "libi2v_hostsim.so"))
    assert all(hasattr(hs, n) for n in _lib.TWINS_EXPORTS) and not hasattr(hs, "i2v_swin_create")
    assert "I2V_HAVE_TWINS" not in open(os.path.join(ROOT, "tests", "hostsim", "build.sh")).read()
    header = open(os.path.join(ROOT, "include", "i2v_twins.h")).read()
    assert all(n + "(" in header for n in _lib.TWINS_EXPORTS)


def test_planned_bytes_are_counted_in_64_bits_and_grow_as_the_saves_do():
    t = graphs.build("twins_svt_large")
    assert 2 ** 33 < t.workspace_bytes([3], 128) < 2 ** 38                 # past 32 bits
    p = graphs.build(PCPVT)
    per = lambda st: p.workspace_bytes(st, 3) - p.workspace_bytes(st, 2)       # noqa: E731
    # one more frame costs, for stage 3 (sr 1, 49 tokens, width 512, MLP 2048, 3 GSA blocks): the embedding with two statistics and the
    # output stream; per block x, y, q (3 D), kv (2 D), h and four statistics; its hook view in place of stage 2's.  The stream-sized
    # scratch is stage 0's already; the four key-side planes grow from 49 keys of width 320 to 49 of width 512.
    T, D, M = 49, 512, 2048
    assert per([3]) - per([2]) == 4 * (T * (D + 2) + T * D + 3 * T * (5 * D + M + 4) + T * D - 196 * 320 + 4 * 49 * (512 - 320))


# ---- the planner (csrc/i2v_twins.cpp) on the host simulation -----------------------------------------------------------------------
@pytest.fixture(scope="module")
def twin_refs():
    """The float64 reference of each twin case, computed once: label -> (spec, sd, x, features, hook gradients, input gradient)."""
    out = {}
    for label, (name, side, _) in mk.TWINS.items():
        spec = graphs.build_tiny(name, (side, side))
        sd = weights.synthetic_state_dict(spec, 0)
        x = mk.twin_input(label)
        ref = TwinsReference(spec, sd, mk.HOOKS)
        rf = ref.forward(x)
        hg = [_rand(*f.shape, seed=30 + i) for i, f in enumerate(rf)]
        out[label] = (spec, sd, x, rf, hg, ref.backward(hg))
    return out


@pytest.mark.parametrize("label", sorted(mk.TWINS))
def test_twin_on_the_host_simulation_against_float64(eng, twin_refs, label):
    """Features at all four depths and the input gradient with all four hook gradients flowing; a net planned for 5 frames gives the same
    bits, frame 0 the bits of a 1-frame run; hooks in another order; a single hook gives the same features and its own gradient."""
    spec, sd, x, rf, hg, want_gx = twin_refs[label]
    stages = [spec.hook_for(d) for d in (1, 2, 3, 4)]
    assert stages == mk.HOOKS and spec.arch == label
    feats, gx = _run_twin(eng, spec, sd, stages, x, hg)
    fp = FP32[label]
    errs, gerr = [_rel(a, b) for a, b in zip(feats, rf)], _rel(gx, want_gx)
    print(f"{label} on the host simulation vs float64: hooks {errs} grad {gerr}; fp32 CPU: {fp['hooks']} {fp['grad']}")
    for e, cpu in zip(errs, fp["hooks"]):
        assert e < bound(cpu, NET_FLOOR)
    assert gerr < bound(fp["grad"], NET_FLOOR)
    feats2, gx2 = _run_twin(eng, spec, sd, stages, x, hg, max_frames=5)
    assert all(torch.equal(a, b) for a, b in zip(feats, feats2)) and torch.equal(gx, gx2)
    f1, g1 = _run_twin(eng, spec, sd, stages, x[:1], [h[:1] for h in hg])
    assert all(torch.equal(a[:1], b) for a, b in zip(feats, f1)) and torch.equal(gx[:1], g1)
    fo, go = _run_twin(eng, spec, sd, stages[::-1], x, hg[::-1])          # hooks in another order
    assert all(torch.equal(a, b) for a, b in zip(feats, fo[::-1])) and torch.equal(gx, go)
    fa, ga = _run_twin(eng, spec, sd, [stages[1]], x, [hg[1]])            # one hook: the net is truncated there
    assert torch.equal(fa[0], feats[1])
    ref1 = TwinsReference(spec, sd, [stages[1]])
    ref1.forward(x)
    assert _rel(ga, ref1.backward([hg[1]])) < bound(fp["grad"], NET_FLOOR)


@pytest.mark.parametrize("label", ["twins_pcpvt_test_96", "twins_svt_test"])
def test_twin_on_the_shared_launch_route_against_float64(eng, twin_refs, label, monkeypatch):
    """I2V_TWINS_ATTN=0, read when the net is planned: the GSA core as gemm + softmax + gemm with P kept, backward the softmax
    backward and four products.  The same bound; the plan holds the probabilities and one array of scratch more, as the formula says;
    a net planned without the switch afterwards is the attention launch's again."""
    spec, sd, x, rf, hg, want_gx = twin_refs[label]
    plain = spec.workspace_bytes(mk.HOOKS, x.shape[0], composed=False)
    monkeypatch.setenv("I2V_TWINS_ATTN", "0")
    feats, gx = _run_twin(eng, spec, sd, mk.HOOKS, x, hg)                  # (checks the planned bytes against the formula under the switch)
    gsa = [(k, j) for k in range(4) for j in range(spec.depths[k]) if not spec.is_lsa(k, j)]
    probs = [x.shape[0] * spec.tokens(k) * spec.heads[k] * ((spec.keys_per_frame(k) + 3) // 4 * 4) for k, _ in gsa]
    assert spec.workspace_bytes(mk.HOOKS, x.shape[0]) - plain == 4 * (sum(probs) + max(probs))
    fp = FP32[label]
    for e, cpu in zip([_rel(a, b) for a, b in zip(feats, rf)], fp["hooks"]):
        assert e < bound(cpu, NET_FLOOR)
    assert _rel(gx, want_gx) < bound(fp["grad"], NET_FLOOR)
    f1, g1 = _run_twin(eng, spec, sd, mk.HOOKS, x[:1], [h[:1] for h in hg])
    assert all(torch.equal(a[:1], b) for a, b in zip(feats, f1)) and torch.equal(gx[:1], g1)
    monkeypatch.delenv("I2V_TWINS_ATTN")
    feats0, gx0 = _run_twin(eng, spec, sd, mk.HOOKS, x, hg)
    assert all(_rel(a, b) < 1e-5 for a, b in zip(feats, feats0)) and _rel(gx, gx0) < 1e-5


def test_the_window_7_twin_of_the_224_probe_runs_through_the_planner(eng):
    """SVT names at 224 x 224 map to a window-7 twin, so that the attack classes' probe of a builder passes; one frame through the
    planner on the host simulation against float64, features at every hook and the input gradient."""
    (label, (name, side, _)), = mk.PROBE.items()
    spec = graphs.build_tiny(name, (side, side))
    assert spec.arch == label and spec.window == 7 and all(d // h == 32 for d, h in zip(spec.dims, spec.heads))
    sd, x = weights.synthetic_state_dict(spec, 0), mk.twin_input(label)
    ref = TwinsReference(spec, sd, mk.HOOKS)
    rf = ref.forward(x)
    hg = [_rand(*f.shape, seed=30 + i) for i, f in enumerate(rf)]
    feats, gx = _run_twin(eng, spec, sd, mk.HOOKS, x, hg)
    for e, cpu in zip([_rel(a, b) for a, b in zip(feats, rf)], FP32[label]["hooks"]):
        assert e < bound(cpu, NET_FLOOR)
    assert _rel(gx, ref.backward(hg)) < bound(FP32[label]["grad"], NET_FLOOR)


@pytest.mark.parametrize("what", ["peg", "sr_norm"])
def test_leaving_the_new_arithmetic_out_is_seen(eng, twin_refs, what):
    """The position encoding and the sub-sampled plane's LayerNorm carry arithmetic: the reference without either misses the hooked
    features of the odd twin by more than 100 x the bound, and so does the library's result."""
    spec, sd, x, rf, hg, _ = twin_refs["twins_pcpvt_test_96"]
    feats, _ = _run_twin(eng, spec, sd, mk.HOOKS, x, hg)
    without = TwinsReference(spec, sd, mk.HOOKS, skip=(what,)).forward(x)
    for got, want, wo, cpu in zip(feats, rf, without, FP32["twins_pcpvt_test_96"]["hooks"]):
        assert _rel(wo, want) > 100 * bound(cpu, NET_FLOOR) and _rel(got, wo) > 100 * bound(cpu, NET_FLOOR)


def test_planner_refusals_on_the_host_simulation(eng):
    spec = graphs.build_tiny(PCPVT, (64, 64))
    sd = weights.synthetic_state_dict(spec, 0)
    with pytest.raises(_lib.I2VError, match="hooked twice"):
        eng.build_twins_net(spec, sd, [1, 1], 2)
    with pytest.raises(_lib.I2VError, match="outside"):
        eng.build_twins_net(spec, sd, [4], 2)
    net = eng.build_twins_net(spec, sd, [0], 2)
    with pytest.raises(_lib.I2VError, match="planned for"):
        net.forward(torch.zeros(3, 3, 64, 64))
    with pytest.raises(_lib.I2VError):
        net.forward(torch.zeros(2, 3, 32, 32))
    net.close()
    four = lambda *v: (C.c_int32 * 4)(*v)      # noqa: E731
    cfg = _lib.TwinsConfig(256, 3, 4, 4, 0, four(16, 32, 40, 64), four(1, 2, 5, 8), four(64, 128, 80, 128), four(2, 2, 2, 2), four(4, 4, 2, 1),
                           1e-6, 1e-5)                                      # stage 0: a 64 x 64 grid under sr 4 is 256 keys
    h, one = C.c_void_p(), (C.c_int32 * 1)(0)
    assert eng.capi.i2v_twins_create(0, C.byref(cfg), (C.c_void_p * 40)(), 40, one, 1, 1, C.byref(h)) != 0
    assert b"256 keys" in eng.capi.i2v_last_error()


def test_i2v_trajectory_on_the_twin_matches_the_reference(eng):
    """4 steps of the I2V attack at depth 4 against `restate.run_attack` on the float32 reference net (costs at rtol 2e-4, as
    tests/test_xcit_cpu.py)."""
    torch.manual_seed(5)
    vid = torch.randn(1, 3, 2, 64, 64)
    atk = attacks.ImageGuidedFMDirection_Adam([PCPVT], depth=4, step_size=0.005, steps=4, engine=eng, graph_builder=graphs.build_tiny,
                                              weight_seed=0)
    adv = atk(vid, torch.zeros(1, dtype=torch.long), ["t"])
    g = graphs.build_tiny(PCPVT, (64, 64))
    check_trajectory(atk, adv, TwinsReference(g, weights.synthetic_state_dict(g, 0), [g.hook_for(4)], dtype=torch.float32), vid, rtol=2e-4, steps=4)


def test_aens_of_the_twin_with_tiny_resnet_matches_the_oracle(eng):
    torch.manual_seed(6)
    vid = torch.randn(1, 3, 2, 96, 96)
    depths = {PCPVT: [1, 4], "resnet": [2, 3]}
    atk = attacks.AENS_I2V_MF([PCPVT, "resnet"], depths=depths, step_size=0.005, steps=3, momentum=0.5, engine=eng,
                              graph_builder=graphs.build_tiny, weight_seed=0)
    _, _, costs = atk(vid, torch.zeros(1, dtype=torch.long), ["a"])
    cs, rs = (graphs.build_tiny(n, (96, 96)) for n in (PCPVT, "resnet"))
    nets = [TwinsReference(cs, weights.synthetic_state_dict(cs, 0), [cs.hook_for(d) for d in depths[PCPVT]], dtype=torch.float32),
            restate.OracleNet(rs, weights.synthetic_state_dict(rs, 0), [rs.hook_for(d, True) for d in depths["resnet"]], dtype=torch.float32)]
    ref = restate.run_attack(nets, vid, steps=3, step_size=0.005, mode="aens", coeffs=torch.ones(4), momentum=0.5)
    np.testing.assert_allclose(costs, ref["costs"], rtol=2e-4)
