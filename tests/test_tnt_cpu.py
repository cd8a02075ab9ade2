"""CPU: timm's TNT family as image surrogates on the transformer stack -- for the two served names the spec,
the hooks and the key / shape contract against tests/golden/timm_tnt_keys.json; the refusals; the packing (qk stacked on v, the padded
pixel filter, pixel_pos pixel-major); the kernel entries on the host simulation, which runs them as scalar code (csrc/i2v_tnt_host.h);
and the planner itself (csrc/i2v_tnt.cpp) on the host simulation: both twins against float64, and a 10-step I2V attack against the oracle.

The bound is relative L2 against float64: the larger of the floor for that kind of case (entries 1e-6 forward, 1e-5 backward; nets 1e-5)
and 4 x the error of the float32 CPU run of the same reference on the same inputs, read from tests/golden/tnt_fp32_cpu_errors.json
(tests/make_tnt_fixtures.py).  A case without a recorded error fails (KeyError)."""
import ctypes as C
import json
import os

import pytest
import torch

from i2v_amd import attacks, graphs, weights
from i2v_amd import lib as _lib
from tests import make_tnt_fixtures as mk
from tests.family_harness import bound, check_net, check_trajectory, rand as _rand, rel as _rel, run_twin as _run_twin
from tests.hostsim_util import hostsim_engine
from tests.tnt_reference import TntReference

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = json.load(open(os.path.join(ROOT, "tests", "golden", "timm_tnt_keys.json")))
FP32 = json.load(open(os.path.join(ROOT, "tests", "golden", "tnt_fp32_cpu_errors.json")))
NAMES = sorted(KEYS["names"])
SMALL = "tnt_s_patch16_224"
NET_FLOOR, FWD_FLOOR, BWD_FLOOR = 1e-5, 1e-6, 1e-5
FWD_PARTS = ("out", "gather")


def _f(v):
    return None if v is None else v.float().contiguous()


@pytest.fixture(scope="module")
def eng():
    e = hostsim_engine()
    _lib.bind(e.capi, _lib._TNT_PROTOS)
    return e


# ---- the specs ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_param_shapes_equal_the_key_fixture(name):
    want = {k: tuple(v) for k, v in KEYS["names"][name].items()}
    got = graphs.build_surrogate(name).param_shapes()
    assert got == want and list(got) == list(want)
    assert KEYS["checked_against"].startswith(("timm ", "unchecked"))


@pytest.mark.parametrize("name", NAMES)
def test_spec_sizes_and_hooks_of_every_name(name):
    dim, in_dim, blocks, heads, in_heads = mk.TABLE[name]
    spec = graphs.build_surrogate(name)
    assert isinstance(spec, graphs.TntSpec) and spec.arch == name and spec.video is False and spec.in_hw == (224, 224)
    assert (spec.dim, spec.in_dim, spec.blocks, spec.heads, spec.in_heads, spec.mlp_ratio, spec.ln_eps) == (dim, in_dim, blocks, heads, in_heads, 4, 1e-5)
    assert spec.grid == 14 and spec.tokens == 197 and spec.hook_dim == 197 * dim and spec.pixel_cols == 148
    assert [spec.hook_for(d) for d in (1, 2, 3, 4)] == [2, 5, 8, 11]
    with pytest.raises(KeyError):
        spec.hook_for(5)
    assert graphs.tnt_named(name) == spec and graphs.is_tnt_name(name)
    assert not any(f(name) for f in (graphs.is_swin_name, graphs.is_vit_name, graphs.is_beit_name, graphs.is_twins_name, graphs.is_pit_name,
                                     graphs.is_coat_name))
    assert not any(k.startswith(("head.", "norm.")) for k in spec.param_shapes())
    for hw in ((384, 384), (112, 112), (224, 192)):
        with pytest.raises(ValueError, match="224 x 224") as ei:
            graphs.build_surrogate(name, hw)
        assert all(n in str(ei.value) for n in NAMES)


def test_refusals_name_the_reason_and_list_the_served_names():
    for name in ("tnt_ti_patch16_224", "tnt_", "tnt_s_patch16_384", "tnt_b_patch8_224", "tnt"):
        assert graphs.is_tnt_name(name)
        with pytest.raises(ValueError, match="not a model of this table") as ei:
            graphs.build_surrogate(name)
        assert all(n in str(ei.value) for n in NAMES)
        with pytest.raises(ValueError):
            graphs.build_tiny(name)
    assert set(graphs.TNT_MODELS) == set(NAMES) and len(NAMES) == 2


def test_the_resolver_serves_the_names_and_leaves_build_as_it_was():
    assert graphs.build_surrogate(SMALL) == graphs.tnt_named(SMALL) and graphs.build_surrogate("resnet").arch == "resnet101"
    assert isinstance(graphs.build_surrogate("coat_lite_tiny"), graphs.CoatSpec)
    with pytest.raises(UnboundLocalError):
        graphs.build_surrogate("transformer")
    with pytest.raises(UnboundLocalError):
        graphs.build(SMALL)


def test_test_size_twins():
    t = graphs.build_tiny(SMALL, (64, 64))
    assert t == graphs.build_tiny("tnt_b_patch16_224", (64, 64)) == graphs.tnt_tiny_twin()
    assert (t.arch, t.grid, t.tokens, t.dim, t.in_dim, t.blocks, t.heads, t.in_heads) == ("tnt_test", 4, 17, 32, 24, 4, 2, 4)
    t48 = graphs.build_tiny(SMALL, (48, 48))
    assert (t48.arch, t48.grid, t48.tokens, t48.dim, t48.in_dim, t48.blocks, t48.heads, t48.in_heads) == ("tnt_test_48", 3, 10, 48, 40, 4, 4, 4)
    assert t.in_dim // t.in_heads == 6 and t48.in_dim // t48.in_heads == 10
    t224 = graphs.build_tiny("tnt_b_patch16_224", (224, 224))
    assert (t224.arch, t224.tokens, t224.blocks) == ("tnt_test_224", 197, 4)
    for tw in (t, t48, t224):
        assert tw.arch not in graphs.TNT_MODELS and [tw.hook_for(d) for d in (1, 2, 3, 4)] == [0, 1, 2, 3]
    for hw in ((72, 72), (128, 128), (64, 48)):
        with pytest.raises(ValueError):
            graphs.build_tiny(SMALL, hw)


# ---- checkpoints and packing -------------------------------------------------------------------------------------------------------
def test_checkpoint_loads_without_the_head(tmp_path, monkeypatch):
    spec = graphs.build_tiny(SMALL, (48, 48))
    monkeypatch.delenv("I2V_SYNTHETIC_WEIGHTS", raising=False)
    monkeypatch.setenv("I2V_WEIGHTS_DIR", str(tmp_path))
    with pytest.raises(weights.MissingWeights, match=spec.arch):
        weights.load_state_dict(spec)
    sd = {k: torch.full(shp, 0.5) for k, shp in spec.param_shapes().items()}
    sd.update({"norm.weight": torch.ones(48), "head.weight": torch.zeros(1000, 48)})
    torch.save(sd, tmp_path / (spec.arch + ".pth"))
    got = weights.load_state_dict(spec)
    assert list(got) == list(spec.param_shapes()) and "head.weight" not in got and "norm.weight" not in got
    torch.save(dict(sd, pixel_pos=torch.zeros(1, 40, 2, 2)), tmp_path / (spec.arch + ".pth"))
    with pytest.raises(ValueError, match="pixel_pos"):
        weights.load_state_dict(spec)


def test_synthetic_weights_let_the_new_arithmetic_show():
    spec = graphs.build_tiny(SMALL, (64, 64))
    sd = weights.load_state_dict(spec, seed=3)
    assert {k: tuple(v.shape) for k, v in sd.items()} == spec.param_shapes()
    assert 0.6 < float(sd["cls_token"].std()) < 1.4 and 0.35 < float(sd["pixel_pos"].std()) < 0.65 and 0.35 < float(sd["patch_pos"].std()) < 0.65
    assert abs(float(sd["blocks.0.norm_in.weight"].mean()) - 1.0) < 0.1
    assert 0.7 * 24 ** -0.5 < float(sd["blocks.1.attn_in.qk.weight"].std()) < 1.3 * 24 ** -0.5


def test_native_arrays_stack_qk_on_v_and_pad_the_pixel_filter():
    spec = graphs.build_tiny(SMALL, (48, 48))
    sd = weights.synthetic_state_dict(spec, 0)
    w = spec.native_arrays(sd, 2)
    d, D = 40, 48
    assert len(w) == 11 + 28 * 2 and all(t.dtype == torch.float32 and t.is_contiguous() for t in w)
    assert tuple(w[0].shape) == (d, 148) and torch.equal(w[0][:, :147], sd["pixel_embed.proj.weight"].reshape(d, 147)) and float(w[0][:, 147].abs().max()) == 0.0
    assert tuple(w[2].shape) == (16, d) and torch.equal(w[2][4 * 2 + 3], sd["pixel_pos"][0, :, 2, 3])
    assert tuple(w[5].shape) == (D, 16 * d) and tuple(w[9].shape) == (D,) and tuple(w[10].shape) == (10, D)
    b1 = w[11 + 28:]
    assert tuple(b1[2].shape) == (3 * d, d) and torch.equal(b1[2][:2 * d], sd["blocks.1.attn_in.qk.weight"]) and torch.equal(b1[2][2 * d:], sd["blocks.1.attn_in.v.weight"])
    assert tuple(b1[3].shape) == (3 * d,) and float(b1[3].abs().max()) == 0.0
    assert torch.equal(b1[12], sd["blocks.1.norm1_proj.weight"]) and torch.equal(b1[14], sd["blocks.1.proj.weight"])
    assert tuple(b1[18].shape) == (3 * D, D) and torch.equal(b1[18][2 * D:], sd["blocks.1.attn_out.v.weight"]) and float(b1[19].abs().max()) == 0.0
    assert torch.equal(b1[27], sd["blocks.1.mlp.fc2.bias"])


def test_new_native_symbols_are_exported_by_the_library_and_the_host_simulation():
    import __graft_entry__ as ge
    cd = C.CDLL(ge.LIB)
    assert all(hasattr(cd, n) for n in _lib.TNT_EXPORTS)
    assert {"i2v_tnt_attention_f32", "i2v_tnt_attention_bwd_f32", "i2v_tnt_pixel_gather_f32", "i2v_tnt_pixel_scatter_f32", "i2v_tnt_create",
            "i2v_tnt_destroy", "i2v_tnt_workspace_bytes", "i2v_tnt_forward", "i2v_tnt_backward", "i2v_tnt_hook_info", "i2v_tnt_read_hook"} <= set(_lib.TNT_EXPORTS)
    assert {"i2v_tnt.hip", "i2v_tnt.cpp"} <= set(ge.UNITS) and "-DI2V_HAVE_TNT" in ge.FLAGS
    assert {"i2v_tnt_host.h", "i2v_tnt_kernels.h"} <= set(ge.HEADERS)
    hs = C.CDLL(os.path.join(ROOT, "tests", "hostsim", "libi2v_hostsim.so"))
    assert all(hasattr(hs, n) for n in _lib.TNT_EXPORTS)
    assert "I2V_HAVE_TNT" not in open(os.path.join(ROOT, "tests", "hostsim", "build.sh")).read()
    header = open(os.path.join(ROOT, "include", "i2v_tnt.h")).read()
    assert all(n + "(" in header for n in _lib.TNT_EXPORTS)


def test_planned_bytes_are_counted_in_64_bits_and_hold_no_score_matrix():
    spec = graphs.build_surrogate(SMALL)
    got = spec.workspace_bytes([8], 128)
    assert 2 ** 31 < got < 2 ** 34                                          # past a signed 32-bit count, under 16 GiB
    more = spec.workspace_bytes([8, 2], 128) - got                          # a hook that is not the deepest: its gradient view and a copy of its stream
    assert more == 2 * 4 * 128 * 197 * 384
    assert spec.workspace_bytes([8], 256) > 1.9 * got


# ---- the kernel entries on the host simulation (csrc/i2v_tnt_host.h) ---------------------------------------------------------------
def run_attn(e, d, dev=lambda t: t):
    qkv = dev(_f(d["qkv"]))
    out = e.tnt_attention(qkv, d["heads"])
    dqkv = e.tnt_attention_bwd(qkv, dev(_f(d["dout"])), d["heads"])
    Cn = dqkv.shape[2] // 3
    return out.cpu(), dqkv[:, :, :Cn].cpu(), dqkv[:, :, Cn:2 * Cn].cpu(), dqkv[:, :, 2 * Cn:].cpu()


def check_attn(got, case):
    d = mk.attn_case(*case)
    want = mk.attn_reference(d)
    fp = FP32["attention"][mk.case_key(*case)]
    errs = {}
    for k, a, b in zip(mk.ATTN_PARTS, got, want):
        if case[1] == 1 and k in ("dq", "dk"):     # a single token: P = 1, so dq and dk are identically 0: held absolutely
            assert float(a.abs().max()) <= 1e-6
        else:
            errs[k] = _rel(a, b)
    print(f"tnt attention {case}: " + ", ".join(f"{k} {v:.3e} (fp32 CPU {fp[k]:.3e})" for k, v in errs.items()))
    for k, v in errs.items():
        assert v < bound(fp[k], FWD_FLOOR if k in FWD_PARTS else BWD_FLOOR), (k, v, fp[k])
    assert all(bool(torch.isfinite(t).all()) for t in got)
    if case[4] == "onehot":                # the one-hot row: out is the key's v exactly, and its dS cancels: dq is 0 to the bit
        Cn = d["qkv"].shape[2] // 3
        assert torch.equal(got[0][:, mk.ONEHOT_ROW], d["qkv"][:, mk.ONEHOT_KEY, 2 * Cn:].float())
        assert float(got[1][:, mk.ONEHOT_ROW].abs().max()) == 0.0


@pytest.mark.parametrize("case", mk.ATTN_CASES, ids=lambda c: mk.case_key(*c))
def test_attention_entries_on_the_host_simulation(eng, case):
    check_attn(run_attn(eng, mk.attn_case(*case)), case)


def test_the_fixture_brackets_a_workgroups_worth_of_sequences(eng):
    assert eng.tnt_attention_group(16, 4, 6) == mk.GROUP
    assert (mk.GROUP - 1, 16, 4, 6, "") in mk.ATTN_CASES and (mk.GROUP + 1, 16, 4, 6, "") in mk.ATTN_CASES
    assert eng.tnt_attention_group(16, 8, 16) >= 1 and eng.tnt_attention_group(1, 1, 4) == 256 and eng.tnt_attention_group(17, 4, 6) == 0


def run_pixels(e, d, dev=lambda t: t):
    """(rows, dx written, dx accumulated onto `base`, base); the padding columns of the rows' gradient are filled with noise: the
    scatter must not read them."""
    x = dev(_f(d["x"]))
    n, Cn, side, _ = x.shape
    rows = e.tnt_pixel_gather(x)
    dr = _f(_rand(rows.shape[0], rows.shape[1], seed=13))
    dr[:, :Cn * 49] = _f(d["drows"])
    dr = dev(dr)
    dx = e.tnt_pixel_scatter(dr, n, Cn, side)
    base = dev(_f(_rand(*x.shape, seed=12)))
    dxa = e.tnt_pixel_scatter(dr, n, Cn, side, into=base.clone())
    return rows.cpu(), dx.cpu(), dxa.cpu(), base.cpu()


def check_pixels(res, case):
    rows, dx, dxa, base = res
    d = mk.pixel_case(*case)
    wrows, wdx = mk.pixel_reference(d)
    K = case[1] * 49
    fp = FP32["pixels"][mk.case_key(*case)]
    assert rows.shape[1] % 4 == 0 and torch.equal(rows[:, :K], wrows.float()) and float(rows[:, K:].abs().sum()) == 0.0      # a copy; zero padding columns
    err = _rel(dx, wdx)
    print(f"tnt pixels {case}: scatter {err:.3e} (fp32 CPU {fp})")
    assert err < bound(fp["scatter"], BWD_FLOOR)
    r = d["drows"].float().double()                                         # the exact transpose: <gather x, r> = <x, scatter r>
    lhs, rhs = float((rows[:, :K].double() * r).sum()), float((d["x"].float().double() * dx.double()).sum())
    assert abs(lhs - rhs) <= bound(fp["scatter"], BWD_FLOOR) * float(rows[:, :K].double().norm() * r.norm())
    assert torch.equal(dxa, base + dx)                                      # accumulate: the sum formed first, then added once


@pytest.mark.parametrize("case", mk.PIXEL_CASES, ids=lambda c: mk.case_key(*c))
def test_pixel_entries_on_the_host_simulation(eng, case):
    check_pixels(run_pixels(eng, mk.pixel_case(*case)), case)


def entry_refusals(e, dev=lambda t: t):
    """T 17, dh 17, 9 heads, heads x dh = 6, a misaligned pointer, null, sizes of 0, a frame side of 24: each returns its text, launches
    nothing and leaves the outputs untouched."""
    capi = e.capi
    qkv, dout = dev(torch.zeros(2, 17, 3 * 72)), dev(torch.zeros(2, 17, 72))
    out, dqkv = dev(torch.full((2, 17, 72), 5.0)), dev(torch.full((2, 17, 3 * 72), 5.0))
    p = lambda t: C.c_void_p(t.data_ptr())      # noqa: E731
    off = lambda t: C.c_void_p(t.data_ptr() + 4)      # noqa: E731
    for (q, S, T, H, dh, o), why in (((p(qkv), 1, 17, 4, 6, p(out)), b"more than 16 tokens"), ((p(qkv), 1, 16, 4, 17, p(out)), b"wider than 16"),
                                     ((p(qkv), 1, 16, 9, 4, p(out)), b"more than 8 heads"), ((p(qkv), 1, 16, 1, 6, p(out)), b"multiple of 4"),
                                     ((off(qkv), 1, 16, 4, 6, p(out)), b"16-byte alignment"), ((p(qkv), 1, 16, 4, 6, off(out)), b"16-byte alignment"),
                                     ((None, 1, 16, 4, 6, p(out)), b"null argument"), ((p(qkv), 1, 16, 4, 6, None), b"null argument"),
                                     ((p(qkv), 0, 16, 4, 6, p(out)), b"must be positive"), ((p(qkv), 1, 0, 4, 6, p(out)), b"must be positive"),
                                     ((p(qkv), 2 ** 31 // (16 * 72) + 1, 16, 4, 6, p(out)), b"more than 2^31")):
        assert capi.i2v_tnt_attention_f32(q, S, T, H, dh, 1.0, o, None) != 0
        msg = capi.i2v_last_error()
        assert why in msg and b"hipErrorInvalidValue" in msg, msg
    bwd = capi.i2v_tnt_attention_bwd_f32
    for (q, g, S, T, H, dh, o), why in (((p(qkv), p(dout), 1, 17, 4, 6, p(dqkv)), b"more than 16 tokens"), ((p(qkv), p(dout), 1, 16, 4, 17, p(dqkv)), b"wider than 16"),
                                        ((p(qkv), p(dout), 1, 16, 9, 4, p(dqkv)), b"more than 8 heads"), ((p(qkv), p(dout), 1, 16, 1, 6, p(dqkv)), b"multiple of 4"),
                                        ((p(qkv), off(dout), 1, 16, 4, 6, p(dqkv)), b"16-byte alignment"), ((p(qkv), None, 1, 16, 4, 6, p(dqkv)), b"null argument"),
                                        ((p(qkv), p(dout), 1, 16, 4, 6, None), b"null argument")):
        assert bwd(q, g, S, T, H, dh, 1.0, o, None) != 0
        msg = capi.i2v_last_error()
        assert why in msg and b"hipErrorInvalidValue" in msg, msg
    y = dev(torch.full((64, 148), 5.0))
    assert capi.i2v_tnt_pixel_gather_f32(p(qkv), 1, 3, 24, p(y), None) != 0 and b"multiple of 16" in capi.i2v_last_error()
    assert capi.i2v_tnt_pixel_gather_f32(None, 1, 3, 16, p(y), None) != 0 and b"null argument" in capi.i2v_last_error()
    assert capi.i2v_tnt_pixel_gather_f32(off(qkv), 1, 3, 16, p(y), None) != 0 and b"16-byte alignment" in capi.i2v_last_error()
    assert capi.i2v_tnt_pixel_scatter_f32(p(qkv), 0, 3, 16, 0, p(y), None) != 0 and b"must be positive" in capi.i2v_last_error()
    if out.is_cuda:
        torch.cuda.synchronize()
    assert all(float((t.cpu() - 5.0).abs().max()) == 0.0 for t in (out, dqkv, y))
    o2 = e.tnt_attention(dev(torch.zeros(1, 16, 72)), 4)                   # the engine goes on afterwards
    assert float(o2.abs().max()) == 0.0


def test_entry_refusals_on_the_host_simulation(eng):
    entry_refusals(eng)


# ---- the planner (csrc/i2v_tnt.cpp) on the host simulation -------------------------------------------------------------------------
def twin_reference(label):
    name, side, _ = mk.TWINS[label]
    spec = graphs.build_tiny(name, (side, side))
    sd = weights.synthetic_state_dict(spec, 0)
    x = mk.twin_input(label)
    hooks = [spec.hook_for(d) for d in (1, 2, 3, 4)]
    ref = TntReference(spec, sd, hooks)
    rf = ref.forward(x)
    hg = [_rand(*f.shape, seed=30 + i) for i, f in enumerate(rf)]
    return (spec, sd, x, hooks, rf, hg, ref.backward(hg))


@pytest.fixture(scope="module")
def twin_refs():
    """The float64 reference of each twin case, computed once: label -> (spec, sd, x, hooks, features, hook gradients, input gradient)."""
    return {label: twin_reference(label) for label in mk.TWINS}


@pytest.mark.parametrize("label", sorted(mk.TWINS))
def test_twin_on_the_host_simulation_against_float64(eng, twin_refs, label):
    """Features at all four depths and the input gradient with all four hook gradients flowing (a hook below the deepest is added to the
    outer gradient behind the step's backward; the deepest block's inner stream gets gradient only through its proj); a net planned
    for 5 frames gives the same bits, frame 0 the bits of a 1-frame run; every single depth gives the same features and its own
    gradient."""
    spec, sd, x, hooks, rf, hg, want_gx = twin_refs[label]
    assert spec.arch == label
    feats, gx = _run_twin(eng, spec, sd, hooks, x, hg)
    check_net(label, feats, gx, rf, want_gx, FP32[label], NET_FLOOR)
    f1, g1 = _run_twin(eng, spec, sd, hooks, x[:1], [h[:1] for h in hg])
    assert all(torch.equal(a[:1], b) for a, b in zip(feats, f1)) and torch.equal(gx[:1], g1)
    feats2, gx2 = _run_twin(eng, spec, sd, hooks[::-1], x, hg[::-1], max_frames=5)
    assert all(torch.equal(a, b) for a, b in zip(feats, feats2[::-1])) and torch.equal(gx, gx2)
    for i in range(4):                                                      # one hook: the net is truncated there
        fa, ga = _run_twin(eng, spec, sd, [hooks[i]], x, [hg[i]])
        assert torch.equal(fa[0], feats[i])
        ref1 = TntReference(spec, sd, [hooks[i]])
        ref1.forward(x)
        assert _rel(ga, ref1.backward([hg[i]])) < bound(FP32[label]["grad"], NET_FLOOR)


@pytest.mark.parametrize("what", ["inner", "pixel_pos"])
def test_leaving_the_new_arithmetic_out_is_seen(twin_refs, what):
    """The inner transformer and the pixel position table carry arithmetic: the reference without either misses every hooked feature of
    tnt_test_48 by more than 100 x its bound."""
    spec, sd, x, hooks, rf, _, _ = twin_refs["tnt_test_48"]
    without = TntReference(spec, sd, hooks, skip=(what,)).forward(x)
    for i in range(4):
        assert _rel(without[i], rf[i]) > 100 * bound(FP32["tnt_test_48"]["hooks"][i], NET_FLOOR)


def test_planner_refusals_on_the_host_simulation(eng):
    spec = graphs.build_tiny(SMALL, (64, 64))
    sd = weights.synthetic_state_dict(spec, 0)
    with pytest.raises(_lib.I2VError, match="hooked twice"):
        eng.build_tnt_net(spec, sd, [1, 1], 2)
    with pytest.raises(_lib.I2VError, match="outside"):
        eng.build_tnt_net(spec, sd, [4], 2)
    net = eng.build_tnt_net(spec, sd, [1], 2)
    with pytest.raises(_lib.I2VError, match="planned for"):
        net.forward(torch.zeros(3, 3, 64, 64))
    with pytest.raises(_lib.I2VError):
        net.forward(torch.zeros(2, 3, 32, 32))
    net.close()
    h, one = C.c_void_p(), (C.c_int32 * 1)(0)
    create = lambda cfg, nw=39: eng.capi.i2v_tnt_create(0, C.byref(cfg), (C.c_void_p * nw)(), nw, one, 1, 1, C.byref(h))      # noqa: E731
    cfg = lambda img=64, dim=32, in_dim=24, heads=2, in_heads=4: _lib.TntConfig(img, 3, dim, in_dim, heads, in_heads, 4, 4, 1e-5)      # noqa: E731
    assert create(cfg(img=72)) != 0 and b"multiple of 16" in eng.capi.i2v_last_error()
    assert create(cfg(img=240)) != 0 and b"outer tokens" in eng.capi.i2v_last_error()
    assert create(cfg(in_dim=68)) != 0 and b"inner width 68" in eng.capi.i2v_last_error()
    assert create(cfg(in_dim=24, in_heads=12)) != 0 and b"inner width 24 under 12 heads" in eng.capi.i2v_last_error()
    assert create(cfg(dim=36, heads=6)) != 0 and b"outer width 36" in eng.capi.i2v_last_error()
    assert create(cfg(), 38) != 0 and b"38 weight arrays given, 39 expected" in eng.capi.i2v_last_error()


def test_attack_classes_and_the_command_line_take_the_names(tmp_path, monkeypatch):
    attacks.ImageGuidedFMDirection_Adam([SMALL, "resnet50", "coat_lite_tiny"], depth=3, step_size=0.005, weight_seed=0)
    attacks.ImageGuidedStd_Adam(["tnt_b_patch16_224"], depth=1, step_size=0.005, weight_seed=0)
    attacks.AENS_I2V_MF([SMALL, "resnet50"], depths={SMALL: [2, 4], "resnet50": [2, 3]}, step_size=0.005, weight_seed=0)
    with pytest.raises(KeyError):
        attacks.ImageGuidedFMDirection_Adam([SMALL], depth=5, step_size=0.005, weight_seed=0)
    with pytest.raises(ValueError, match="not a model of this table") as ei:
        attacks.ImageGuidedFMDirection_Adam(["tnt_ti_patch16_224"], depth=2, step_size=0.005, weight_seed=0)
    assert all(n in str(ei.value) for n in NAMES)
    import image_main
    monkeypatch.setattr(image_main, "OPT_PATH", str(tmp_path))
    base = ["--attack_method", "ImageGuidedFMDirection_Adam", "--step", "2"]
    for name in NAMES:
        for depth in ("1", "2", "3", "4"):
            a = image_main.arg_parse(base + ["--direction_image_model", name, "--depth", depth])
            assert image_main.build_attack(a).model_names == [name]
    for bad in (["--direction_image_model", "tnt_s_patch16_384"], ["--direction_image_model", SMALL, "--depth", "5"],
                ["--direction_image_model", SMALL, "--hw", "112"]):
        with pytest.raises(SystemExit):
            image_main.arg_parse(base + bad)


def test_i2v_trajectory_on_the_twin_matches_the_float64_trajectory(eng):
    """10 steps of the I2V attack on tnt_test at depth 3, the costs against the float64 trajectory of `restate.run_attack` within
    max(1e-5, 4 x the float32 reference's own relative cost error on the same clip) (tests/golden/tnt_fp32_cpu_errors.json,
    "trajectory")."""
    label, depth = "tnt_test", mk.TRAJECTORY_DEPTH
    name, side, _ = mk.TWINS[label]
    clip = mk.TRAJECTORY_CLIP
    rtol = bound(FP32["trajectory"][label][str(depth)], NET_FLOOR)
    vid = mk.video(*clip)
    atk = attacks.ImageGuidedFMDirection_Adam([name], depth=depth, step_size=0.005, steps=10, engine=eng, graph_builder=graphs.build_tiny, weight_seed=0)
    adv = atk(vid, torch.zeros(clip[0], dtype=torch.long), ["a", "b"])
    spec = graphs.build_tiny(name, (side, side))
    assert spec.arch == label
    check_trajectory(atk, adv, TntReference(spec, weights.synthetic_state_dict(spec, 0), [spec.hook_for(depth)], dtype=torch.float64), vid, rtol=rtol)
