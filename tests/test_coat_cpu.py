"""CPU: timm's CoaT-Lite family as image surrogates on the transformer stack -- for the three served names the
spec, the hooks and the key / shape contract against tests/golden/timm_coat_keys.json; the refusals (the parallel models with their
reason); checkpoint loading with the block-level duplicates of the shared cpe / crpe verified; the packing against the reference's conv2d
arithmetic, and that leaving cpe, one crpe window or the class tokens out is seen; the kernel entries on the host simulation, which runs
them as scalar code (csrc/i2v_coat_host.h); and the planner itself (csrc/i2v_coat.cpp) on the host simulation: all three twins against
float64, and a 4-step I2V attack against the oracle.

The bound is relative L2 against float64: the larger of the floor for that kind of case (entries 1e-6 forward, 1e-5 backward; nets 1e-5)
and 4 x the error of the float32 CPU run of the same reference on the same inputs, read from tests/golden/coat_fp32_cpu_errors.json
(tests/make_coat_fixtures.py).  A case without a recorded error fails (KeyError)."""
import ctypes as C
import json
import os

import pytest
import torch

from i2v_amd import attacks, graphs, weights
from i2v_amd import lib as _lib
from tests import make_coat_fixtures as mk
from tests.coat_reference import CoatReference
from tests.family_harness import bound, check_net, check_trajectory, rand as _rand, rel as _rel, run_twin as _run_twin
from tests.hostsim_util import hostsim_engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = json.load(open(os.path.join(ROOT, "tests", "golden", "timm_coat_keys.json")))
FP32 = json.load(open(os.path.join(ROOT, "tests", "golden", "coat_fp32_cpu_errors.json")))
NAMES = sorted(KEYS["names"])
TINY = "coat_lite_tiny"
NET_FLOOR, FWD_FLOOR, BWD_FLOOR = 1e-5, 1e-6, 1e-5
FWD_PARTS = ("out", "gram", "fwd", "gather")


def _f(v):
    return None if v is None else v.float().contiguous()


@pytest.fixture(scope="module")
def eng():
    e = hostsim_engine()
    _lib.bind(e.capi, _lib._COAT_PROTOS)
    return e


# ---- the specs ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_param_shapes_equal_the_key_fixture(name):
    want = {k: tuple(v) for k, v in KEYS["names"][name].items()}
    assert graphs.build_surrogate(name).param_shapes() == want
    assert KEYS["checked_against"].startswith(("timm ", "unchecked"))


@pytest.mark.parametrize("name", NAMES)
def test_spec_sizes_and_hooks_of_every_name(name):
    widths, depths, ratios = mk.TABLE[name]
    spec = graphs.build_surrogate(name)
    assert isinstance(spec, graphs.CoatSpec) and spec.arch == name and spec.video is False and spec.in_hw == (224, 224)
    assert (tuple(spec.widths), tuple(spec.depths), tuple(spec.mlp_ratios), spec.heads, tuple(spec.windows), spec.ln_eps) == \
        (widths, depths, ratios, 8, (2, 3, 3), 1e-6)
    assert spec.grids == (56, 28, 14, 7) and [spec.tokens(k) for k in range(4)] == [3137, 785, 197, 50]
    assert [spec.hook_for(d) for d in (1, 2, 3, 4)] == [0, 1, 2, 3]
    with pytest.raises(KeyError):
        spec.hook_for(5)
    assert graphs.coat_named(name) == spec and graphs.is_coat_name(name)
    assert not any(f(name) for f in (graphs.is_swin_name, graphs.is_vit_name, graphs.is_beit_name, graphs.is_twins_name, graphs.is_pit_name))
    assert not any(k.startswith(("head.", "norm", "aggregate.")) for k in spec.param_shapes())
    for hw in ((384, 384), (112, 112), (224, 192)):
        with pytest.raises(ValueError, match="224 x 224") as ei:
            graphs.build_surrogate(name, hw)
        assert all(n in str(ei.value) for n in NAMES)


def test_hooked_feature_sizes_and_head_widths():
    spec = graphs.build_surrogate(TINY)
    assert [spec.hook_shape(spec.hook_for(d)) for d in (1, 2, 3, 4)] == [(3137, 64), (785, 128), (197, 256), (50, 320)]
    assert spec.head_widths == (8, 16, 32, 40) and graphs.build_surrogate("coat_lite_small").head_widths == (8, 16, 40, 64)
    assert spec.window_channels(3) == (80, 120, 120)


def test_refusals_name_the_reason_and_list_the_served_names():
    for name in ("coat_tiny", "coat_mini"):
        with pytest.raises(ValueError, match="parallel blocks need bilinear cross-scale resampling") as ei:
            graphs.build_surrogate(name)
        assert all(n in str(ei.value) for n in NAMES)
    for name in ("coat_lite_base", "coat_", "coat_small", "coat_lite_tiny_384"):
        assert graphs.is_coat_name(name)
        with pytest.raises(ValueError, match="not a model of this table") as ei:
            graphs.build_surrogate(name)
        assert all(n in str(ei.value) for n in NAMES)
        with pytest.raises(ValueError):
            graphs.build_tiny(name)
    assert set(graphs.COAT_MODELS) == set(NAMES) and len(NAMES) == 3


def test_the_resolver_serves_the_names_and_leaves_build_as_it_was():
    assert graphs.build_surrogate(TINY) == graphs.coat_named(TINY) and graphs.build_surrogate("resnet").arch == "resnet101"
    assert isinstance(graphs.build_surrogate("pit_s_224"), graphs.PitSpec)
    with pytest.raises(UnboundLocalError):
        graphs.build_surrogate("transformer")
    with pytest.raises(UnboundLocalError):
        graphs.build(TINY)


def test_test_size_twins():
    t = graphs.build_tiny(TINY, (64, 64))
    assert t == graphs.build_tiny("coat_lite_small", (64, 64)) == graphs.coat_tiny_twin()
    assert (t.arch, t.grids, t.heads, t.windows, t.widths, t.head_widths, t.depths) == \
        ("coat_test", (16, 8, 4, 2), 8, (2, 3, 3), (32, 32, 64, 96), (4, 4, 8, 12), (2, 1, 2, 1))
    t96 = graphs.build_tiny(TINY, (96, 96))
    assert (t96.arch, t96.grids, t96.heads, t96.windows, t96.widths, t96.head_widths, t96.depths) == \
        ("coat_test_96", (24, 12, 6, 3), 4, (1, 2, 1), (48, 48, 80, 160), (12, 12, 20, 40), (1, 2, 1, 2))
    t224 = graphs.build_tiny("coat_lite_mini", (224, 224))
    assert (t224.arch, t224.tokens(0), t224.widths, t224.depths) == ("coat_test_224", 3137, (32, 64, 64, 96), (1, 1, 1, 1))
    assert not any(tw.arch in graphs.COAT_MODELS for tw in (t, t96, t224))
    for hw in ((72, 72), (128, 128), (64, 96)):
        with pytest.raises(ValueError):
            graphs.build_tiny(TINY, hw)


# ---- checkpoints and packing -------------------------------------------------------------------------------------------------------
def test_checkpoint_loads_and_a_differing_block_level_duplicate_is_refused(tmp_path, monkeypatch):
    spec = graphs.build_surrogate(TINY)
    monkeypatch.delenv("I2V_SYNTHETIC_WEIGHTS", raising=False)
    monkeypatch.setenv("I2V_WEIGHTS_DIR", str(tmp_path))
    with pytest.raises(weights.MissingWeights, match=TINY):
        weights.load_state_dict(spec)
    path = tmp_path / (TINY + ".pth")
    sd = {k: torch.full(shp, 0.5) for k, shp in spec.param_shapes().items()}
    sd.update({"norm4.weight": torch.ones(320), "head.weight": torch.zeros(1000, 320)})
    torch.save(sd, path)                                                    # without the duplicates: accepted
    got = weights.load_state_dict(spec)
    assert list(got) == list(spec.param_shapes()) and "head.weight" not in got and "norm4.weight" not in got
    dups = spec.shared_duplicates()
    assert len(dups) == 8 * 8 and dups["serial_blocks3.1.factoratt_crpe.crpe.conv_list.2.weight"] == "crpe3.conv_list.2.weight"
    assert dups["serial_blocks1.0.cpe.proj.bias"] == "cpe1.proj.bias"
    full = dict(sd, **{d: sd[k].clone() for d, k in dups.items()})
    torch.save(full, path)                                                  # with equal duplicates: accepted, and not returned
    assert list(weights.load_state_dict(spec)) == list(spec.param_shapes())
    for bad in ("serial_blocks2.1.cpe.proj.weight", "serial_blocks4.0.factoratt_crpe.crpe.conv_list.1.bias"):
        torch.save(dict(full, **{bad: full[bad] + 1.0}), path)
        with pytest.raises(ValueError, match=bad.replace(".", r"\.")):
            weights.load_state_dict(spec)
    torch.save(dict(sd, cls_token2=torch.zeros(1, 1, 64)), path)
    with pytest.raises(ValueError, match="cls_token2"):
        weights.load_state_dict(spec)


def test_synthetic_weights_let_the_new_arithmetic_show():
    spec = graphs.build_tiny(TINY, (96, 96))
    sd = weights.load_state_dict(spec, seed=3)
    assert {k: tuple(v.shape) for k, v in sd.items()} == spec.param_shapes()
    assert all(0.6 < float(sd[f"cls_token{s}"].std()) < 1.4 for s in (1, 2, 3, 4))
    for s in (1, 4):
        assert 0.8 / 3 < float(sd[f"cpe{s}.proj.weight"].std()) < 1.2 / 3
        for i, K in enumerate((3, 5, 7)):
            assert 0.75 / K < float(sd[f"crpe{s}.conv_list.{i}.weight"].std()) < 1.25 / K


def test_native_arrays_pack_the_filters_tap_major_and_the_patches_in_cell_order():
    spec = graphs.build_tiny(TINY, (96, 96))
    sd = weights.synthetic_state_dict(spec, 0)
    w = spec.native_arrays(sd, 2)
    assert len(w) == 12 + 12 * 1 + 12 + 12 * 2 and all(t.dtype == torch.float32 and t.is_contiguous() for t in w)
    assert tuple(w[0].shape) == (48, 48) and torch.equal(w[0], sd["patch_embed1.proj.weight"].reshape(48, 48))
    assert tuple(w[4].shape) == (48,) and tuple(w[5].shape) == (577, 48) and float(w[5].abs().max()) == 0.0
    assert tuple(w[6].shape) == (9, 48) and torch.equal(w[6][5], sd["cpe1.proj.weight"][:, 0, 1, 2])
    assert [tuple(t.shape) for t in w[8:12]] == [(9, 12), (25, 24), (49, 12), (48,)]
    assert torch.equal(w[9][2 * 5 + 3], sd["crpe1.conv_list.1.weight"][:, 0, 2, 3])
    assert torch.equal(w[11][12:36], sd["crpe1.conv_list.1.bias"])
    pe2 = w[24]
    assert tuple(pe2.shape) == (48, 4 * 48) and torch.equal(pe2[:, (1 * 2 + 0) * 48 + 7], sd["patch_embed2.proj.weight"][:, 7, 1, 0])


def test_new_native_symbols_are_exported_by_the_library_and_the_host_simulation():
    import __graft_entry__ as ge
    cd = C.CDLL(ge.LIB)
    assert all(hasattr(cd, n) for n in _lib.COAT_EXPORTS)
    assert {"i2v_coat_factor_attention_f32", "i2v_coat_factor_attention_bwd_f32", "i2v_coat_dwmix_f32", "i2v_coat_dwmix_bwd_f32",
            "i2v_coat_cell_gather_f32", "i2v_coat_cell_scatter_f32", "i2v_coat_create"} <= set(_lib.COAT_EXPORTS)
    assert {"i2v_coat.hip", "i2v_coat.cpp"} <= set(ge.UNITS) and "-DI2V_HAVE_COAT" in ge.FLAGS
    assert {"i2v_coat_host.h", "i2v_coat_kernels.h"} <= set(ge.HEADERS)
    hs = C.CDLL(os.path.join(ROOT, "tests", "hostsim", "libi2v_hostsim.so"))
    assert all(hasattr(hs, n) for n in _lib.COAT_EXPORTS)
    assert "I2V_HAVE_COAT" not in open(os.path.join(ROOT, "tests", "hostsim", "build.sh")).read()
    header = open(os.path.join(ROOT, "include", "i2v_coat.h")).read()
    assert all(n + "(" in header for n in _lib.COAT_EXPORTS)


def test_planned_bytes_are_counted_in_64_bits_and_hold_no_token_by_token_matrix():
    spec = graphs.build_surrogate(TINY)
    got = spec.workspace_bytes([2], 128)
    assert 2 ** 31 < got < 2 ** 37                                          # past a signed 32-bit count
    F, T0, D0 = 128, 3137, 64
    assert got < 4 * 80 * F * T0 * D0                                       # a few dozen streams of the widest stage ...
    assert 4 * F * 8 * T0 * T0 > 5 * got                                    # ... where ONE block's token-by-token scores would be five times that


# ---- the kernel entries on the host simulation (csrc/i2v_coat_host.h) --------------------------------------------------------------
def run_attn(e, d, dev=lambda t: t):
    qkv, E = dev(_f(d["qkv"])), dev(_f(d["E"]))
    out, gram, kstat = e.coat_attention(qkv, E, d["heads"])
    dqkv, dE = e.coat_attention_bwd(qkv, E, gram, kstat, dev(_f(d["dout"])), d["heads"])
    Cn = dqkv.shape[2] // 3
    return out.cpu(), gram.cpu(), dqkv[:, :, :Cn].cpu(), dqkv[:, :, Cn:2 * Cn].cpu(), dqkv[:, :, 2 * Cn:].cpu(), dE.cpu(), kstat.cpu()


def check_attn(got, case):
    d = mk.attn_case(*case)
    want = mk.attn_reference(d)
    fp = FP32["attention"][mk.case_key(*case)]
    errs = {}
    for k, a, b in zip(mk.ATTN_PARTS, got, want):
        if case[1] == 1 and k == "dk":     # a single token: Ks = 1, so dk is identically 0: held absolutely
            assert float(a.abs().max()) <= 1e-6
        else:
            errs[k] = _rel(a, b)
    Cn = d["qkv"].shape[2] // 3            # the saved statistics: the column maximum exactly, the log of the column sum
    k = d["qkv"][:, :, Cn:2 * Cn].float().double().reshape(case[0], case[1], case[2], case[3]).transpose(1, 2)
    assert torch.equal(got[6][:, :, 0].double(), k.max(dim=2).values)
    assert float((got[6][:, :, 1].double() - (torch.logsumexp(k, dim=2) - k.max(dim=2).values)).abs().max()) < 1e-5
    print(f"coat attention {case}: " + ", ".join(f"{k} {v:.3e} (fp32 CPU {fp[k]:.3e})" for k, v in errs.items()))
    for k, v in errs.items():
        assert v < bound(fp[k], FWD_FLOOR if k in FWD_PARTS else BWD_FLOOR), (k, v, fp[k])


@pytest.mark.parametrize("case", mk.ATTN_CASES, ids=lambda c: mk.case_key(*c))
def test_attention_entries_on_the_host_simulation(eng, case):
    check_attn(run_attn(eng, mk.attn_case(*case)), case)


def _packed(d):
    """The filters tap-major and the bias as the launch takes them; a window without channels: None."""
    return tuple(None if d[f"w{K}"].shape[0] == 0 else _f(d[f"w{K}"].reshape(-1, K * K).t()) for K in (3, 5, 7)), _f(d["b"])


def run_dw(e, d, dev=lambda t: t):
    """(y, dx written, dx accumulated onto `base`, base): the backward accumulates into the v columns of a qkv-shaped array in the
    "qkv" form, into an array of its own otherwise."""
    Cn, g, pre, form = d["C"], d["g"], d["prefix"], d["form"]
    filt, b = _packed(d)
    filt, b = tuple(None if w is None else dev(w) for w in filt), dev(b)
    col, res = (2 * Cn if form == "qkv" else 0), form == "cpe"
    x, dy = dev(_f(d["x"])), dev(_f(d["dy"]))
    y = e.coat_dwmix(x, filt, b, g, pre, res, col, Cn)
    dx = e.coat_dwmix(dy, filt, None, g, pre, res, bwd=True)
    base = dev(_f(_rand(*d["x"].shape, seed=11)))
    dxa = e.coat_dwmix(dy, filt, None, g, pre, res, bwd=True, into=base.clone(), into_col=col)
    return y.cpu(), dx.cpu(), dxa.cpu(), base.cpu()


def check_dw(res, case):
    y, dx, dxa, base = res
    d = mk.dw_case(*case)
    Cn, pre, form = d["C"], d["prefix"], d["form"]
    wy, wdx = mk.dw_reference(d)
    fp = FP32["dwmix"][mk.case_key(*case)]
    print(f"coat dwmix {case}: fwd {_rel(y, wy):.3e} bwd {_rel(dx, wdx):.3e} (fp32 CPU {fp})")
    assert _rel(y, wy) < bound(fp["fwd"], FWD_FLOOR) and _rel(dx, wdx) < bound(fp["bwd"], BWD_FLOOR)
    if pre and form != "cpe":              # E's class row is 0 and carries no gradient; cpe passes the class row through
        assert float(y[:, :pre].abs().max()) == 0.0 and float(dx[:, :pre].abs().max()) == 0.0
    elif pre:
        assert torch.equal(y[:, :pre], d["x"][:, :pre].float()) and torch.equal(dx[:, :pre], d["dy"][:, :pre].float())
    col = 2 * Cn if form == "qkv" else 0
    assert torch.equal(dxa[:, :, col:col + Cn], base[:, :, col:col + Cn] + dx)       # accumulate: the sum formed first, then added once
    assert torch.equal(dxa[:, :, :col], base[:, :, :col])                             # q and k of a qkv gradient are not touched


@pytest.mark.parametrize("case", mk.DW_CASES, ids=lambda c: mk.case_key(*c))
def test_dwmix_entries_on_the_host_simulation(eng, case):
    check_dw(run_dw(eng, mk.dw_case(*case)), case)


def run_cells(e, d, dev=lambda t: t):
    x, g, s = dev(_f(d["x"])), d["g"], d["s"]
    rows = e.coat_cell_gather(x, g, s)
    dr = dev(_f(d["drows"]))
    dx = e.coat_cell_scatter(dr, x.shape[0], g, s)
    base = dev(_f(_rand(*x.shape, seed=12)))
    dxa = e.coat_cell_scatter(dr, x.shape[0], g, s, into=base.clone())
    return rows.cpu(), dx.cpu(), dxa.cpu(), base.cpu()


def check_cells(res, case):
    rows, dx, dxa, base = res
    wrows, wdx = mk.cell_reference(mk.cell_case(*case))
    assert torch.equal(rows, wrows.float()) and torch.equal(dx, wdx.float())          # copies, against float64 autograd; the class row 0
    assert float(dx[:, 0].abs().max()) == 0.0
    assert torch.equal(dxa[:, 1:], base[:, 1:] + dx[:, 1:]) and torch.equal(dxa[:, :1], base[:, :1])


@pytest.mark.parametrize("case", mk.CELL_CASES, ids=lambda c: mk.case_key(*c))
def test_cell_entries_on_the_host_simulation(eng, case):
    check_cells(run_cells(eng, mk.cell_case(*case)), case)


def entry_refusals(e, dev=lambda t: t):
    """dh 6, dh 68, null and misaligned arrays, frames 0, a group width of 6, a plane side of 0, cells that do not tile: each returns its
    text, launches nothing and leaves the outputs untouched."""
    capi = e.capi
    qkv, E = dev(torch.zeros(1, 8, 3 * 72)), dev(torch.zeros(1, 8, 72))
    out, gram, kstat = dev(torch.full((1, 8, 72), 5.0)), dev(torch.full((1, 9, 8, 8), 5.0)), dev(torch.full((1, 9, 2, 8), 5.0))
    p = lambda t: C.c_void_p(t.data_ptr())      # noqa: E731
    off = lambda t: C.c_void_p(t.data_ptr() + 4)      # noqa: E731
    for args, why in (((p(qkv), p(E), 1, 8, 1, 6, 1.0, p(gram), p(kstat), p(out)), b"multiple of 4"),
                      ((p(qkv), p(E), 1, 8, 1, 68, 1.0, p(gram), p(kstat), p(out)), b"wider than 64"),
                      ((None, p(E), 1, 8, 1, 8, 1.0, p(gram), p(kstat), p(out)), b"null argument"),
                      ((p(qkv), p(E), 1, 8, 1, 8, 1.0, p(gram), None, p(out)), b"null argument"),
                      ((off(qkv), p(E), 1, 7, 1, 8, 1.0, p(gram), p(kstat), p(out)), b"16-byte alignment"),
                      ((p(qkv), p(E), 1, 8, 1, 8, 1.0, p(gram), p(kstat), off(out)), b"16-byte alignment"),
                      ((p(qkv), p(E), 0, 8, 1, 8, 1.0, p(gram), p(kstat), p(out)), b"must be positive"),
                      ((p(qkv), p(E), 1, 0, 1, 8, 1.0, p(gram), p(kstat), p(out)), b"must be positive")):
        assert capi.i2v_coat_factor_attention_f32(*args, None) != 0
        msg = capi.i2v_last_error()
        assert why in msg and b"hipErrorInvalidValue" in msg, msg
    dq, dE = dev(torch.full((1, 8, 24), 5.0)), dev(torch.full((1, 8, 8), 5.0))
    bwd = capi.i2v_coat_factor_attention_bwd_f32
    assert bwd(p(qkv), p(E), p(gram), p(kstat), None, 1, 8, 1, 8, 1.0, p(gram), p(dq), p(dE), None) != 0
    assert b"null argument" in capi.i2v_last_error()
    assert bwd(p(qkv), p(E), p(gram), p(kstat), p(E), 1, 8, 1, 6, 1.0, p(gram), p(dq), p(dE), None) != 0
    assert b"multiple of 4" in capi.i2v_last_error()
    y = dev(torch.full((1, 5, 24), 5.0))
    dw = capi.i2v_coat_dwmix_f32
    for args, why in (((p(qkv), 24, p(E), p(E), p(E), None, 1, 2, 24, 6, 6, 1, 0, p(y), 24), b"group width must be a multiple of 4"),
                      ((p(qkv), 24, p(E), p(E), p(E), None, 1, 2, 24, 8, 20, 1, 0, p(y), 24), b"do not partition"),
                      ((p(qkv), 24, p(E), None, p(E), None, 1, 2, 24, 8, 8, 1, 0, p(y), 24), b"null argument"),
                      ((p(qkv), 24, p(E), p(E), p(E), None, 1, 0, 24, 8, 8, 1, 0, p(y), 24), b"must be positive"),
                      ((p(qkv), 24, p(E), p(E), p(E), None, 1, 70000, 24, 8, 8, 1, 0, p(y), 24), b"over 65535"),
                      ((p(qkv), 24, p(E), p(E), p(E), None, 1, 40000, 24, 8, 8, 1, 0, p(y), 24), b"more than 2^31"),
                      ((p(qkv), 20, p(E), p(E), p(E), None, 1, 2, 24, 8, 8, 1, 0, p(y), 24), b"row stride"),
                      ((off(qkv), 24, p(E), p(E), p(E), None, 1, 2, 24, 8, 8, 1, 0, p(y), 24), b"16-byte alignment")):
        assert dw(*args, None) != 0
        msg = capi.i2v_last_error()
        assert why in msg and b"hipErrorInvalidValue" in msg, msg
    assert capi.i2v_coat_dwmix_bwd_f32(p(qkv), 24, p(E), p(E), p(E), 1, 2, 24, 6, 6, 1, 0, 0, p(y), 24, None) != 0
    assert b"multiple of 4" in capi.i2v_last_error()
    assert capi.i2v_coat_cell_gather_f32(p(qkv), 1, 3, 8, 2, 1, p(y), None) != 0 and b"do not tile" in capi.i2v_last_error()
    assert capi.i2v_coat_cell_scatter_f32(p(qkv), 1, 2, 6, 2, 1, 0, p(y), None) != 0 and b"multiple of 4" in capi.i2v_last_error()
    if out.is_cuda:
        torch.cuda.synchronize()
    assert all(float((t.cpu() - 5.0).abs().max()) == 0.0 for t in (out, gram, kstat, dq, dE, y))
    o2, _, _ = e.coat_attention(dev(torch.zeros(1, 8, 24)), dev(torch.zeros(1, 8, 8)), 1)      # the engine goes on afterwards
    assert float(o2.abs().max()) == 0.0


def test_entry_refusals_on_the_host_simulation(eng):
    entry_refusals(eng)


# ---- the planner (csrc/i2v_coat.cpp) on the host simulation ------------------------------------------------------------------------
def twin_reference(label):
    name, side, _ = mk.TWINS[label]
    spec = graphs.build_tiny(name, (side, side))
    sd = weights.synthetic_state_dict(spec, 0)
    x = mk.twin_input(label)
    hooks = [spec.hook_for(d) for d in (1, 2, 3, 4)]
    ref = CoatReference(spec, sd, hooks)
    rf = ref.forward(x)
    hg = [_rand(*f.shape, seed=30 + i) for i, f in enumerate(rf)]
    return (spec, sd, x, hooks, rf, hg, ref.backward(hg))


@pytest.fixture(scope="module")
def twin_refs():
    """The float64 reference of each twin case, computed once: label -> (spec, sd, x, hooks, features, hook gradients, input gradient)."""
    return {label: twin_reference(label) for label in mk.TWINS}


@pytest.mark.parametrize("label", sorted(mk.TWINS))
def test_twin_on_the_host_simulation_against_float64(eng, twin_refs, label):
    """Features at all four depths and the input gradient with all four hook gradients flowing (a hook behind a lower stage is added
    where the next stage's patch-embedding backward writes); a net planned for 5 frames gives the same bits, frame 0 the bits of a
    1-frame run; every single depth gives the same features and its own gradient."""
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
        ref1 = CoatReference(spec, sd, [hooks[i]])
        ref1.forward(x)
        assert _rel(ga, ref1.backward([hg[i]])) < bound(FP32[label]["grad"], NET_FLOOR)


@pytest.mark.parametrize("what", ["cpe", "crpe0", "crpe1", "crpe2", "cls"])
def test_leaving_the_new_arithmetic_out_is_seen(eng, twin_refs, what):
    """cpe, each crpe window's filter and the class tokens carry arithmetic: the reference without the term misses every hooked
    feature of coat_test_96 by more than 100 x its bound, and the library's result through the packing follows the state dict."""
    spec, sd, x, hooks, rf, hg, _ = twin_refs["coat_test_96"]
    feats, _ = _run_twin(eng, spec, sd, hooks, x, hg)
    without = CoatReference(spec, sd, hooks, skip=(what,)).forward(x)
    blind = dict(sd)                                                        # ... and through the packing: the same state dict with the term zeroed
    for s in (1, 2, 3, 4):
        if what == "cpe":
            blind[f"cpe{s}.proj.weight"], blind[f"cpe{s}.proj.bias"] = torch.zeros_like(sd[f"cpe{s}.proj.weight"]), torch.zeros_like(sd[f"cpe{s}.proj.bias"])
        elif what == "cls":
            blind[f"cls_token{s}"] = torch.zeros_like(sd[f"cls_token{s}"])
        else:
            k = f"crpe{s}.conv_list.{what[-1]}.weight"
            blind[k] = torch.zeros_like(sd[k])
    fb, _ = _run_twin(eng, spec, blind, hooks, x, hg)
    for i in range(4):
        cpu = FP32["coat_test_96"]["hooks"][i]
        assert _rel(without[i], rf[i]) > 100 * bound(cpu, NET_FLOOR) and _rel(feats[i], without[i]) > 100 * bound(cpu, NET_FLOOR)
        assert _rel(fb[i], feats[i]) > 100 * bound(cpu, NET_FLOOR) and _rel(fb[i], without[i]) < bound(cpu, NET_FLOOR)


def test_planner_refusals_on_the_host_simulation(eng):
    spec = graphs.build_tiny(TINY, (64, 64))
    sd = weights.synthetic_state_dict(spec, 0)
    with pytest.raises(_lib.I2VError, match="hooked twice"):
        eng.build_coat_net(spec, sd, [1, 1], 2)
    with pytest.raises(_lib.I2VError, match="outside"):
        eng.build_coat_net(spec, sd, [4], 2)
    net = eng.build_coat_net(spec, sd, [1], 2)
    with pytest.raises(_lib.I2VError, match="planned for"):
        net.forward(torch.zeros(3, 3, 64, 64))
    with pytest.raises(_lib.I2VError):
        net.forward(torch.zeros(2, 3, 32, 32))
    net.close()
    h, one = C.c_void_p(), (C.c_int32 * 1)(0)
    four = lambda *v: (C.c_int32 * 4)(*v)      # noqa: E731
    create = lambda cfg, nw=36: eng.capi.i2v_coat_create(0, C.byref(cfg), (C.c_void_p * nw)(), nw, one, 1, 1, C.byref(h))      # noqa: E731
    cfg = lambda img=64, dims=(32, 32, 64, 96), heads=8, win=(2, 3, 3): _lib.CoatConfig(      # noqa: E731
        img, 3, four(*dims), heads, four(2, 1, 2, 1), four(8, 8, 4, 4), *win, 1e-6)
    assert create(cfg(img=72)) != 0 and b"multiple of 32" in eng.capi.i2v_last_error()
    assert create(cfg(dims=(544, 32, 64, 96))) != 0 and b"heads of width 68" in eng.capi.i2v_last_error()
    assert create(cfg(dims=(48, 32, 64, 96))) != 0 and b"stage 0 has width 48" in eng.capi.i2v_last_error()
    assert create(cfg(win=(2, 3, 2))) != 0 and b"sum to the 8 heads" in eng.capi.i2v_last_error()
    assert create(cfg(win=(0, 5, 3))) != 0 and b"sum to the 8 heads" in eng.capi.i2v_last_error()
    assert create(cfg(), 35) != 0 and b"35 weight arrays given, 36 expected" in eng.capi.i2v_last_error()


def test_attack_classes_and_the_command_line_take_the_names(tmp_path, monkeypatch):
    attacks.ImageGuidedFMDirection_Adam([TINY, "resnet50", "pit_s_224"], depth=3, step_size=0.005, weight_seed=0)
    attacks.ImageGuidedStd_Adam(["coat_lite_small"], depth=1, step_size=0.005, weight_seed=0)
    attacks.AENS_I2V_MF(["coat_lite_mini", "resnet50"], depths={"coat_lite_mini": [2, 4], "resnet50": [2, 3]}, step_size=0.005, weight_seed=0)
    with pytest.raises(KeyError):
        attacks.ImageGuidedFMDirection_Adam([TINY], depth=5, step_size=0.005, weight_seed=0)
    with pytest.raises(ValueError, match="parallel blocks") as ei:
        attacks.ImageGuidedFMDirection_Adam(["coat_tiny"], depth=2, step_size=0.005, weight_seed=0)
    assert all(n in str(ei.value) for n in NAMES)
    import image_main
    monkeypatch.setattr(image_main, "OPT_PATH", str(tmp_path))
    base = ["--attack_method", "ImageGuidedFMDirection_Adam", "--step", "2"]
    for name in NAMES:
        for depth in ("1", "2", "3", "4"):
            a = image_main.arg_parse(base + ["--direction_image_model", name, "--depth", depth])
            assert image_main.build_attack(a).model_names == [name]
    for bad in (["--direction_image_model", "coat_mini"], ["--direction_image_model", TINY, "--depth", "5"],
                ["--direction_image_model", TINY, "--hw", "112"]):
        with pytest.raises(SystemExit):
            image_main.arg_parse(base + bad)


def test_i2v_trajectory_on_the_twin_matches_the_reference(eng):
    """4 steps of the I2V attack at depth 3 (two patch embeddings behind a class row passed) against `restate.run_attack` on the float32
    reference net (costs at rtol 2e-4, as tests/test_pit_cpu.py)."""
    torch.manual_seed(5)
    vid = torch.randn(1, 3, 2, 64, 64)
    atk = attacks.ImageGuidedFMDirection_Adam([TINY], depth=3, step_size=0.005, steps=4, engine=eng, graph_builder=graphs.build_tiny, weight_seed=0)
    adv = atk(vid, torch.zeros(1, dtype=torch.long), ["t"])
    g = graphs.build_tiny(TINY, (64, 64))
    check_trajectory(atk, adv, CoatReference(g, weights.synthetic_state_dict(g, 0), [g.hook_for(3)], dtype=torch.float32), vid, rtol=2e-4, steps=4)
