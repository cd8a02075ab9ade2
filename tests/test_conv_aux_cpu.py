"""The grouped / depthwise / squeeze-and-excitation case table (tests/conv_aux_cases.py) on the CPU.  The two convolution kernels have no
host twin, so for them nothing here runs a kernel; what is checked:

  * the packers, which every build exports: the packed operands, tap masks and class geometry of every conv case, put through the formulas
    of csrc/i2v_params.h as a plain float64 loop (`params_eval`), equal the float64 convolution and its autograd gradient at both
    strides -- this separates "packed wrong" from "kernel wrong" when a device case fails;
  * the SE cases through `i2v_se_f32` on the host simulation (csrc/i2v_se_host.h) at the device's bounds, and the written-out float64
    node against a literal SE module under autograd;
  * the committed float32 fixture: its ids and names, and three cases recomputed;
  * the restated plan arithmetic: every case still takes the branch it exists for;
  * sensitivity: each wrong variant of the reference -- a plausible slip of a kernel or a packer -- is fed to `check` as what the device
    returned; the cases it must break fail, and every case it cannot change still passes."""
import numpy as np
import pytest
import torch

from tests import conv_aux_cases as cc
from tests.hostsim_util import hostsim_engine
from tests.make_conv_aux_fixtures import compute, load

E32 = load()
IDS = [c.id for c in cc.CASES]


def _kw(id):
    return cc.BY_ID[id].kw


# ---- the table ----------------------------------------------------------------------------------------------------------------------
def test_the_fixture_covers_the_table_and_three_cases_recompute():
    assert list(E32) == IDS
    assert all(tuple(E32[c.id]) == cc.VALUE[c.op] for c in cc.CASES)
    ids = ("gconv-g2x64-3x56-s2-n1-b-mask", "dwconv-c5-k3-5x8-s2-n2-rg-mask", "se-n2-c16-rd6-hw20-arg-hot")
    assert compute(ids) == {i: E32[i] for i in ids}
    # no bound is vacuous: every e32 is some float32 roundings of the plane's scale.  The largest are planes whose value cancels: dx of the
    # 2048-channel SE row where g s and dmh nearly do (1.7e-5), the 4-term gradient of a 1 x 1 grouped plane (4.2e-6)
    assert all(e < 1e-4 for v in E32.values() for e in v.values())


def test_the_gconv_cases_take_the_branches_they_exist_for():
    plan = {c.id: (cc.port_plan(c, False), cc.port_plan(c, True)) for c in cc.GCONV_CASES}
    f, b = plan["gconv-g2x4-2x63-s1-n2-br-none"]
    assert f["pitch"] == 65 > 64 and (f["waves"], f["rows"], f["lds_bytes"]) == (4, 14, 14560)           # the second staging trip
    assert plan["gconv-g2x4-5x1-s1-n5--none"][0]["rows"] == 360 and cc.lpr(3) == 8
    f, b = plan["gconv-g2x32-3x56-s1-n1-br-none"]
    assert (f["waves"], f["lds_bytes"]) == (1, 44544) and f["lds_bytes"] > 40 * 1024                      # no width fits: the smallest image
    f, b = plan["gconv-g2x64-3x56-s1-n1--none"]
    assert f["lds_bytes"] == 89088 > 64 * 1024                                                           # the attribute path
    assert plan["gconv-g2x64-3x56-s2-n1-b-mask"][1]["lds_bytes"] == 115200
    f, b = plan["gconv-g2x16-5x28-s2-n2-rg-mask"]
    assert cc.lpr(f["pitch"]) == 32 and cc.lpr(b["pitch"]) == 16 and b["waves"] == 2
    assert [c[:2] for c in cc.classes(5, 28, 2, True)] == [(3, 14), (3, 14), (2, 14), (2, 14)]
    assert len({c[:2] for c in cc.classes(7, 9, 2, True)}) == 4
    assert cc.lpr(plan["gconv-g3x16-6x15-s1-n2-br-none"][0]["pitch"]) == 32
    assert {cc.lpr(p["pitch"]) for fb in plan.values() for p in fb} == {8, 16, 32, 64}
    kws = [c.kw for c in cc.GCONV_CASES]
    assert {k["gw"] for k in kws} == {4, 8, 16, 32, 64} and {k["N"] for k in kws} == {1, 2, 5} and {k["G"] for k in kws} == {2, 3}
    for gw in (4, 8, 16, 32, 64):
        assert {k["st"] for k in kws if k["gw"] == gw and k["H"] != k["W"]} == {1, 2}
    assert any(k["H"] < k["W"] for k in kws) and any(k["H"] > k["W"] for k in kws)
    total = [k["N"] * cc.out_plane(k["H"], k["st"]) * cc.out_plane(k["W"], k["st"]) for k in kws]
    assert any(t % 64 == 0 for t in total) and any(t % 64 for t in total)
    # the recorded limit: tiny planes at gw 64 are refused
    assert cc.gconv_plan(64, 2, 130, 1, False) is None and cc.gconv_refused_lds(64, 2, 130, 1, False) == 202752
    assert cc.gconv_plan(64, 3, 3, 2, True) is None and cc.gconv_refused_lds(64, 3, 3, 2, True) == 261120
    assert cc.gconv_plan(64, 2, 2, 2, False) is None and cc.gconv_refused_lds(64, 2, 2, 2, False) == 261120
    assert cc.gconv_plan(64, 7, 7, 1, True)["lds_bytes"] == 36864                # resnext101_32x8d's layer4 at 224: the 7 x 7 launches fit, at one wave


def test_the_dwconv_cases_take_the_branches_they_exist_for():
    plan = {c.id: (cc.port_plan(c, False), cc.port_plan(c, True)) for c in cc.DWCONV_CASES}
    f, b = plan["dwconv-c3-k5-6x12-s2-n2-b-mask"]
    assert (f["v4"], f["pitch"]) == (1, 20) and (b["v4"], b["pitch"]) == (0, 10)
    f, b = plan["dwconv-c5-k3-5x8-s2-n2-rg-mask"]
    assert f["v4"] == 1 and b["v4"] == 1
    f, b = plan["dwconv-c3-k5-2x160-s2-n2-br-none"]
    assert (f["first_waves"], f["waves"], f["lds_bytes"]) == (16, 8, 31584)
    f, b = plan["dwconv-c2-k5-2x200-s2-n1-r-gate"]
    assert (f["first_waves"], f["waves"]) == (16, 4)
    assert cc.dwconv_plan(5, 1, 3300, 1, False) is None                          # 5 rows x 3308 floats at one wave: 66 160 B > 64 KB
    # all eight instantiations: K x ALL / tapmask x V4 / plain
    seen = set()
    for c in cc.DWCONV_CASES:
        for backward, p in enumerate(plan[c.id]):
            seen.add((c.kw["k"], "mask" if backward and c.kw["st"] == 2 else "all", p["v4"]))
    assert seen == {(k, t, v) for k in (3, 5) for t in ("all", "mask") for v in (0, 1)}
    # 16-byte staging dropped by alignment alone
    for cid, how in cc.V4_DROPPED:
        c = cc.BY_ID[cid]
        base = [cc.port_plan(c, bw) for bw in (False, True)]
        dropped = [cc.port_plan(c, bw, **how) for bw in (False, True)]
        assert any(p["v4"] for p in base) and not any(p["v4"] for p in dropped), (cid, how)
    kws = [c.kw for c in cc.DWCONV_CASES]
    assert {k["C"] for k in kws} >= {3, 5, 6} and {k["N"] for k in kws} == {1, 2, 3, 5}
    assert any(k["H"] * k["W"] == 49 and k["N"] == 3 and k["gout"] for k in kws) and any(k["H"] * k["W"] == 49 and k["N"] == 1 and k["gout"] for k in kws)


@pytest.mark.parametrize("cases", (cc.GCONV_CASES, cc.DWCONV_CASES), ids=("gconv", "dwconv"))
def test_every_epilogue_occurs_for_each_kernel(cases):
    kws = [c.kw for c in cases]
    assert any(not k["shift"] for k in kws) and any(k["shift"] and not k["relu"] for k in kws) and any(k["relu"] and k["gout"] for k in kws)
    assert {k["bwd"] for k in kws} == {"gate", "mask", "none"}
    assert any(k["gap"] for k in kws) and any(k["sgap"] for k in kws) and any(not k["gap"] and not k["sgap"] for k in kws)


def test_the_se_cases_take_the_branches_they_exist_for():
    kws = [c.kw for c in cc.SE_CASES]
    assert any(k["HW"] > 256 and k["HW"] % 4 for k in kws) and any(k["HW"] > 256 and k["HW"] % 4 == 0 and k["HW"] % 256 for k in kws)
    assert {1, 3, 4} <= {k["HW"] for k in kws} and {6, 70, 300, 2048} <= {k["C"] for k in kws} and {1, 6, 16, 128} <= {k["rd"] for k in kws}
    assert any(k["N"] * k["HW"] % 32 for k in kws) and any(k["N"] * k["HW"] % 4 == 0 and k["N"] * k["HW"] % 1024 for k in kws)
    assert {(k["res"], k["relu"], k["gout"]) for k in kws} >= {(1, 1, 1), (0, 1, 1), (1, 0, 0), (0, 0, 0)}
    assert all(_kw(i)["HW"] % 4 == 0 and _kw(i)["gap"] % 4 == 0 for i in cc.SE_MISALIGNED)
    for cid in cc.FRAME_INVARIANCE:
        assert _kw(cid)["N"] > 1


def test_the_hot_case_saturates_and_has_exact_zeros():
    ref = cc.reference(cc.HOT)
    s, h = ref["s"][1], ref["h"][1]
    sat = torch.minimum(s, 1 - s) < 1e-6
    assert int(sat.sum()) == s.numel() // 2 and bool((s[sat] > 0.5).any()) and bool((s[sat] < 0.5).any())
    s32 = cc.evaluate(cc.HOT, torch.float32)["s"][1]
    assert bool((s32 == 1.0).any())                                 # float32: 1 - s is exactly 0 there, the backward's s (1 - s) with it
    assert bool((h == 0).any()) and bool((h > 0).any())
    assert all(bool((cc.reference(c)["h"][1] > 0).all()) for c in cc.SE_CASES if c is not cc.HOT)    # the exact zeros are this case's alone


# ---- the packers ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", cc.CONV_CASES, ids=[c.id for c in cc.CONV_CASES])
def test_the_packed_operands_in_the_stated_formula_are_the_convolution(case):
    kw = case.kw
    fwd, bwd, cls = cc.packed(case)
    assert not np.isnan(fwd).any() and not np.isnan(bwd).any()                                   # written whole
    assert [c[:4] for c in cls] == cc.classes(kw["H"], kw["W"], kw["st"], True)
    k = 3 if case.op == "gconv" else kw["k"]
    masks = [c[4] for c in cls]
    if kw["st"] == 1:
        assert masks == [(1 << (k * k)) - 1]
    else:       # the four parities share the k x k slots out between them: per axis (k + 1) / 2 slots for parity pad % 2, k / 2 for the other
        assert sum(bin(m).count("1") for m in masks) == k * k and len(masks) == 4
    y, dx = cc.conv_by_params(case)
    ref = cc.conv_eval(dataclass_none(case))
    assert y.shape == tuple(ref["y"][1].shape) and dx.shape == tuple(ref["dx"][1].shape)
    for got, want in ((y, ref["y"][1]), (dx, ref["dx"][1])):
        assert float(np.abs(got - want.numpy()).max()) <= 1e-13 * max(1.0, float(want.abs().max()))


def dataclass_none(case):
    """The case with no epilogue: the bare sums."""
    d = dict(case.kw, shift=0, relu=0, gout=0, bwd="none")
    return cc.Case(case.id, case.op, tuple(sorted(d.items())))


def test_the_pack_entries_refuse_bad_arguments():
    capi = cc.host_capi()
    w = np.zeros(64, np.float32)
    assert capi.i2v_gconv_pack_f32(None, 1, 4, 1, 3, 3, None, None, None) != 0
    assert capi.i2v_last_error().decode().startswith("i2v_gconv_pack_f32:")
    assert capi.i2v_dwconv_pack_f32(cc.P(w.ctypes.data), 1, 4, 1, 3, 3, None, None) != 0
    assert capi.i2v_last_error().decode().startswith("i2v_dwconv_pack_f32:")


# ---- the reference ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", cc.CASES, ids=IDS)
def test_the_reference_passes_its_own_check_and_a_spoilt_sentinel_does_not(case):
    inp = cc.inputs(case)
    assert all(bool(torch.isfinite(t).all()) for t in inp.values() if t.dtype.is_floating_point)
    if case.op != "se":
        m = inp["mask"]
        assert bool(((m > 0) == inp["on"]).all())                                                  # the mask's signs are the gate's bits
        tiny = torch.finfo(torch.float32).tiny
        assert bool(((m == 0) | (m.abs() >= tiny)).all())                                          # no denormals
        if int((~inp["on"]).sum()) >= 3:
            assert bool((m < 0).any()) and bool(torch.signbit(m[m == 0]).any()) and not bool(torch.signbit(m[m == 0]).all())   # negatives, +0.0 and -0.0
    cc.check(case, cc.as_got(case, cc.reference(case)), E32[case.id])
    spoilt = cc.as_got(case, cc.reference(case))
    spoilt["dx_slack"][-1] = 0.0
    with pytest.raises(AssertionError, match="dx_slack"):
        cc.check(case, spoilt, E32[case.id])
    if "ygate" in spoilt:
        spoilt = cc.as_got(case, cc.reference(case))
        spoilt["ygate"][-1] = 0                                                                    # a word past the last row
        with pytest.raises(AssertionError, match="ygate"):
            cc.check(case, spoilt, E32[case.id])


@pytest.mark.parametrize("case", cc.SE_CASES, ids=[c.id for c in cc.SE_CASES])
def test_the_written_out_node_is_a_literal_se_module_under_autograd(case):
    kw, inp = case.kw, cc.inputs(case)
    N, C, rd, HW = kw["N"], kw["C"], kw["rd"], kw["HW"]
    x = inp["x"].double().reshape(N, C, HW, 1).requires_grad_(True)
    fc1, fc2 = torch.nn.Conv2d(C, rd, 1).double(), torch.nn.Conv2d(rd, C, 1).double()
    with torch.no_grad():
        fc1.weight.copy_(inp["w1"].double().reshape(rd, C, 1, 1)); fc1.bias.copy_(inp["b1"].double())
        fc2.weight.copy_(inp["w2"].double().reshape(C, rd, 1, 1)); fc2.bias.copy_(inp["b2"].double())
    m = x.mean((2, 3), keepdim=True)
    m.retain_grad()
    scaled = x * torch.sigmoid(fc2(torch.relu(fc1(m))))
    y = scaled + (inp["r"].double().reshape(N, C, HW, 1) if kw["res"] else 0)
    y = torch.relu(y) if kw["relu"] else y
    scaled.backward(inp["g"].double().reshape(N, C, HW, 1))
    ref = cc.reference(case)
    close = lambda a, b: float((a.reshape(b.shape) - b).abs().max()) <= 1e-12 * max(1.0, float(b.abs().max()))
    assert close(y.detach(), ref["y"][1]) and close(x.grad, ref["dx"][1]) and close(m.detach(), ref["m"][1])
    assert close(m.grad / HW, ref["dmh"][1])


# ---- the SE node on the host simulation -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", cc.SE_CASES, ids=[c.id for c in cc.SE_CASES])
def test_se_case_on_the_host_simulation(case):
    eng = hostsim_engine()
    first, second = cc.run(eng, case), cc.run(eng, case)
    cc.check(case, first, E32[case.id], report=print, rmw=True)
    assert all(cc.same_bits(first[n], second[n]) for n in first)


@pytest.mark.parametrize("cid", [c for c in cc.FRAME_INVARIANCE if c.startswith("se-")])
def test_se_frame_0_has_the_bits_of_a_one_frame_call_on_the_host_simulation(cid):
    eng, case = hostsim_engine(), cc.BY_ID[cid]
    whole, alone = cc.run(eng, case), cc.run(eng, case, frames=1)
    for name in cc.VALUE["se"]:
        assert alone[name].shape[0] == 1 and cc.same_bits(alone[name][0], whole[name][0]), (cid, name)


# ---- sensitivity: the table must bite -------------------------------------------------------------------------------------------------
def _ids(cases, pred):
    return {c.id for c in cases if pred(c.kw)}


CONV, SE = {c.id for c in cc.CONV_CASES}, {c.id for c in cc.SE_CASES}
GC = {c.id for c in cc.GCONV_CASES}


def _by_params(**how):
    return lambda case: cc.conv_eval(case, sums=cc.conv_by_params(case, **how))


# variant -> (the wrong reference, the cases that must fail, the cases it cannot change, which must still pass)
VARIANTS = {
    "taps_transposed": (lambda c: cc.conv_eval(c, transposed=True), _ids(cc.CONV_CASES, lambda k: k["H"] * k["W"] > 1), _ids(cc.CONV_CASES, lambda k: k["H"] * k["W"] == 1)),      # (a 1 x 1 plane sees the centre tap alone)
    "last_column_from_the_one_before": (lambda c: cc.conv_eval(c, last_col=True), _ids(cc.CONV_CASES, lambda k: k["W"] > 1), _ids(cc.CONV_CASES, lambda k: k["W"] == 1)),
    "stride_2_classes_swapped": (_by_params(swap_classes=True), _ids(cc.CONV_CASES, lambda k: k["st"] == 2 and (k["H"] > 1 or k["W"] > 1)),
                                 _ids(cc.CONV_CASES, lambda k: k["st"] == 1 or (k["H"] == 1 and k["W"] == 1))),
    "next_groups_filter": (lambda c: cc.conv_eval(c, next_group=True), GC, CONV - GC),
    "shift_after_relu": (lambda c: cc.conv_eval(c, shift_after_relu=True), _ids(cc.CONV_CASES, lambda k: k["shift"] and k["relu"]),
                         _ids(cc.CONV_CASES, lambda k: not (k["shift"] and k["relu"]))),
    "gate_from_mask_ge_0": (lambda c: cc.conv_eval(c, mask_ge=True), _ids(cc.CONV_CASES, lambda k: k["bwd"] == "mask"), _ids(cc.CONV_CASES, lambda k: k["bwd"] != "mask")),
    "no_zero_rows_between_frames": (_by_params(bleed=True), _ids(cc.CONV_CASES, lambda k: k["N"] > 1), _ids(cc.CONV_CASES, lambda k: k["N"] == 1)),
    "se_mean_over_hw_minus_1": (lambda c: cc.se_eval(c, mean_short=True), SE, set()),
    "se_s_for_s_1_minus_s": (lambda c: cc.se_eval(c, ds_plain=True), SE, set()),
    "se_h_ge_0": (lambda c: cc.se_eval(c, h_ge=True), {cc.HOT.id}, SE - {cc.HOT.id}),
}


@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_a_wrong_reference_fails_exactly_its_cases(variant):
    wrong, must_fail, unaffected = VARIANTS[variant]
    assert must_fail and not must_fail & unaffected
    family = CONV if must_fail <= CONV else SE
    assert must_fail | unaffected == family, sorted(family - must_fail - unaffected)
    failed = set()
    for case in cc.CASES:
        if case.id not in family:
            continue
        try:
            cc.check(case, cc.as_got(case, wrong(case)), E32[case.id])
        except AssertionError:
            failed.add(case.id)
    assert must_fail <= failed, (variant, sorted(must_fail - failed))
    assert not unaffected & failed, (variant, sorted(unaffected & failed))


def test_the_unswitched_formula_route_passes_every_conv_case():
    """The route the class-swap and frame-bleed variants take, without a switch: it is the reference."""
    for case in cc.CONV_CASES:
        cc.check(case, cc.as_got(case, _by_params()(case)), E32[case.id])


def test_a_nonzero_where_the_gate_is_off_and_a_wrong_gate_bit_fail():
    case = cc.BY_ID["gconv-g2x8-9x5-s1-n5-brg-gate"]
    got = cc.as_got(case, cc.reference(case))
    off = cc.reference(case)["dx"][3]
    n, c, i, j = (int(v[0]) for v in torch.nonzero(off, as_tuple=True))
    got["dx"][n, c, i, j] = -0.0                                                                   # equal to zero, not +0.0
    with pytest.raises(AssertionError, match=r"not \+0.0"):
        cc.check(case, got, E32[case.id])
    got = cc.as_got(case, cc.reference(case))
    got["ygate"][cc.GFRONT] ^= 1
    with pytest.raises(AssertionError, match="ygate"):
        cc.check(case, got, E32[case.id])
    got = cc.as_got(case, cc.reference(case))
    nbits = case.kw["N"] * 45
    assert nbits % 32
    got["ygate"][cc.GFRONT + nbits // 32] |= -(1 << 31)                                              # an unused high bit of the last word
    with pytest.raises(AssertionError, match="ygate"):
        cc.check(case, got, E32[case.id])
