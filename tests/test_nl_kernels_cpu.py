"""The non-local-block case table (tests/nl_cases.py) on the host simulation against the float64 references -- the scalar twins
`k_attn_gemm`, `k_softmax_rows` and `k_addmask` of tests/hostsim/hostsim_backend.cpp, which the CPU suites run the I3D planner on --,
a second run with the same bits, the checks that keep a case from passing vacuously, and the refusals of the three entries of
include/i2v_nl_launch.h.  tests/test_gpu_nl_kernels.py runs the same table on the device and holds it to these twins bit for bit."""
import pytest
import torch

from tests import nl_cases as nc
from tests.hostsim_util import hostsim_engine
from tests.make_nl_fixtures import load

E32 = load()


def test_the_fixture_covers_exactly_the_table():
    assert set(E32) == {c.id for c in nc.CASES}
    assert 250 <= len(nc.CASES) <= 400


@pytest.mark.parametrize("case", nc.CASES, ids=[c.id for c in nc.CASES])
def test_case_on_the_host_simulation(case):
    eng = hostsim_engine()
    first = nc.run(eng, case)
    nc.check(case, first, E32[case.id], report=print)
    second = nc.run(eng, case)
    diff = [n for n in first if not nc.same_bits(first[n], second[n])]
    assert not diff, f"{case.id}: a second run changed {diff}"


@pytest.mark.parametrize("cid", nc.INVARIANCE)
def test_a_clip_alone_has_its_bits_in_the_batched_launch(cid):
    case, eng = nc.BY_ID[cid], hostsim_engine()
    whole = nc.run(eng, case)
    name = "D" if case.op == "gemm1" else "C"
    for b in range(whole[name].shape[0]):
        alone = nc.run_clip_alone(eng, case, b)
        assert nc.same_bits(alone[name][0], whole[name][b]), (cid, b)
        assert bool((alone[name + "_slack"] == nc.SENTINEL).all())


# ---- generator sanity ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", nc.CASES, ids=[c.id for c in nc.CASES])
def test_inputs_are_finite_and_float32_torch_meets_the_bound(case):
    for name, t in nc.inputs(case).items():
        assert bool(torch.isfinite(t).all()), (case.id, name)
    ref, e32 = nc.reference(case), nc.fp32_errors(case)
    assert set(e32) == set(E32[case.id])
    for name, err in e32.items():
        assert bool(torch.isfinite(ref[name][1]).all()), (case.id, name)
        assert err <= nc.bound(E32[case.id][name]), (case.id, name, err, E32[case.id][name])


def _kws(*ops):
    return [c.kw for c in nc.CASES if c.op in ops]


def test_every_branch_parameter_takes_each_of_its_values():
    for form in (1, 2, 3):
        kws = _kws(f"gemm{form}")
        plain = [k for k in kws if not k.get("ksplit") and not k.get("block")]
        for axis in ("rows", "cols", "K"):
            assert set(nc.EDGES) <= {k[axis] for k in plain}, (form, axis)
        assert set(nc.KS) <= {k["K"] for k in plain} and {1, 2, 3} <= {k["K"] % 4 for k in plain}
        grids = {((k["rows"] + 63) // 64, (k["cols"] + 63) // 64) for k in plain}
        assert {(3, 1), (1, 3), (3, 2), (2, 3), (1, 1)} <= grids, (form, grids)
        chunks = {(k["K"] + 31) // 32 for k in plain}
        assert {1, 2, 3, 4} <= chunks
        views = {(nc.prod_spec(k)["a"]["T"], nc.prod_spec(k)["a"]["HW"]) for k in kws}
        assert {(t, hw) for hw in nc.VIEW_HW for t in nc.VIEW_T} <= views and {(3, 4), (2, 16)} <= views
        flags = {n: nc.prod_flags(nc.BY_ID[f"gemm{form}-flag-{n}"].kw) for n in ("all-set", "a-hw", "a-nstride", "a-base", "d-base")}
        assert flags["all-set"] == (True, True) and flags["a-nstride"] == flags["a-base"] == (False, True), flags
        assert flags["a-hw"][0] is False and (form == 1 or flags["d-base"] == (True, False)), flags
        other = "b" if form == 1 else "c"
        assert any(nc.prod_spec(k)["a"]["nstride"] > k["rows" if form != 1 else "K"] * nc.prod_spec(k)["a"]["HW"] for k in kws)
        assert any((nc.prod_spec(k)[other]["T"], nc.prod_spec(k)[other]["HW"]) != (nc.prod_spec(k)["a"]["T"], nc.prod_spec(k)["a"]["HW"]) for k in kws)
        assert {k.get("clips", 1) for k in kws} >= {1, 3}
        if form == 1:
            assert {k.get("scale", 1.0) for k in kws} == {1.0, 0.125}
            assert nc.prod_flags(nc.BY_ID["gemm1-flag-b-hw"].kw) == nc.prod_flags(nc.BY_ID["gemm1-flag-b-nstride"].kw) == (True, False)
            assert nc.prod_flags(nc.BY_ID["gemm1-flag-b-base"].kw) == (True, False)
            assert any(k["rows"] != k["cols"] and k.get("a") and k.get("b") for k in kws)
        else:
            assert {k.get("acc", 0) for k in kws} == {0, 1}
            assert any(nc.prod_spec(k)["N"] % 4 for k in kws) and any(k.get("d_off") for k in kws)
            split = [k for k in kws if k.get("ksplit")]
            assert {k["ksplit"] for k in split} == {2, 3, 8} and any(k.get("acc") for k in split) and any(k.get("clips", 1) == 3 for k in split)
            segs = {(k["K"], k["ksplit"]): [max(0, min(k["K"], (z + 1) * nc.kseg(k["K"], k["ksplit"])) - min(k["K"], z * nc.kseg(k["K"], k["ksplit"])))
                                            for z in range(k["ksplit"])] for k in split}
            assert segs[(64, 3)] == [32, 32, 0] and segs[(512, 2)] == [256, 256] and segs[(70, 2)] == [64, 6] and segs[(250, 8)][-1] == 26
            for ks in (2, 3, 8):
                last = [s[-1] for (K, n), s in segs.items() if n == ks]
                assert any(len(set(s)) == 1 for (K, n), s in segs.items() if n == ks), ks          # a whole number of segments
                assert any(32 < l and l % 32 for l in last) and any(0 < l < 32 for l in last), (ks, last)
    assert nc.prod_flags(nc.BY_ID["gemm3-flag-d-n"].kw) == (True, False)
    assert nc.BY_ID["gemm1-split4-ignored"].kw["ksplit"] == 4
    assert {k["block"] for k in _kws(*nc.PRODUCT_OPS) if k.get("block")} == {"S", "y", "dP", "dg", "dtheta", "dphi"}
    sm = _kws("softmax")
    assert {k["N"] for k in sm} >= set(nc.SM_N) and {k["rows"] for k in sm} >= set(nc.SM_ROWS)
    for N in nc.SM_N:
        assert {k["rows"] for k in sm if k["N"] == N} >= set(nc.SM_ROWS)
    assert {k["kind"] for k in sm if k["N"] > 256} >= set(nc.SM_KINDS) and {k["N"] for k in sm if k["kind"] == "equal"} == {1, 2, 64, 256, 512}
    am = _kws("addmask")
    assert {(k["adds"], k["gate"]) for k in am} >= {(a, g) for a in [(i, j, l) for i in (0, 1) for j in (0, 1) for l in (0, 1)] for g in ("bits", "mask", "none")}
    assert {(k["HW"], k["N"], k["gate_pad"] > 0) for k in am if k["gate"] == "bits"} >= {(hw, n, p) for hw in (5, 32, 49) for n in (1, 3) for p in (False, True)}
    assert {k["gain"] for k in am} == {0.0, 0.5}
    assert any(256 < k["N"] * k["C"] * k["HW"] < 1024 for k in am) and any(k["N"] * k["C"] * k["HW"] > 4096 * 256 for k in am)


def test_planted_edges_are_in_the_inputs():
    sat = nc.inputs(nc.BY_ID["softmax-N513-r5-sat-all-kinds"])["X"]
    assert float(sat.abs().max(1).values.min()) == pytest.approx(60) and float(sat.max() - sat.min()) > 100
    sp = nc.inputs(nc.BY_ID["softmax-N257-r5-spike-all-kinds"])["X"]
    assert sp.argmax(1).tolist() == [256, 255, 254, 253, 252]                   # row 0's maximum lies in the second trip, alone
    top = sp.topk(2, dim=1).values
    assert float((top[:, 0] - top[:, 1]).min()) >= 100
    sp = nc.inputs(nc.BY_ID["softmax-N513-r5-spike-all-kinds"])["X"]
    assert int(sp.argmax(1).min()) >= 508
    eq = nc.inputs(nc.BY_ID["softmax-N256-r5-equal"])["X"]
    assert bool((eq == eq[:, :1]).all())
    am = nc.inputs(nc.BY_ID["addmask-two-blocks-mask"])
    z = am["mask"] == 0
    assert int(z.sum()) > 50 and int((torch.signbit(am["mask"]) & z).sum()) > 10 and int((~torch.signbit(am["mask"]) & z).sum()) > 10
    assert int(torch.signbit(am["a0"]).logical_and(am["a0"] == 0).sum()) > 10
    keep = nc.inputs(nc.BY_ID["addmask-bits-N3-HW49-pad0"])["keep"]
    assert not bool((keep[0] == keep[1]).all()) and 0.3 < float(keep.float().mean()) < 0.9
    ch = nc.block_chain()
    assert float(ch["P"].sum(-1).sub(1).abs().max()) < 1e-6 and float(ch["dS"].abs().max()) > 0


# ---- refusals -----------------------------------------------------------------------------------------------------------------
def test_refusals_name_their_entry_and_write_nothing():
    eng = hostsim_engine()
    thunks, nothing, untouched, keep = nc.refusals(eng)
    assert len(thunks) >= 50
    for label, name, thunk in thunks:
        assert thunk() != 0, label
        text = eng.capi.i2v_last_error().decode()
        assert text.startswith(name + ": bad argument"), (label, text)
    for label, thunk in nothing:
        assert thunk() == 0, label
    assert untouched()
    del keep
    for cid in ("gemm2-split2-K100-accumulate", "softmax-N257-r5-sat-all-kinds", "addmask-two-blocks-bits"):     # the library goes on
        nc.check(nc.BY_ID[cid], nc.run(eng, nc.BY_ID[cid]), E32[cid])


# ---- the entries' declarations, tables and exports in step ----------------------------------------------------------------------
def test_header_ctypes_table_and_exports_agree():
    import ctypes
    import os
    import re
    from i2v_amd import lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "i2v_nl_launch.h")).read(), flags=re.S)
    assert sorted(set(re.findall(r"\b(i2v_nl_[a-z0-9_]+)\s*\(", text))) == sorted(lib.NL_EXPORTS)
    assert not set(lib.NL_EXPORTS) & set(lib.EXPORTS + lib.XF_EXPORTS)
    for struct, cname in ((lib.NlAct, "i2v_nl_act"), (lib.NlGemmDesc, "i2v_nl_gemm_desc"), (lib.NlAddMaskDesc, "i2v_nl_addmask_desc")):
        decl = re.search(r"typedef struct \{([^{}]*)\} " + cname + ";", text).group(1)
        assert [n for n, _ in struct._fields_] == re.findall(r"[\s*,](\w+)(?:\[3\])?(?=[,;])", decl), cname
    # 5 int32 (+ 4 padding), two views of 24 bytes, 8 + 8 + 4 + 4, two pointers, 3 x 4 (+ 4 padding), a pointer
    assert ctypes.sizeof(lib.NlAct) == 24 and ctypes.sizeof(lib.NlGemmDesc) == 136 and ctypes.sizeof(lib.NlAddMaskDesc) == 16 + 48 + 16 + 8 + 4 * 4 + 8
    hs = hostsim_engine().capi
    assert all(hasattr(hs, n) for n in lib.NL_EXPORTS)
    import __graft_entry__ as ge
    ge.build()
    cd = ctypes.CDLL(lib.LIB_PATH)
    assert all(hasattr(cd, n) for n in lib.NL_EXPORTS) and cd.i2v_abi_version() == 1
