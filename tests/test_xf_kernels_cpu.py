"""The shared-launch case table (tests/xf_cases.py) on the host simulation against the float64 references -- the GEMM, LayerNorm and
patchify twins of csrc/i2v_xf_host.h, which the CPU suites of ConvNeXt, Mixer, CaiT, ConViT and XCiT run their planners on --, the
checks that keep a case from passing vacuously, and the refusals of the GEMM twin.  Softmax, attention and the embed entries are
device-only (tests/test_gpu_xf_kernels.py); their generators and references are checked here all the same."""
import pytest
import torch

from tests import xf_cases as xc
from tests.hostsim_util import hostsim_engine
from tests.make_xf_fixtures import load

E32 = load()
HOST = [c for c in xc.CASES if c.op in xc.HOST_OPS]


def test_the_fixture_covers_the_table():
    assert set(E32) == {c.id for c in xc.CASES}
    assert 250 <= len(xc.CASES) <= 600


@pytest.mark.parametrize("case", HOST, ids=[c.id for c in HOST])
def test_case_on_the_host_simulation(case):
    xc.check(case, xc.run(hostsim_engine(), case), E32[case.id], report=print)


@pytest.mark.parametrize("cid", xc.INVARIANCE)
def test_a_batch_alone_has_its_bits_in_the_batched_launch(cid):
    case, eng = xc.BY_ID[cid], hostsim_engine()
    whole = xc.run(eng, case)
    for b in range(whole["C"].shape[0]):
        alone = xc.run_batch_alone(eng, case, b)
        assert xc.same_bits(alone["C"], whole["C"][b]), (cid, b)
        assert bool((alone["C_slack"] == xc.SENTINEL).all())


# ---- generator sanity ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", xc.CASES, ids=[c.id for c in xc.CASES])
def test_inputs_are_finite_and_float32_torch_meets_the_bound(case):
    for name, t in xc.inputs(case).items():
        assert bool(torch.isfinite(t).all()), (case.id, name)
    ref, e32 = xc.reference(case), xc.fp32_errors(case)
    assert set(e32) == set(E32[case.id])
    for name, err in e32.items():
        assert bool(torch.isfinite(ref[name][1]).all()), (case.id, name)
        assert err <= xc.bound(E32[case.id][name]), (case.id, name, err, E32[case.id][name])


def _vals(op, key, default=None):
    return {c.kw.get(key, default) for c in xc.CASES if c.op == op}


def test_every_branch_parameter_takes_each_of_its_values():
    gemm = [c for c in xc.CASES if c.op == "gemm"]
    flags = {(c.kw["la"], c.kw["lb"]) + xc.gemm_flags(c.kw) for c in gemm}
    for la, lb in xc.LAYOUTS:
        assert (la, lb, 1, 1, 1, 1) in flags and (la, lb, 0, 0, 0, 0) in flags, (la, lb)
    only = {f[2:] for f in flags}
    assert {(0, 1, 1, 1), (1, 0, 1, 1), (1, 1, 0, 1), (1, 1, 1, 0)} <= only
    # each switch of a flag, on its own, drops exactly that flag
    want = {"a-ld": 0, "a-base": 0, "a-bi6": 0, "a-bo": 0, "b-ld": 1, "b-base": 1, "b-bi6": 1, "b-bo": 1, "c-ld": 2, "c-base": 2, "c-bi": 2, "c-bo": 2,
            "c-aligned-R-not": 2, "c-aligned-R-off2": 2, "c-aligned-C2-not": 2, "c-aligned-H-not": 2, "bias-not-c-vec": 3, "bias-off2-R": 3,
            "Am-Bk-a-ld": 0, "Am-Bk-a-base": 0, "Ak-Bn-b-ld": 1, "Ak-Bn-b-base": 1, "Am-Bn-a-bi": 0, "Am-Bn-b-bi": 1}
    for name, which in want.items():
        f = xc.gemm_flags(xc.BY_ID["gemm-flag-" + name].kw)
        assert f == tuple(int(i != which) for i in range(4)), (name, f)
    assert xc.gemm_flags(xc.BY_ID["gemm-flags-all-set"].kw) == (1, 1, 1, 1)
    assert xc.gemm_flags(xc.BY_ID["gemm-head6-qk"].kw)[:2] == (0, 0) and xc.gemm_flags(xc.BY_ID["gemm-head6-pv"].kw)[1:3] == (0, 0)
    for dim in ("M", "N"):
        for path in (True, False):
            assert set(xc.EDGES) <= {c.kw[dim] for c in gemm if c.kw.get("vec", True) == path}, (dim, path)
    for path in (True, False):
        assert set(xc.KS) <= {c.kw["K"] for c in gemm if c.kw.get("vec", True) == path}
    assert _vals("gemm", "mode", "plain") == set(xc.EPI) and {1.0, 0.125, 0.3} <= _vals("gemm", "alpha", 1.0)
    assert _vals("gemm", "R") == {None, "sep", "inplace"} and _vals("gemm", "bias", False) >= {True, False}
    assert {(c.kw.get("bias", False), c.kw.get("R")) for c in gemm} >= {(True, None), (False, "sep"), (True, "sep"), (False, None)}
    assert any(c.kw.get("nb_in0") for c in gemm) and any(c.kw.get("b_shared") for c in gemm) and any(c.kw.get("inner", 1) > 1 and c.kw.get("outer", 1) > 1 for c in gemm)
    assert {c.kw["degenerate"][0] for c in gemm if c.kw.get("degenerate")} == {"M", "N", "batch"}
    # tails under a set flag
    for r in (1, 2, 3):
        assert any(c.kw["N"] % 4 == r and xc.gemm_flags(c.kw)[2] and xc.gemm_spec(c.kw)["c"]["ld"] > c.kw["N"] for c in gemm)
        assert any(c.kw["K"] % 4 == r and c.kw["la"] == c.kw["lb"] == "k" and xc.gemm_flags(c.kw)[:2] == (1, 1) for c in gemm)
        assert any(c.kw["M"] % 4 == r and c.kw["la"] == "m" and xc.gemm_flags(c.kw)[0] for c in gemm)
        assert any(c.kw["N"] % 4 == r and c.kw["lb"] == "n" and xc.gemm_flags(c.kw)[1] for c in gemm)
    assert _vals("ln", "rows") == set(xc.LN_ROWS) and _vals("ln", "C") >= set(xc.LN_C) and _vals("ln", "add") == set(xc.LN_ADD)
    assert _vals("ln", "mis") == {None, "gamma", "beta", "x", "out", "dy", "dx", "add0", "add1"} and _vals("ln", "alias") == {None, "a0", "a1", "block"}
    assert {c.kw["add"] for c in xc.CASES if c.op == "ln" and not c.kw.get("alias") and not c.kw.get("mis")} == set(xc.LN_ADD)
    assert _vals("softmax", "N") == set(xc.SM_N) and _vals("softmax", "rows") == set(xc.SM_ROWS) and _vals("softmax", "kind") == set(xc.SM_KINDS)
    assert _vals("softmax", "scale") == {1.0, 0.125}
    sm = [c.kw for c in xc.CASES if c.op == "softmax"]
    for N in xc.SM_N:
        assert {k["ld"] - xc._r4(N) for k in sm if k["N"] == N} >= {0, 8}
    assert {k["kind"] for k in sm if k["N"] > 259} == set(xc.SM_KINDS)
    assert {(k["T"], k["dh"]) for k in (c.kw for c in xc.CASES if c.op == "attn")} >= {(5, 6), (4, 8), (129, 8)}
    for op in ("patchify", "embed"):
        assert _vals(op, "patch") == {4, 8, 16} and _vals(op, "cin") == {1, 3} and _vals(op, "g") == {1, 2, 3} and _vals(op, "acc") == {0, 1}
    assert _vals("embed", "npre") == {1, 2} and _vals("embed", "ex") == {True, False} and _vals("embed", "pos0") == {True, False}


def test_planted_edges_are_in_the_inputs():
    H = xc.inputs(xc.BY_ID["gemm-epi-gelu-bwd-vec"])["H"]
    assert float(H.min()) < -5 and float(H.max()) > 5 and int((H == 0).sum()) > 10
    x = xc.inputs(xc.BY_ID["ln-r5-C64-mean100"])["x"]
    assert float((x.mean(1) - 100).abs().max()) < 0.01 and 0.005 < float(x.std()) < 0.02
    sm = {k: next(c for c in xc.CASES if c.op == "softmax" and c.kw["kind"] == k and c.kw["N"] == 263) for k in xc.SM_KINDS}
    big = xc.inputs(sm["big"])["X"]
    assert float(big.abs().max(1).values.min()) == pytest.approx(80) and float(big.abs().max()) == pytest.approx(80)
    assert not bool(torch.isfinite(torch.exp(xc.inputs(sm["huge"])["X"])).all())              # a naive float32 exp overflows
    eq = xc.inputs(sm["equal"])["X"]
    assert bool((eq == eq[:, :1]).all())
    sp = xc.inputs(sm["spike"])["X"]
    top = sp.topk(2, dim=1).values
    assert float((top[:, 0] - top[:, 1]).min()) >= 100
    P_ = xc.reference(sm["spike"])["P"][1].float()
    assert int((P_ > 0.5).sum()) == sp.shape[0] and float(P_.sum()) == pytest.approx(sp.shape[0])
    e = xc.inputs(next(c for c in xc.CASES if c.op == "embed" and c.kw["pos0"]))
    assert not bool(e["pos"][:1].any()) and bool(e["pos"][-1].any())


# ---- refusals -----------------------------------------------------------------------------------------------------------------
def test_gemm_refusals_name_the_launch_and_write_nothing():
    eng = hostsim_engine()
    thunks, untouched, keep = xc.gemm_refusals(eng)
    assert len(thunks) >= 7
    for label, name, thunk in thunks:
        assert thunk() != 0, label
        text = eng.capi.i2v_last_error().decode()
        assert text.startswith(name + ":"), (label, text)
    assert untouched()
    del keep
    case = xc.BY_ID["gemm-flags-all-set"]                  # the library goes on after the refusals
    xc.check(case, xc.run(eng, case), E32[case.id])


# ---- the entries' declarations, tables and exports in step ----------------------------------------------------------------------
def test_header_ctypes_table_and_exports_agree():
    import ctypes
    import os
    import re
    from i2v_amd import lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "i2v_xf_launch.h")).read(), flags=re.S)
    assert sorted(set(re.findall(r"\b(i2v_xf_[a-z0-9_]+)\s*\(", text))) == sorted(lib.XF_EXPORTS)
    others = (lib.EXPORTS + lib.LOADER_EXPORTS + lib.VIT_EXPORTS + lib.SWIN_EXPORTS + lib.CONVNEXT_EXPORTS + lib.MIXER_EXPORTS + lib.CAIT_EXPORTS
              + lib.CONVIT_EXPORTS + lib.XCIT_EXPORTS)
    assert not set(lib.XF_EXPORTS) & set(others)
    # the descriptor is VitGemm without its four *_vec fields: 4 + 4 + 3 strides, 7 pointers, 5 sizes, alpha, mode
    fields = [n for n, _ in lib.XfGemmDesc._fields_]
    decl = re.search(r"typedef struct \{(.*?)\} i2v_xf_gemm_desc;", text, flags=re.S).group(1)
    assert fields == re.findall(r"[\s*,](\w+)(?=[,;])", decl) and ctypes.sizeof(lib.XfGemmDesc) == 8 * 18 + 4 * 8
    hs = hostsim_engine().capi
    assert all(hasattr(hs, n) for n in lib.XF_HOST_PROTOS) and not hasattr(hs, "i2v_xf_softmax_f32") and not hasattr(hs, "i2v_xf_softmax_bwd_f32")
    assert set(lib.XF_EXPORTS) - set(lib.XF_HOST_PROTOS) == {"i2v_xf_softmax_f32", "i2v_xf_softmax_bwd_f32"}
    import __graft_entry__ as ge
    ge.build()
    cd = ctypes.CDLL(lib.LIB_PATH)
    assert all(hasattr(cd, n) for n in lib.XF_EXPORTS) and cd.i2v_abi_version() == 1
