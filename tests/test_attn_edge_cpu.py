"""The talking-heads / gated positional attention case table (tests/attn_edge_cases.py) on the CPU: every case through the C entries of the
host simulation, which runs the five launches as scalar code (csrc/i2v_cait_host.h, csrc/i2v_convit_host.h), against float64; and that the
table can tell a wrong kernel from a right one:

  * the table takes the branches its comments name (LDS bytes either side of 64 KiB and at the 160 KiB budget, wave-task counts, pads);
  * the conditions that make the `huge`, `spike`, `equal` and `bl-large` kinds worth having, asserted on the float64 logits;
  * the committed fixture: its ids and names, three cases recomputed, every e32 below 1e-4 (no bound is vacuous);
  * the exact relations: reruns, frame 0 of an F-frame call, one head of an H-head ConViT call, CaiT `identity` against ungated ConViT
    (values), c = 1 with a zero table against the ungated call (bits);
  * the refusals of the three small launches, and the LDS refusal boundaries of both attention launches -- the refusal functions are
    host code both builds share (csrc/i2v_cait_kernels.h, csrc/i2v_convit_kernels.h);
  * sensitivity: each wrong form of the reference is fed to `check` as what the device returned; the cases it must break fail, and
    every other case still passes."""
import pytest
import torch

from tests import attn_edge_cases as ac
from tests.hostsim_util import hostsim_engine
from tests.make_attn_edge_fixtures import compute, load

E32 = load()
ATTN = {c.id: c for c in ac.ATTN_CASES}


@pytest.fixture(scope="module")
def eng():
    return hostsim_engine()


def _ids(pred, cases=ac.ATTN_CASES):
    return {c.id for c in cases if pred(c)}


def _same(a, b):
    assert a.keys() == b.keys()
    return [n for n in a if not ac.same_bits(a[n], b[n])]


# ---- the table ----------------------------------------------------------------------------------------------------------------------
def test_the_table_takes_the_branches_its_comments_name():
    lds = {c.id: ac.lds_bytes(c) for c in ac.ATTN_CASES}
    assert (lds["cait-f1-T240-h4-dh8-dense"], lds["cait-f1-T256-h4-dh8-dense"], lds["cait-f1-T144-h16-dh4-dense"]) == (62464, 66560, 151552)
    assert (lds["convit-f1-T1008-h1-dh4-ungated"], lds["convit-f1-T1009-h1-dh4-gated"]) == (64768, 65792)
    assert ac.lds_bytes(ac._a("cait", 1, 145, 16, 4, "dense")) > ac.LDS_MAX >= max(lds.values())
    for op, HM in (("cait", 4), ("cait", 8), ("cait", 16), ("convit", 1)):        # raise_lds on every instantiation, and a case below it
        mine = [c for c in ac.ATTN_CASES if c.op == op and (op == "convit" or (4 if c.kw["H"] <= 4 else 8 if c.kw["H"] <= 8 else 16) == HM)]
        if (op, HM) != ("cait", 8):                                               # (<8> crosses it in tests/make_cait_fixtures.ATTN_CASES: 8 heads, 196 tokens)
            assert any(lds[c.id] > ac.LDS_DEFAULT for c in mine), (op, HM)
        assert any(lds[c.id] <= ac.LDS_DEFAULT for c in mine), (op, HM)
    heads = {c.kw["H"] for c in ac.CAIT_CASES}
    assert {1, 2, 3, 4} <= heads and 5 in heads and {9, 16} <= heads              # <4> with H < HM, <8> with H < HM, <16> at both ends
    for cases in (ac.CAIT_CASES, ac.CONVIT_CASES):
        assert {1, 15, 16, 17, 63, 64, 65} <= {c.kw["T"] for c in cases}
        assert {4, 8, 20, 80} <= {c.kw["dh"] for c in cases} and any(c.kw["F"] == 3 for c in cases)
        assert any(c.kw["T"] % 4 for c in cases) and any(c.kw["T"] % 4 == 0 for c in cases)
    assert {c.kw["kind"] for c in ac.CAIT_CASES} == set(ac.CAIT_KINDS) and {c.kw["kind"] for c in ac.CONVIT_CASES} == set(ac.CONVIT_KINDS)
    for kind in ac.CAIT_KINDS + ac.CONVIT_KINDS:                                  # every kind on a tail-tile shape
        assert any(c.kw["kind"] == kind and c.kw["T"] % 16 for c in ac.ATTN_CASES), kind
    tasks = {c.id: c.kw["H"] * -(-c.kw["dh"] // 16) for c in ac.CAIT_CASES}
    assert (tasks["cait-f1-T17-h2-dh64-dense"], tasks["cait-f1-T17-h2-dh80-dense"]) == (8, 10)
    assert {c.kw["H"] for c in ac.CONVIT_CASES} >= {1, 3}
    assert all(a in ATTN and b in ATTN for a, b in ac.IDENTITY_PAIRS + ac.C1Z_PAIRS) and all(i in ATTN for i in ac.ONE_HEAD)
    assert len(ac.POS_CASES) == len(ac.JOIN_CASES) == 12


@pytest.mark.parametrize("case", ac.ATTN_CASES, ids=[c.id for c in ac.ATTN_CASES])
def test_the_kinds_are_what_they_claim(case):
    """Conditions on the inputs, not measurements of a kernel."""
    kw, inp = case.kw, ac.inputs(case)
    assert all(bool(torch.isfinite(t).all()) for t in inp.values())
    a = ac.logits(case)
    top = a.amax(-1)
    kind = kw["kind"]
    if kind == "huge":                       # float32 exp overflows at 88.7 and underflows to zero below -103.3
        assert bool((top[:, :, 0::2] > 100).all()) and bool((top[:, :, 1::2] < -100).all())
        assert float((top - a.amin(-1)).min()) > 1 and float((top - a.amin(-1)).max()) < 40          # rows that are neither equal nor one-hot
    elif kind == "spike":
        second = a.sort(-1).values[..., -2]
        assert float((top - second).min()) > 104 and 0 < float(top.min()) and float(a.max()) < 88     # one-hot; no row overflows or vanishes without the max
        assert bool((a.argmax(-1)[:, :, 0::2] == kw["T"] - 1).all()) and bool((a.argmax(-1)[:, :, 1::2] == 0).all())
        ref = ac.evaluate(case)              # (asserts that what float64 leaves of dq and dk is below the smallest float32)
        assert not bool(ref["dq"][1].any()) and not bool(ref["dk"][1].any()) and bool(ac.zero_ds_planes(case).all())
    elif kind == "equal":
        assert float((top - a.amin(-1)).max()) == 0
        want = ac.reference(case)
        assert torch.equal(want["probs"][1], torch.full_like(want["probs"][1], 1.0 / kw["T"])) and not bool(want["dk"][1].any())
    elif kind == "bl-large":
        assert float(inp["bl"].abs().max()) > 50
    else:
        assert float(a.abs().max()) < 30
    if case.op == "cait":
        ident = all(torch.equal(inp[n], torch.eye(kw["H"])) for n in ("wl", "ww")) and not bool(inp["bl"].any()) and not bool(inp["bw"].any())
        assert ident == (kind == "identity")
        if kind in ("dense", "bl-large") and kw["T"] > 1 and kw["H"] > 1:
            p, ww, bw = ac.reference(case)["probs"][1], inp["ww"].double(), inp["bw"].double()
            pm = torch.einsum("gh,fhij->fgij", ww, p) + bw.view(1, -1, 1, 1)
            assert float(pm.min()) < 0 and bool((inp["wl"] < 0).any())                               # P' leaves [0, 1]
    else:
        assert ("c" in inp) == (kind != "ungated")
        if kind == "c0":
            assert float(inp["c"][ac.c0_head(kw)]) == 0 and int((inp["c"] == 0).sum()) == 1
            assert not bool(ac.reference(case)["dq"][1][:, ac.c0_head(kw)].any())
        if kind == "c1z":
            assert bool((inp["c"] == 1).all()) and not bool(inp["table"].any())
        if kind == "zrows":
            assert not bool(inp["table"][:, 0].any()) and bool(inp["table"][:, 1].all())
    if kw["T"] == 1:
        want = ac.reference(case)
        assert bool((want["probs"][1] == 1).all()) and not bool(want["dq"][1].any()) and not bool(want["dk"][1].any())


def test_the_fixture_covers_the_table_and_three_cases_recompute():
    assert set(E32) == set(ATTN)
    assert all(tuple(v) == ac.VALUE_OUTPUTS for v in E32.values())
    ids = ("cait-f1-T17-h2-dh8-huge", "convit-f1-T65-h3-dh20-gated", "cait-f2-T33-h5-dh12-dense")
    assert compute(ids) == {i: E32[i] for i in ids}
    hot = _ids(lambda c: c.kw["kind"] in ("huge", "bl-large"))
    assert all(e < 4e-6 for k, v in E32.items() if k not in hot for e in v.values())
    assert 1e-5 < max(e for k in hot for e in E32[k].values()) < 1e-4                             # no bound is vacuous: the widest is 4e-4
    with pytest.raises(KeyError):
        E32["cait-f1-T18-h2-dh8-dense"]


# ---- the table on the host twins ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ac.CASES, ids=[c.id for c in ac.CASES])
def test_case_on_the_host_simulation(eng, case):
    first = ac.run(eng, case)
    errs = ac.check(case, first, E32[case.id] if case.op in ("cait", "convit") else {}, report=print)
    diff = _same(first, ac.run(eng, case))
    assert not diff, f"{case.id}: a second run changed {diff}"
    assert errs is not None
    # the reference passes its own check, and one float past the tail does not
    ac.check(case, ac.as_got(ac.reference(case)), E32.get(case.id, {}))
    spoilt = ac.as_got(ac.reference(case))
    name = next(n for n in spoilt if n.endswith("_slack"))
    spoilt[name][-1] = 0.0
    with pytest.raises(AssertionError):
        ac.check(case, spoilt, E32.get(case.id, {}))


@pytest.mark.parametrize("cid", ac.FRAME_INVARIANCE)
def test_frame_0_has_the_bits_of_a_one_frame_call(eng, cid):
    case = ac.BY_ID[cid]
    whole, alone = ac.run(eng, case), ac.run(eng, case, frames=1)
    for name in ac.VALUE_OUTPUTS:
        assert alone[name].shape[0] == 1 and ac.same_bits(alone[name][0], whole[name][0]), (cid, name)
    assert all(bool((v == ac.SENTINEL).all()) for k, v in alone.items() if k.endswith("_slack"))


@pytest.mark.parametrize("cid", ac.ONE_HEAD)
def test_one_head_of_a_convit_call_is_the_one_head_call(eng, cid):
    case = ac.BY_ID[cid]
    whole = ac.run(eng, case)
    for h in range(case.kw["H"]):
        alone = ac.run(eng, case, head=h)
        for name in ac.VALUE_OUTPUTS:
            assert ac.same_bits(alone[name][:, 0], whole[name][:, h]), (cid, h, name)


@pytest.mark.parametrize("a,b", ac.IDENTITY_PAIRS)
def test_cait_identity_equals_ungated_convit(eng, a, b):
    """Values (torch.equal: a mix with weights 1 and 0 may turn -0 into +0)."""
    ca, cb = ac.run(eng, ac.BY_ID[a]), ac.run(eng, ac.BY_ID[b])
    assert all(torch.equal(ca[n], cb[n]) for n in ac.VALUE_OUTPUTS), [n for n in ac.VALUE_OUTPUTS if not torch.equal(ca[n], cb[n])]


@pytest.mark.parametrize("a,b", ac.C1Z_PAIRS)
def test_c_1_with_a_zero_table_has_the_bits_of_the_ungated_call(eng, a, b):
    ca, cb = ac.run(eng, ac.BY_ID[a]), ac.run(eng, ac.BY_ID[b])
    assert all(ac.same_bits(ca[n], cb[n]) for n in ac.VALUE_OUTPUTS)


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
def test_small_launch_refusals_name_their_launch_and_the_engine_goes_on(eng):
    thunks, untouched, keep = ac.small_refusals(eng)
    assert len(thunks) >= 40
    for label, name, thunk in thunks:
        assert thunk() != 0, (name, label)
        text = eng.capi.i2v_last_error().decode()
        assert text.startswith(name + ":") and "hipErrorInvalidValue" in text, (label, text)
    assert untouched()
    del keep
    for cid in ("pos-f3-T3-C68", "join-f3-T3-C68"):
        ac.check(ac.BY_ID[cid], ac.run(eng, ac.BY_ID[cid]), {})


@pytest.mark.parametrize("op,H,served,refused", [("cait", 16, 144, 145), ("cait", 9, 272, 273), ("convit", 1, 2544, 2545)])
def test_lds_refusal_boundary(eng, op, H, served, refused):
    """H (Tp + 4) <= 2560 floats per LDS row set is served (CaiT; ConViT: Tp + 4 <= 2560), one tile more is refused by both entries
    with the reason, nothing is written, and the engine goes on."""
    fwd, bwd, touched = ac.boundary_calls(eng, op, served, H)
    assert (fwd, bwd) == (0, 0) and set(touched) == {"probs", "out", "dS", "dqkv"}
    rows = (H if op == "cait" else 1) * ((served + 15) // 16 * 16 + 4)
    assert rows <= 2560 < rows + (H if op == "cait" else 1) * 16
    fwd, bwd, touched = ac.boundary_calls(eng, op, refused, H)
    assert fwd != 0 and bwd != 0 and touched == []
    text = eng.capi.i2v_last_error().decode()
    assert text.startswith(op + "_attention_bwd:") and "hipErrorInvalidValue" in text and "LDS budget" in text, text
    cid = "cait-f1-T17-h2-dh8-dense" if op == "cait" else "convit-f1-T17-h2-dh8-gated"
    ac.check(ac.BY_ID[cid], ac.run(eng, ac.BY_ID[cid]), E32[cid])


# ---- sensitivity: the table must bite -----------------------------------------------------------------------------------------------
def _softmax(a, no_max=False, drop_last=False):
    if no_max:                                   # exp without the max subtraction, in float32: its values, under the softmax's own gradient
        e = torch.exp(a.detach().float())
        p = a.softmax(-1)
        return p + ((e / e.sum(-1, keepdim=True)).to(a.dtype) - p.detach())
    if drop_last and a.shape[-1] > 1:            # the last key left out of the row sum
        e = torch.exp(a - a.amax(-1, keepdim=True))
        return e / e[..., :-1].sum(-1, keepdim=True)
    return a.softmax(-1)


def _cait(no_max=False, drop_last=False, wl_t=False, no_bw=False):
    """A local copy of cait_reference.talking_heads with switches."""
    lin = torch.nn.functional.linear

    def attention(qkv, heads, scale, wl, bl, ww, bw):
        n, T, C3 = qkv.shape
        dh = C3 // (3 * heads)
        q, k, v = qkv.reshape(n, T, 3, heads, dh).permute(2, 0, 3, 1, 4)
        a = (q * scale) @ k.transpose(-2, -1)
        a = lin(a.permute(0, 2, 3, 1), wl.t() if wl_t else wl, bl).permute(0, 3, 1, 2)
        p = _softmax(a, no_max, drop_last)
        a = lin(p.permute(0, 2, 3, 1), ww, None if no_bw else bw).permute(0, 3, 1, 2)
        return (a @ v).transpose(1, 2).reshape(n, T, heads * dh), p
    return attention


def _convit(no_max=False, drop_last=False, next_head=False, c_not_in_ds=False):
    """A local copy of convit_reference.blend_attention with switches."""
    def attention(qkv, heads, scale, c=None, table=None):
        n, T, C3 = qkv.shape
        dh = C3 // (3 * heads)
        q, k, v = qkv.reshape(n, T, 3, heads, dh).permute(2, 0, 3, 1, 4)
        p = _softmax((q * scale) @ k.transpose(-2, -1), no_max, drop_last)
        if table is None:
            a = p
        else:
            tb = torch.roll(table, -1, 0) if next_head else table                # head h reads the table of head (h + 1) % heads
            cp = c.view(1, -1, 1, 1) * p
            a = (cp.detach() + (p - p.detach()) if c_not_in_ds else cp) + tb.unsqueeze(0)
        return (a @ v).transpose(1, 2).reshape(n, T, heads * dh), p
    return attention


def _evaluate(case, switch):
    """What a kernel with the slip `switch` would return for the case, as float32 tensors by name."""
    kw = case.kw
    if switch == "copied_last_row":              # the last row of the last tile copied from the one before it
        got = ac.as_got(ac.reference(case))
        if kw["T"] > 1:
            for name in ("probs", "out", "dq"):
                got[name][:, :, -1] = got[name][:, :, -2]
        return got
    if switch == "no_scale_on_dk":
        got = ac.as_got(ac.reference(case))
        got["dk"] = got["dk"] * kw["dh"] ** 0.5
        return got
    cait_sw = {k: True for k in (switch,) if k in ("no_max", "drop_last", "wl_t", "no_bw")}
    convit_sw = {k: True for k in (switch,) if k in ("no_max", "drop_last", "next_head", "c_not_in_ds")}
    return ac.as_got(ac.evaluate(case, cait=_cait(**cait_sw), convit=_convit(**convit_sw)))


def test_the_local_copies_without_a_switch_are_the_references():
    for case in ac.ATTN_CASES:
        ref, mine = ac.reference(case), ac.evaluate(case, cait=_cait(), convit=_convit())
        assert all(torch.equal(ref[n][1], mine[n][1]) for n in ref), case.id


def _overflows(c):
    """float32 exp without the max subtraction leaves its range: a logit above 88.7 is inf, a row wholly below -103.3 sums to zero."""
    a = ac.logits(c)
    return float(a.max()) > 88.7 or float(a.amax(-1).min()) < -103.3


_gated = lambda c: c.op == "convit" and c.kw["kind"] != "ungated"      # noqa: E731
_zero_ds = lambda c: bool(ac.zero_ds_planes(c).all())                  # noqa: E731
# switch -> the cases that must fail; every other case must still pass.  Where a listed class has members that provably cannot see the
# slip, they are taken out here, with the reason:
#   no_max           the `huge` cases, and `bl-large`, whose bias of -104 puts whole rows below exp's range the same way (`_overflows`;
#                    the `spike` cases are built inside exp's range and must NOT fail: they test the one-hot row, not the max)
#   wl_t             not `spike`: P is one-hot whichever way a positive mix goes, so out and dv do not move and dq = dk = 0
#   next_head        not `c1z`: its table is zero in every head
#   c_not_in_ds      not where dS is exactly zero (`spike`, T = 1): c times zero
#   no_scale_on_dk   dk != 0: not T = 1, `spike`, `equal` (q = 0)
MUST_FAIL = {
    "no_max": _ids(_overflows),
    "drop_last": _ids(lambda c: c.kw["T"] > 1),
    "copied_last_row": _ids(lambda c: c.kw["T"] > 1),
    "wl_t": _ids(lambda c: c.op == "cait" and c.kw["kind"] not in ("identity", "spike") and c.kw["H"] > 1),
    "no_bw": _ids(lambda c: c.op == "cait" and c.kw["kind"] != "identity"),
    "next_head": _ids(lambda c: _gated(c) and c.kw["H"] > 1 and c.kw["kind"] != "c1z"),
    "c_not_in_ds": _ids(lambda c: _gated(c) and c.kw["kind"] != "c1z" and not _zero_ds(c)),
    "no_scale_on_dk": _ids(lambda c: not _zero_ds(c) and c.kw["kind"] != "equal"),
}


def test_the_must_fail_lists_are_the_issues():
    huge = _ids(lambda c: c.kw["kind"] == "huge")
    assert huge and huge <= MUST_FAIL["no_max"] and MUST_FAIL["no_max"] - huge == {"cait-f1-T17-h2-dh8-bl-large"}
    assert not MUST_FAIL["no_max"] & _ids(lambda c: c.kw["kind"] == "spike")
    assert all(v and v < set(ATTN) for v in MUST_FAIL.values())
    assert MUST_FAIL["no_scale_on_dk"] == _ids(lambda c: bool(ac.reference(c)["dk"][1].any()))
    assert MUST_FAIL["no_bw"] == _ids(lambda c: c.op == "cait" and bool(ac.inputs(c)["bw"].any()))
    assert MUST_FAIL["c_not_in_ds"] | _ids(lambda c: _gated(c) and _zero_ds(c)) == _ids(lambda c: _gated(c) and bool((ac.inputs(c)["c"] != 1).any()))


@pytest.mark.parametrize("switch", sorted(MUST_FAIL))
def test_a_wrong_reference_fails_exactly_its_cases(switch):
    must_fail = MUST_FAIL[switch]
    failed = []
    for case in ac.ATTN_CASES:
        try:
            ac.check(case, _evaluate(case, switch), E32[case.id])
        except AssertionError:
            failed.append(case.id)
    assert must_fail <= set(failed), (switch, "passed but must fail", sorted(must_fail - set(failed)))
    assert set(failed) <= must_fail, (switch, "failed but cannot see it", sorted(set(failed) - must_fail))


def test_one_wrong_key_in_one_row_is_not_averaged_away():
    """The last key of the last row of one head, off by 1e-5 of the plane's largest probability: the whole-tensor relative L2 of the
    earlier attention tests (bound 1e-6 at best) sees 4e-7; the per-slice measure fails it, and fails `probs` alone."""
    case = ATTN["cait-f1-T144-h16-dh4-dense"]
    want = ac.reference(case)["probs"][1]
    got = ac.as_got(ac.reference(case))
    got["probs"][0, 7, -1, -1] += 1e-5 * float(want[0, 7].max())
    assert float((got["probs"].double() - want).norm() / want.norm()) < 1e-6
    errs = {n: ac.error(got[n], ac.reference(case)[n][1]) for n in ac.VALUE_OUTPUTS}
    assert errs["probs"] > 5e-6 and max(errs[n] for n in ("out", "dq", "dk", "dv")) < 1e-7
    with pytest.raises(AssertionError, match="probs error"):
        ac.check(case, got, E32[case.id])
