"""GPU (-m gpu): the talking-heads / gated positional attention case table (tests/attn_edge_cases.py) through the C entries on the gfx950
kernels of csrc/i2v_cait.hip and csrc/i2v_convit.hip -- cait_attention(_bwd), convit_attention(_bwd), cait_add_pos and
convit_join_cls(_bwd).  Per case:

  * the device against the float64 reference, every output at its bound (attn_edge_cases.check: probs, out, dq, dk and dv each on its
    own, the error taken per slice and normalised by the slice's (frame, head) plane, held to max(2e-6, 4 e32) with e32 from
    tests/golden/attn_edge_fp32_cpu_errors.json; planes whose reference is exactly zero exactly zero; the three small launches, the
    slack around every output and the pad columns T .. ld of probs, dS and Pm bit for bit);
  * a second run of the same case gives the same bits;
  * the launch counter moves by 1 for the forward and by 2 for the backward.

Frame 0 of an F-frame call has the bits of a 1-frame call; one head of an H-head ConViT call has the bits of the 1-head call on its
columns; CaiT with identity mixes and zero biases equals the ungated ConViT call in value; c = 1 with a zero table has the bits of the
ungated call; every refusal names its launch and launches nothing, and an ordinary case runs after them.

NOT YET MEASURED ON A DEVICE.  This module was written and run on the host twins only (tests/test_attn_edge_cpu.py runs the same
table, the same checks and the same exact relations there); no MI355X could be reached while it was written, so there is no table of
device error against bound here yet, no running time, and the CaiT-identity / ungated-ConViT equality is read from the code and seen
on the host twins, not on the device.  Every case prints its errors next to its bounds (pytest -s): whoever runs it first puts the
table here and the worst ratio into DESIGN.md section 36.  The bounds per case and output are max(2e-6, 4 e32) of the committed
fixture: 2e-6 to 1.6e-5 outside the `huge` and `bl-large` kinds, up to 1.6e-4 (dk of cait-f2-T33-h5-dh12-huge) inside them.
"""
import pytest
import torch

from i2v_amd import attacks
from tests import attn_edge_cases as ac
from tests.family_harness import stat
from tests.make_attn_edge_fixtures import load

pytestmark = pytest.mark.gpu

E32 = load()
COUNTER = {"cait": b"cait_attention_launches", "convit": b"convit_attention_launches"}


@pytest.fixture(scope="module")
def eng():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    e = attacks.get_engine("cuda:0")
    assert e.capi.i2v_backend() == b"hip:gfx950"
    return e


def _same(a, b):
    assert a.keys() == b.keys()
    return [n for n in a if not ac.same_bits(a[n], b[n])]


def _counters(eng):
    return {op: stat(eng, name) for op, name in COUNTER.items()}


@pytest.mark.parametrize("case", ac.CASES, ids=[c.id for c in ac.CASES])
def test_case_on_the_device(eng, case):
    attn = case.op in COUNTER
    before = _counters(eng)
    first = ac.run(eng, case)
    after = _counters(eng)
    assert {op: after[op] - before[op] for op in COUNTER} == {op: 3 if op == case.op else 0 for op in COUNTER}      # 1 forward + 2 backward
    second = ac.run(eng, case)
    errs = ac.check(case, first, E32[case.id] if attn else {}, report=print)
    diff = _same(first, second)
    assert not diff, f"{case.id}: a second run changed {diff}"
    assert errs is not None


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
    """Read from the code both are the same fma chains and the same butterfly: a head mix with weights 1 and 0 and a zero bias returns its
    operand (fma(0, x, acc) = acc, fma(1, x, 0) = x, x + 0 = x; -0 may become +0, hence values, not bits)."""
    ca, cb = ac.run(eng, ac.BY_ID[a]), ac.run(eng, ac.BY_ID[b])
    diff = [n for n in ac.VALUE_OUTPUTS if not torch.equal(ca[n], cb[n])]
    assert not diff, (a, diff, {n: float((ca[n] - cb[n]).abs().max()) for n in diff})


@pytest.mark.parametrize("a,b", ac.C1Z_PAIRS)
def test_c_1_with_a_zero_table_has_the_bits_of_the_ungated_call(eng, a, b):
    ca, cb = ac.run(eng, ac.BY_ID[a]), ac.run(eng, ac.BY_ID[b])
    diff = [n for n in ac.VALUE_OUTPUTS if not ac.same_bits(ca[n], cb[n])]
    assert not diff, (a, diff)


def test_refusals_name_their_launch_and_the_engine_goes_on(eng):
    thunks, untouched, keep = ac.small_refusals(eng)
    assert len(thunks) >= 40
    before = _counters(eng)
    for label, name, thunk in thunks:
        assert thunk() != 0, (name, label)
        text = eng.capi.i2v_last_error().decode()
        assert text.startswith(name + ":") and "hipErrorInvalidValue" in text, (label, text)
    assert untouched()
    del keep
    for op, H, refused in (("cait", 16, 145), ("cait", 9, 273), ("convit", 1, 2545)):          # one tile past the LDS budget
        fwd, bwd, touched = ac.boundary_calls(eng, op, refused, H)
        assert fwd != 0 and bwd != 0 and touched == [], (op, H, refused)
        assert "LDS budget" in eng.capi.i2v_last_error().decode()
    assert _counters(eng) == before                                                            # nothing was launched
    for cid in ("pos-f3-T3-C68", "join-f3-T3-C68", "cait-f1-T17-h2-dh8-dense", "convit-f1-T17-h2-dh8-gated"):
        ac.check(ac.BY_ID[cid], ac.run(eng, ac.BY_ID[cid]), E32.get(cid, {}))
