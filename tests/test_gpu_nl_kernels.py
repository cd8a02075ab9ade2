"""GPU (-m gpu): the non-local-block case table (tests/nl_cases.py) through the C entries of include/i2v_nl_launch.h on the gfx950
kernels of csrc/i2v_kernels.hip -- attn_gemm_kernel<1|2|3>, attn_split_reduce_kernel, softmax_rows_kernel and addmask_kernel.  Per case:

  * the device against the float64 reference, every output at its bound (nl_cases.check: max(2e-6, 4 e32) of the output's largest
    element, e32 from tests/golden/nl_fp32_cpu_errors.json; exact outputs -- addmask, the slack around every output, the inputs after
    the launch, the uniform and the N = 1 softmax rows, the empty-segment identity -- bit for bit);
  * a second run of the same case gives the same bits;
  * the device against the host simulation, BIT FOR BIT: every product case (one k-ordered fmaf chain per element, K-split segments
    added in order), the softmax backward and addmask.  The softmax cases are flagged `host_bits=False` for their forward output P
    alone (the device's expf and glibc's round differently); their dS and slack are held to the host's bits all the same.

Clip b of a 3-clip launch has the bits of that clip launched alone (nl_cases.INVARIANCE: forms 1, 2, 3 and a split launch).  Every
refusal of the three entries is made once on the device library, names its entry and writes nothing; an ordinary case runs after them.

Measured on an MI355X: 307 tests in 3.1 s; the slowest are the first case (0.24 s with its setup: it opens the engine),
addmask-second-pass-bits (0.14 s: a million elements) and the first case of form 3 (0.12 s); every other test takes <= 0.01 s.  276 of
the 300 cases have the host simulation's bits in every output; 24 softmax cases
differ from it in P alone (flagged, see above; the other 14 -- the uniform rows and N <= 2 -- agree there
too).  Worst device error per launch and output, normalised as its bound is, next to the bound it was held to and the e32 behind it:

    launch    output  error     bound     e32       case
    gemm1     D       3.73e-07  2e-06     3.73e-07  gemm1-K96
    gemm2     C       5.2e-07   2e-06     1.1e-07   gemm2-view-A5x49-C3x3
    gemm3     C       4.7e-07   2e-06     4.7e-07   gemm3-split2-K512-planner-smallest
    softmax   P       9.57e-08  2e-06     1.44e-07  softmax-block
    softmax   dS      2.45e-07  2e-06     3.8e-07   softmax-block

One of the 283 bounded outputs has a bound wider than the floor: C of gemm3-split8-K256-whole at 2.05e-06 (float32 torch's own
blocked sum over K = 256 is off by 5.1e-07 there; the device by 1.6e-07).  The saturated softmax rows stay at the floor: the float64
reference subtracts the row maximum from float32 inputs exactly, float32 torch and the device round only differences that exp then
takes to nothing (e32 <= 1.2e-07, device <= 9e-08).  No device error exceeds 0.26 of its bound, and every product, softmax-backward
and addmask output has the host simulation's bits: the table found no fault in the kernels or their twins.  The errors are printed
(pytest -s).
"""
import pytest
import torch

from i2v_amd import attacks
from tests import nl_cases as nc
from tests.make_nl_fixtures import load

pytestmark = pytest.mark.gpu

E32 = load()


@pytest.fixture(scope="module")
def eng():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    e = attacks.get_engine("cuda:0")
    assert e.capi.i2v_backend() == b"hip:gfx950"
    return e


def _differing(a, b):
    return [n for n in a if not nc.same_bits(a[n], b[n])]


@pytest.mark.parametrize("case", nc.CASES, ids=[c.id for c in nc.CASES])
def test_nl_case_on_the_device(eng, case):
    from tests.hostsim_util import hostsim_engine
    first = nc.run(eng, case)
    second = nc.run(eng, case)
    host = nc.run(hostsim_engine(), case)
    assert first.keys() == second.keys() == host.keys()
    errs = nc.check(case, first, E32[case.id], report=print)
    assert not _differing(first, second), f"{case.id}: a second run changed {_differing(first, second)}"
    diff = _differing(first, host)
    print(f"{case.id:44s} device vs host simulation: {'equal bits' if not diff else 'differ in ' + ', '.join(diff)}")
    if not case.host_bits:
        assert case.why_not and case.op == "softmax"
        nc.check(case, host, E32[case.id])
        diff = [n for n in diff if n != "P"]                   # the forward's expf; everything else has the host's bits
    assert not diff, f"{case.id}: device and host simulation differ in {diff}: " + "; ".join(
        f"{n} at {int((first[n] != host[n]).sum())} of {first[n].numel()} element(s), max |difference| {float((first[n].double() - host[n].double()).abs().max()):.3g}"
        for n in diff)
    assert errs is not None


@pytest.mark.parametrize("cid", nc.INVARIANCE)
def test_a_clip_alone_has_its_bits_in_the_batched_launch(eng, cid):
    case = nc.BY_ID[cid]
    whole = nc.run(eng, case)
    name = "D" if case.op == "gemm1" else "C"
    for b in range(whole[name].shape[0]):
        alone = nc.run_clip_alone(eng, case, b)
        assert nc.same_bits(alone[name][0], whole[name][b]), (cid, b, float((alone[name][0] - whole[name][b]).abs().max()))
        assert bool((alone[name + "_slack"] == nc.SENTINEL).all())


def test_refusals_name_their_entry_and_the_engine_goes_on(eng):
    thunks, nothing, untouched, keep = nc.refusals(eng)
    for label, name, thunk in thunks:
        assert thunk() != 0, label
        text = eng.capi.i2v_last_error().decode()
        assert text.startswith(name + ": bad argument"), (label, text)
    for label, thunk in nothing:
        assert thunk() == 0, label
    torch.cuda.synchronize()
    assert untouched()                                          # no launch: every output still has its initial bits
    del keep
    for cid in ("gemm2-split2-K100-accumulate", "softmax-N257-r5-sat-all-kinds", "addmask-two-blocks-bits"):
        nc.check(nc.BY_ID[cid], nc.run(eng, nc.BY_ID[cid]), E32[cid])
