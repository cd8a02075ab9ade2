"""GPU (-m gpu): the loop-kernel case table (tests/loop_cases.py) through the C entries on the gfx950 kernels.  Per case:

  * the device against the float64 reference, every output at its bound (loop_cases.check: max(floor, 4 e32) with e32 from
    tests/golden/loop_fp32_cpu_errors.json; exact outputs -- resample forward, sign, compose, the slack of every gradient view, gated
    elements, momentum == out -- bit for bit);
  * a second run of the same case gives the same bits;
  * the device against the host simulation, BIT FOR BIT, except the cases flagged `host_bits=False` (aens_coeffs: the scalar twin sums
    its fp32 softmax in index order with glibc's expf, the one-wave kernel as an xor butterfly with the device's).

The refusals of tests/test_loop_kernels_cpu.py run once on the device library too: nothing is launched by them.

Measured on an MI355X: 260 tests in 3.2 s; the slowest are gp-1x3x32x224x224 (0.23 s: 4.8 M elements through the float64
reference), the first case (0.17 s: it opens the engine) and tap_sign-n4194309 (0.07 s); every other case takes <= 0.06 s.  257 of
the 259 cases have the host simulation's bits; aens_coeffs-L64 and aens_coeffs-L6-equal-prev differ from it (flagged, see above).
Worst device error per entry and kind, normalised as its bound is, next to the bound it was held to and the e32 behind it:

    entry        kind    error     bound     e32       case, output
    cos          cos     1.19e-07  2e-07     0         cos-D1-pad0-m0a1 cos          (one float32 ulp of cos = 1)
    cos          tensor  2.9e-07   2e-06     3.25e-07  cos-D3-pad1-m1a0 grad
    std          scalar  5.39e-08  1e-05     5.39e-08  std-D5-f3-pad0-m1a0 std
    std          tensor  5.65e-08  2e-06     6.04e-08  std-D8197-f4-pad3-m1a0 grad
    ilaf         scalar  4.64e-08  1e-05     1.11e-07  ilaf-D37-f6-seg2-pad3-m0a0 loss
    ilaf         tensor  1.03e-07  2e-06     4.9e-07   ilaf-D8197-f6-seg3-pad3-m1a0 grad
    tapd         scalar  7.6e-08   1e-05     7.6e-08   tapd-D5-f3-seg1-pad0-m1a0 dist
    tapd         tensor  1.15e-07  2e-06     9.18e-08  tapd-D5-f3-seg1-pad3-m0a0 grad
    head         tensor  3.29e-07  2e-06     2.36e-07  head-s2-bias0-pad1-m0a0 grad2
    head         scalar  1.78e-07  1e-05     1.07e-06  head-s1-bias0-pad3-m1a0 loss_each
    gp           tensor  1.16e-07  2e-06     1.16e-07  gp-2x3x2x150x150-mode0-fm1-mom1 out
    tap_perts    tensor  6.33e-08  2e-06     6.33e-08  tap_perts-2x3x3x5x7 out
    tap_grad     tensor  4.7e-08   2e-06     4.7e-08   tap_grad-2x3x3x5x7 out
    tap_sign     scalar  2.09e-08  1e-05     2.09e-08  tap_sign-n4097 reg
    aens_reduce  tensor  4.42e-08  2e-06     1.05e-07  aens_reduce-L64-f65 weighted
    aens_coeffs  tensor  1.21e-07  2e-06     8.4e-08   aens_coeffs-L64 coeffs
    dwconv       tensor  6.71e-08  2e-06     6.23e-08  dwconv-2x3x3x4x5-axis2-k15 out
    resample     tensor  3.21e-08  2e-06     4.86e-08  resample-5x7-to-7x9 bwd
    ttmix        tensor  2.51e-07  2e-06     2.32e-07  ttmix-D64-w0.0 out

Where 4 e32 exceeds the floor the bound is wider than the floor: most cosines (the float32 reference's own sum; 2.1e-07 .. 1.1e-06
against device errors <= 9.6e-08), a dozen gradients at 2.2e-06 .. 3.8e-06, and three outliers -- head-s1-bias1-pad3-m1a0 grad1 at
1.04e-05 (a two-class softmax that cancels in float32; device 3.3e-08) and cos-D262151 at 1.4e-05 (cos) and 3e-05 (gradient)
(the float32 torch reduction over 262 151 elements; device 2e-08 and 4.3e-08).  No device error exceeds 3.3e-07.
The errors are printed (pytest -s).
"""
import pytest
import torch

from i2v_amd import attacks
from tests import loop_cases as lc
from tests.make_loop_fixtures import load

pytestmark = pytest.mark.gpu

E32 = load()


@pytest.fixture(scope="module")
def eng():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    e = attacks.get_engine("cuda:0")
    assert e.capi.i2v_backend() == b"hip:gfx950"
    return e


def _differing(a, b):
    return [n for n in a if not lc.same_bits(a[n], b[n])]


@pytest.mark.parametrize("case", lc.CASES, ids=[c.id for c in lc.CASES])
def test_loop_case_on_the_device(eng, case):
    from tests.hostsim_util import hostsim_engine
    first = lc.run(eng, case)
    second = lc.run(eng, case)
    host = lc.run(hostsim_engine(), case)
    assert first.keys() == second.keys() == host.keys()
    errs = lc.check(case, first, E32[case.id], report=print)
    assert not _differing(first, second), f"{case.id}: a second run changed {_differing(first, second)}"
    diff = _differing(first, host)
    print(f"{case.id:44s} device vs host simulation: {'equal bits' if not diff else 'differ in ' + ', '.join(diff)}")
    if case.host_bits:
        assert not diff, f"{case.id}: device and host simulation differ in {diff}: " + "; ".join(
            f"{n} at {int((first[n] != host[n]).sum())} of {first[n].numel()} element(s), max |difference| {float((first[n].double() - host[n].double()).abs().max()):.3g}"
            for n in diff)
    else:
        assert case.why_not
        lc.check(case, host, E32[case.id])
    assert errs is not None


def test_refusals_name_their_entry_on_the_device_library(eng):
    thunks, keep = lc.refusals(eng)
    for label, name, thunk in thunks:
        assert thunk() != 0, label
        text = eng.capi.i2v_last_error().decode()
        assert text.startswith(name + ":"), (label, text)
    torch.cuda.synchronize()
    del keep
    case = lc.BY_ID["cos-D37-pad3-off0"]              # the engine goes on after the refusals
    lc.check(case, lc.run(eng, case), E32[case.id])
