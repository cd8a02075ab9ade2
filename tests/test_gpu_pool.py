"""GPU (-m gpu): the pooling case table (tests/pool_cases.py) on the gfx950 kernels.  Plans are made without the autotuner, so they
are deterministic.  Per case:

  * the device against the host simulation of the same planned net, BIT FOR BIT: every node's activation and the input gradient.
    The scalar twins have no bands and no float4 path, so this is what catches a band-edge or alignment error (the banded cases
    put every 2-D max-pool instantiation over more than one LDS band, with windows that straddle two); it is immune to near-ties;
  * the device against the float64 autograd reference at the bounds of tests/test_pool_cpu.py;
  * a second pass over the same net gives the same bits.

The measured errors are printed (pytest -s).  On an MI355X, device against float64 (max |pooled error|, max feature error /
max|ref|, max gradient error / max|ref|), every case bit-identical to the host simulation:

    case                           pooled    feature   gradient
    patch321-random                1.35e-06  4.41e-07  2.15e-07
    patch321-exact-relu            0         3.61e-07  1.55e-07
    patch321-exact-linear          0         3.6e-07   1.55e-07
    g321_vec-random                1.56e-06  3.11e-07  1.64e-07
    g321_vec-exact-relu            0         4.35e-07  1.38e-07
    g321_scalar-random             1.44e-06  4.15e-07  1.83e-07
    p220-random                    1.92e-06  2.98e-07  1.84e-07
    p220-exact-linear              0         2.92e-07  1.72e-07
    p320_ceil_1001-random          8.39e-07  4.85e-07  2e-07
    p320_ceil_1001-exact-relu      0         4.5e-07   1.76e-07
    p320_ceil_1000-random          1.45e-06  4.87e-07  2.08e-07
    p320_ceil_1000-exact-linear    0         3.69e-07  1.81e-07
    gen_k3s1-exact-relu            0         4.45e-07  1.68e-07
    gen_k3s1-exact-linear          0         4.45e-07  1.73e-07
    gen_k5s3-random                1.09e-06  3.58e-07  1.67e-07
    s321_13x11-exact-relu          0         2.85e-07  1.75e-07
    s321_13x11-exact-linear        0         2.85e-07  1.62e-07
    s321_12x16-exact-relu          0         1.78e-07  1.42e-07
    s321_12x16-exact-linear        0         1.99e-07  1.43e-07
    s320_ceil_13x11-exact-relu     0         1.78e-07  1.02e-07
    s320_ceil_13x11-exact-linear   0         1.78e-07  1.02e-07
    s220_ceil_13x11-exact-relu     0         1.75e-07  1.43e-07
    s220_ceil_13x11-exact-linear   0         1.09e-07  1.95e-07
    s311_9x12-exact-relu           0         2.38e-07  1.22e-07
    s311_9x12-exact-linear         0         2.38e-07  1.59e-07
    v33_22_11                      6.59e-07  2.2e-07   1.59e-07
    v21_21_00                      1.1e-06   2.15e-07  2.33e-07
    v31_11_10                      5.69e-07  4.45e-07  2.47e-07
    v23_12_01                      7.88e-07  3.54e-07  1.98e-07
    v32_22_10                      1.21e-06  2.55e-07  1.61e-07
    v33_11_11-stride-exact         0         3.32e-07  2.05e-07
    a22_13x11                      3.17e-07  1.97e-07  4.13e-07
    a23_13x11                      1.8e-07   2.29e-07  1.44e-07
    a33_14x16                      1.23e-07  1.86e-07  2.74e-07
    a22_relu                       2.33e-07  2.25e-07  1.59e-07
    a32_13x11                      1.86e-07  2.91e-07  4.02e-07
    a22_stride                     3.16e-07  5.52e-07  5.07e-07
"""
import pytest
import torch

from i2v_amd import attacks
from tests import pool_cases as pc
from tests.test_gpu_parity import dev, write_hook_grads

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    e = attacks.get_engine("cuda:0")
    assert e.capi.i2v_backend() == b"hip:gfx950"
    return e


def _host(case, **kw):
    from tests.hostsim_util import hostsim_engine
    from tests.test_planner_hostsim import write_hook_grads as write_cpu
    return pc.run(hostsim_engine(), case, lambda t: t.contiguous(), write_cpu, **kw)


def _same_bits(tag, a, b):
    (acts_a, gx_a), (acts_b, gx_b) = a, b
    assert acts_a.keys() == acts_b.keys()
    for t in acts_a:
        d = acts_a[t] != acts_b[t]
        assert not bool(d.any()), f"{tag}: tensor {t} differs at {int(d.sum())} elements, first at {[int(v) for v in d.nonzero()[0]]}"
    d = ~((gx_a == gx_b) | (torch.isnan(gx_a) & torch.isnan(gx_b)))
    assert not bool(d.any()), f"{tag}: input gradient differs at {int(d.sum())} elements, first at {[int(v) for v in d.nonzero()[0]]}"


@pytest.mark.parametrize("case", pc.CASES, ids=[c.id for c in pc.CASES])
def test_pool_case_on_the_device(eng, monkeypatch, case):
    monkeypatch.setenv("I2V_AUTOTUNE", "0")
    first, second = pc.run(eng, case, dev, write_hook_grads, passes=2)
    torch.cuda.synchronize()
    host, = _host(case)
    built, ref = pc.build(case), pc.reference(case)
    print(case.id, "device vs float64: pooled %.3g  feature %.3g  gradient %.3g" % pc.errors(case, built, *first, ref))
    _same_bits(case.id + " device vs host simulation", first, host)
    _same_bits(case.id + " second pass", second, first)
    pc.check(case, built, *first, ref)


def test_fewer_frames_than_planned(eng, monkeypatch):
    """Planned for 4 frames, run with 2: the bits of a net planned for 2 (and of the host simulation planned for 4)."""
    monkeypatch.setenv("I2V_AUTOTUNE", "0")
    case = pc.FEWER_FRAMES
    four, = pc.run(eng, case, dev, write_hook_grads, planned=4)
    two, = pc.run(eng, case, dev, write_hook_grads)
    _same_bits("planned for 4 vs planned for 2", four, two)
    _same_bits("planned for 4, device vs host simulation", four, _host(case, planned=4)[0])
    pc.check(case, pc.build(case), *four, pc.reference(case))


def test_too_wide_a_row_is_refused_and_the_engine_goes_on(eng, monkeypatch):
    """3/2/1 on a 6 x 1400 plane: 4096 // 1400 = 2 rows < k fit the forward LDS band.  The launch code refuses on the host before
    anything is launched; the refusal reaches Python as a RuntimeError with its text, and a net built afterwards on the same engine
    computes what it should."""
    monkeypatch.setenv("I2V_AUTOTUNE", "0")
    with pytest.raises(RuntimeError, match=pc.REFUSAL_TEXT):
        pc.run(eng, pc.REFUSED, dev, write_hook_grads)
    torch.cuda.synchronize()
    case = pc.BY_ID["s321_13x11-exact-relu"]
    after, = pc.run(eng, case, dev, write_hook_grads)
    _same_bits("after the refusal, device vs host simulation", after, _host(case)[0])
    pc.check(case, pc.build(case), *after, pc.reference(case))
