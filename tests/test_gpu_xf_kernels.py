"""GPU (-m gpu): the shared-launch case table (tests/xf_cases.py) through the C entries on the gfx950 kernels of csrc/i2v_vit.hip --
vit_gemm, vit_layernorm(_bwd), vit_softmax(_bwd), vit_patchify and vit_assemble, which ViT / DeiT, Swin, ConvNeXt, MLP-Mixer / ResMLP,
CaiT, ConViT and XCiT all run on.  Per case:

  * the device against the float64 reference, every output at its bound (xf_cases.check: max(2e-6, 4 e32) of the output's largest
    element, e32 from tests/golden/xf_fp32_cpu_errors.json; exact outputs -- patchify, the prefix rows of assemble under zero pos
    rows, the slack around every output, the uniform softmax row -- bit for bit);
  * a second run of the same case gives the same bits.

Batch b of a batched GEMM on its own has the bits it has inside the batched launch (xf_cases.INVARIANCE).  Every refusal of the GEMM,
softmax and embed entries is made once, names its launch and launches nothing; an ordinary case runs after them.  Device and host
simulation are not compared bit for bit: csrc/i2v_xf_host.h sums in another order on purpose.

Measured on an MI355X: 282 tests in 2.9 s; the slowest is the first case (0.24 s with its setup: it opens the engine), every other
test takes <= 0.02 s.  Worst device error per launch and output, normalised as its bound is, next to the bound it was held to and the
e32 behind it:

    launch    output    error     bound     e32       case
    gemm      C         2.34e-07  2e-06     2.34e-07  gemm-K48-Am-Bk-scalar
    gemm      C2        1.98e-07  2e-06     1.98e-07  gemm-stem-linear-K27
    ln        out       9.73e-04  3.89e-03  9.73e-04  ln-r3-C3-mean100
    ln        mean      1.48e-07  2e-06     4.34e-08  ln-r3-C63-none
    ln        rstd      1.72e-06  6.88e-06  1.72e-06  ln-r3-C3-mean100
    ln        dx        3.99e-03  1.6e-02   3.99e-03  ln-r3-C3-mean100
    softmax   P         1.05e-07  2e-06     1.05e-07  softmax-N197-ld200-r1-big
    softmax   dX        4.53e-07  2e-06     4.53e-07  softmax-N2-ld4-r3-big
    attn      probs     2.84e-07  2e-06     2.37e-07  attn-f1-T129-h1-dh8
    attn      out       6.16e-07  2.46e-06  6.16e-07  attn-f1-T130-h2-dh6
    attn      dprobs    2.78e-07  2e-06     2.78e-07  attn-f1-T129-h1-dh8
    attn      dqkv      2.83e-07  2e-06     2.72e-07  attn-f1-T130-h2-dh6
    embed     emb       6.32e-07  2e-06     4.65e-07  embed-p16-c3-g3-pre1-acc1
    embed     tokens    6.56e-07  2e-06     4.77e-07  embed-p16-c3-g3-pre1-acc1
    embed     dpatches  3.09e-07  2e-06     3.09e-07  embed-p8-c1-g3-pre1-acc0
    embed     gimg      3.09e-07  2e-06     3.09e-07  embed-p8-c1-g3-pre1-acc0

12 of the 517 bounded outputs have a bound wider than the floor: the `out`, `dx` and one `rstd` of the four mean-100 LayerNorm rows
(a float32 mean of values near 100 is off by up to an ulp of 100, 7.6e-6, which is 8e-4 of a spread of 0.01; float32 torch and the
device lose the same digits: 4 e32 = 4.3e-4 .. 1.6e-2 against device errors 1.2e-5 .. 4.0e-3; over the order-one rows the
device is within 1.4e-07 for out, 3.4e-07 for dx and 1.2e-07 for rstd), two embed outputs and one attention
output at 2.5e-06 .. 2.6e-06 (device 6.2e-07 .. 6.5e-07).  No device error exceeds 0.41 of its bound: the table found no fault in
the kernels.  The errors are printed (pytest -s).
"""
import pytest
import torch

from i2v_amd import attacks
from tests import xf_cases as xc
from tests.make_xf_fixtures import load

pytestmark = pytest.mark.gpu

E32 = load()


@pytest.fixture(scope="module")
def eng():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    e = attacks.get_engine("cuda:0")
    assert e.capi.i2v_backend() == b"hip:gfx950"
    return e


@pytest.mark.parametrize("case", xc.CASES, ids=[c.id for c in xc.CASES])
def test_xf_case_on_the_device(eng, case):
    first = xc.run(eng, case)
    second = xc.run(eng, case)
    errs = xc.check(case, first, E32[case.id], report=print)
    assert first.keys() == second.keys()
    diff = [n for n in first if not xc.same_bits(first[n], second[n])]
    assert not diff, f"{case.id}: a second run changed {diff}"
    assert errs is not None


@pytest.mark.parametrize("cid", xc.INVARIANCE)
def test_a_batch_alone_has_its_bits_in_the_batched_launch(eng, cid):
    case = xc.BY_ID[cid]
    whole = xc.run(eng, case)
    for b in range(whole["C"].shape[0]):
        alone = xc.run_batch_alone(eng, case, b)
        assert xc.same_bits(alone["C"], whole["C"][b]), (cid, b, float((alone["C"] - whole["C"][b]).abs().max()))
        assert bool((alone["C_slack"] == xc.SENTINEL).all())


def test_refusals_name_their_launch_and_the_engine_goes_on(eng):
    thunks, untouched, keep = xc.gemm_refusals(eng)
    more, keep2 = xc.device_refusals(eng)
    for label, name, thunk in thunks + more:
        assert thunk() != 0, label
        text = eng.capi.i2v_last_error().decode()
        assert text.startswith(name + ":"), (label, text)
    torch.cuda.synchronize()
    assert untouched()
    del keep, keep2
    for cid in ("gemm-flags-all-set", "softmax-N263-one-all-kinds"):
        xc.check(xc.BY_ID[cid], xc.run(eng, xc.BY_ID[cid]), E32[cid])
