"""The pooling case table (tests/pool_cases.py) on the host simulation against the float64 autograd reference: the pooled tensor,
the hooked feature and the input gradient, at the bounds of test_maxpool_geometries.  The scalar twins have no bands and no float4
path: what this file pins is the DEFINITION the device kernels are compared with bit for bit (tests/test_gpu_pool.py) -- the tie
rule, ceil_mode's overhanging windows, the temporal windows, and the average pool's adjoint for every k / stride and a ReLU'd source.

A near-tie that fp32 and fp64 decide differently would move a whole gradient cone; there is no tolerance for that here: the fp32
host simulation meets the bounds for the committed seeds."""
import pytest
import torch

from tests import pool_cases as pc
from tests.hostsim_util import hostsim_engine
from tests.test_planner_hostsim import write_hook_grads


def _run(case, **kw):
    return pc.run(hostsim_engine(), case, lambda t: t.contiguous(), write_hook_grads, **kw)


@pytest.mark.parametrize("case", pc.CASES, ids=[c.id for c in pc.CASES])
def test_pool_case_matches_float64_autograd(case):
    (acts, gx), = _run(case)
    built, ref = pc.build(case), pc.reference(case)
    print(case.id, "pooled %.3g  feature %.3g  gradient %.3g" % pc.errors(case, built, acts, gx, ref))
    pc.check(case, built, acts, gx, ref)


@pytest.mark.parametrize("case", [c for c in pc.SMALL if c.op == "max"], ids=[c.id for c in pc.SMALL])
def test_exact_data_ties(case):
    """The exact construction does what it is for: windows whose maximum occurs more than once (a 2-frame 8-channel 13 x 11 plane
    has dozens), so the first-maximum rule decides where the gradient goes."""
    tied = pc.tied_windows(case)
    print(case.id, "tied windows:", tied)
    assert tied >= 10


def test_fewer_frames_than_planned():
    """Planned for 4 frames, run with 2: the bits of a net planned for 2."""
    case = pc.FEWER_FRAMES
    (a4, g4), = _run(case, planned=4)
    (a2, g2), = _run(case)
    assert a4.keys() == a2.keys() and all(torch.equal(a4[t], a2[t]) for t in a2)
    assert torch.equal(g4, g2)
    pc.check(case, pc.build(case), a4, g4, pc.reference(case))


def test_oracle_avgpool_backward_for_any_window():
    """OracleNet's hand-written backward through an average pool (ATen's adjoint) against autograd, k > stride and k < stride."""
    from oracle import restate
    for cid in ("a32_13x11", "a23_13x11", "a22_13x11"):
        case = pc.BY_ID[cid]
        b, ref = pc.build(case), pc.reference(case)
        onet = restate.OracleNet(b.graph, b.sd, [b.hook], dtype=torch.float64)
        feats = onet.forward(b.x.double())
        assert torch.allclose(feats[0], ref["feat"], rtol=1e-12, atol=1e-12)
        gx = onet.backward([b.hg.double()])          # (its conv branch applies the hook's own ReLU gate)
        assert (gx - ref["gx"]).abs().max() <= 1e-12 * ref["gx"].abs().max(), cid
