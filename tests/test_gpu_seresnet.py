"""GPU: the squeeze-and-excitation kernels (k_se_squeeze / k_se_excite / k_se_scale) alone and inside the SE-ResNets, against the
float64 CPU reference of tests/seresnet_reference.py.

The bound is relative L2 against float64: the larger of 1e-5 and 4 x the error of the float32 CPU run of the same reference on the same
inputs, read from tests/golden/seresnet_fp32_cpu_errors.json (tests/make_seresnet_fixtures.py), never from the device run (DESIGN.md
sections 14 to 17)."""
import json

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from i2v_amd import attacks, graphs, weights  # noqa: E402
from oracle import restate  # noqa: E402
from tests import make_seresnet_fixtures as mk  # noqa: E402
from tests import seresnet_reference as sr  # noqa: E402
from tests.test_gpu_parity import dev, write_hook_grads  # noqa: E402

FP32 = json.load(open(mk.ERRS))
FLOOR = 1e-5


def bound(fp32_err):
    return max(FLOOR, 4.0 * fp32_err)


@pytest.fixture(scope="module")
def eng():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    e = attacks.get_engine("cuda:0")
    assert e.capi.i2v_backend() == b"hip:gfx950"
    return e


def stat(eng, name):
    return eng.capi.i2v_backend_stat(name)


def run_net(eng, g, sd, hooks, x, gated, feats64):
    """Plan, forward, backward: (hook features, input gradient, SE launches, grouped-convolution launches)."""
    N = x.shape[0]
    net = eng.build_net(g, sd, hooks, N)
    s0, g0 = stat(eng, b"se_launches"), stat(eng, b"gconv_launches")
    net.forward(dev(x))
    feats = [net.read_tensor(t, N).cpu() for t in hooks]
    write_hook_grads(net, [torch.ones_like(f) for f in feats64], gated, N)       # (the gradients are gated already: gate of ones)
    gx = torch.empty(N, 3, x.shape[2], x.shape[3], device="cuda:0")
    net.backward(gx)
    torch.cuda.synchronize()
    out = feats, gx.cpu(), stat(eng, b"se_launches") - s0, stat(eng, b"gconv_launches") - g0
    net.close()
    return out


_REF = {}


def reference(tag, g, sd, hooks, frames):
    """Inputs and the float64 results of a case, computed once per module run."""
    if tag not in _REF:
        x, hg = sr.case_inputs(tag, g, frames, hooks)
        f64, gated, g64, _ = sr.reference(g, sd, hooks, x, hg)
        _REF[tag] = (x, gated, f64, g64)
    return _REF[tag]


def check_case(eng, monkeypatch, case, one_frame=True):
    monkeypatch.setenv("I2V_AUTOTUNE", "0")
    tag, g, sd, hooks, frames = case
    n = sr.n_se(g, hooks)
    assert n >= 1
    x, gated, f64, g64 = reference(tag, g, sd, hooks, frames)
    a = run_net(eng, g, sd, hooks, x, gated, f64)
    b = run_net(eng, g, sd, hooks, x, gated, f64)
    assert a[2] == 6 * n and b[2] == 6 * n, (a[2], n)                              # three launches per node and pass
    for i in range(len(hooks)):
        assert torch.equal(a[0][i], b[0][i])                                       # the same bits every run
        e, bd = sr.rel_l2(a[0][i], f64[i]), bound(FP32[tag]["hooks"][i])
        print(f"{tag} hook {i}: device {e:.3e} fp32-cpu {FP32[tag]['hooks'][i]:.3e} bound {bd:.3e}")
        assert e <= bd
    assert torch.equal(a[1], b[1])
    e, bd = sr.rel_l2(a[1], g64), bound(FP32[tag]["gx"])
    print(f"{tag} gx: device {e:.3e} fp32-cpu {FP32[tag]['gx']:.3e} bound {bd:.3e}")
    assert e <= bd
    if one_frame:               # frame 0 has the same bits at `frames` frames and at 1
        one = run_net(eng, g, sd, hooks, x[:1], [h[:1] for h in gated], [f[:1] for f in f64])
        assert all(torch.equal(p[:1], q) for p, q in zip(a[0], one[0])) and torch.equal(a[1][:1], one[1])
    return a


@pytest.mark.parametrize("case", sr.NODE_CASES, ids=sr.case_id)
def test_se_node_alone(eng, monkeypatch, case):
    check_case(eng, monkeypatch, mk.node_case(case))


@pytest.mark.parametrize("tag", ["seresnet_tiny", "seresnext_tiny"])
def test_tiny_twins(eng, monkeypatch, tag):
    a = check_case(eng, monkeypatch, mk.net_case(tag))
    assert (a[3] > 0) == (tag == "seresnext_tiny")


@pytest.mark.parametrize("tag", ["seresnet50", "seresnext50_32x4d"])
def test_full_size(eng, monkeypatch, tag):
    case = mk.net_case(tag)
    assert sr.n_se(case[1], case[3]) == 16
    a = check_case(eng, monkeypatch, case, one_frame=False)
    if tag == "seresnext50_32x4d":
        assert a[3] == 2 * 16                                                       # conv2 of every block on the grouped kernel, both passes
    else:
        assert a[3] == 0


def test_gates_off_agrees_with_the_default(eng, monkeypatch):
    monkeypatch.setenv("I2V_AUTOTUNE", "0")
    tag, g, sd, hooks, frames = mk.net_case("seresnet_tiny")
    x, gated, f64, _ = reference(tag, g, sd, hooks, frames)
    a = run_net(eng, g, sd, hooks, x, gated, f64)
    monkeypatch.setenv("I2V_GATES", "0")
    b = run_net(eng, g, sd, hooks, x, gated, f64)
    assert a[2] == b[2] == 6 * sr.n_se(g, hooks)
    assert all(torch.equal(p, q) for p, q in zip(a[0], b[0])) and torch.equal(a[1], b[1])


def test_i2v_trajectory_ten_steps(eng):
    torch.manual_seed(11)
    vid = torch.randn(1, 3, 4, 64, 64)
    atk = attacks.ImageGuidedFMDirection_Adam(["seresnet_tiny"], depth=3, step_size=0.005, steps=10, graph_builder=graphs.build_tiny, weight_seed=0)
    adv = atk(vid, torch.zeros(1, dtype=torch.long), ["t"])
    torch.cuda.synchronize()
    g = graphs.build_tiny("seresnet_tiny", (64, 64))
    ref = restate.run_attack([sr.SeRef(g, weights.synthetic_state_dict(g, 0), [g.hooks[3]], dtype=torch.float64)], vid, steps=10, step_size=0.005)
    np.testing.assert_allclose(atk.last_costs, ref["costs"], rtol=2e-4)
    assert float((adv.cpu() - ref["adv"].float()).abs().mean()) < 5e-3


#: i2v_net_workspace_bytes of seresnet50 planned for 128 frames of 224 x 224 at depth 3 (DESIGN.md section 17 records the same figure and
#: how it is made up: the host simulation's plan of the same net, which lays out the same arena and packs the same operands, the node
#: vectors and weights included).  It does not depend on the autotuner.
SERESNET50_D3_128_BYTES = 16809037344


def test_seresnet50_plans(eng, monkeypatch):
    """The plan only: 128 frames at depth 3; the workspace equals the recorded figure, on both calls."""
    monkeypatch.setenv("I2V_AUTOTUNE", "0")
    g = graphs.build("seresnet50", (224, 224))
    sd = weights.synthetic_state_dict(g.truncated([g.hooks[3]]), 0)
    sizes = []
    for _ in range(2):
        net = eng.build_net(g, sd, [g.hooks[3]], 128)
        sizes.append(int(net.workspace_bytes()))
        net.close()
    print("seresnet50 depth 3, 128 frames: workspace bytes", sizes)
    assert sizes[0] == sizes[1] == SERESNET50_D3_128_BYTES


def test_aens_seresnet_tiny_with_tiny_resnet_and_tiny_vit_matches_the_oracle():
    """AENS over seresnet_tiny + the tiny ResNet + the tiny ViT: the SE net through the ensemble path (accumulated input gradients, the
    coefficient kernels) against the oracle's costs, weights and coefficients.  Bounds as
    tests/test_gpu_mnasnet.py::test_aens_mnasnet_tiny_with_tiny_resnet_and_tiny_vit_matches_the_oracle."""
    from tests.vit_reference import VitReference
    gen = torch.Generator().manual_seed(24)
    u8 = torch.randint(0, 256, (1, 3, 4, 64, 64), generator=gen, dtype=torch.uint8)
    vid = (u8.float() / 255 - torch.tensor(restate.MEAN).view(1, 3, 1, 1, 1)) / torch.tensor(restate.STD).view(1, 3, 1, 1, 1)
    vit = graphs.VIT_NAME
    depths = {"seresnet_tiny": [2, 3], "resnet": [2, 3], vit: [1, 2]}
    atk = attacks.AENS_I2V_MF(["seresnet_tiny", "resnet", vit], depths=depths, step_size=0.005, steps=4, momentum=0.5,
                              graph_builder=graphs.build_tiny, weight_seed=0)
    adv, _, costs = atk(vid, torch.zeros(1, dtype=torch.long), ["a"])
    assert atk.engine.capi.i2v_backend() == b"hip:gfx950"
    ss, rs, vs = (graphs.build_tiny(n, (64, 64)) for n in ("seresnet_tiny", "resnet", vit))
    nets = [sr.SeRef(ss, weights.synthetic_state_dict(ss, 0), [ss.hook_for(d, True) for d in depths["seresnet_tiny"]], dtype=torch.float64),
            restate.OracleNet(rs, weights.synthetic_state_dict(rs, 0), [rs.hook_for(d, True) for d in depths["resnet"]], dtype=torch.float64),
            VitReference(vs, weights.synthetic_state_dict(vs, 0), [vs.hook_for(d) for d in depths[vit]], dtype=torch.float64)]
    ref = restate.run_attack(nets, vid, steps=4, step_size=0.005, mode="aens", coeffs=torch.ones(6, dtype=torch.float64), momentum=0.5)
    np.testing.assert_allclose(costs, ref["costs"], rtol=2e-4)
    w = np.stack(atk.weights)
    np.testing.assert_allclose(w, np.stack(ref["weights"]), rtol=1e-4, atol=1e-6)
    np.testing.assert_allclose(atk.coeffs.cpu().numpy(), ref["coeffs"].float().numpy(), rtol=1e-4)
    assert np.abs(w[-1] - 1 / 6).max() > 1e-4                        # the coefficients moved off uniform
