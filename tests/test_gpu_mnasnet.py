"""GPU: the depthwise convolution kernel (k_dwconv) alone and inside the MNASNets, against the float64 CPU reference of
tests/mnasnet_reference.py.

The bound is relative L2 against float64: the larger of 1e-5 and 4 x the error of the float32 CPU run of the same reference on the same
inputs, read from tests/golden/mnasnet_fp32_cpu_errors.json (tests/make_mnasnet_fixtures.py), never from the device run (DESIGN.md
sections 14 to 16)."""
import json

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from i2v_amd import attacks, graphs, weights  # noqa: E402
from oracle import restate  # noqa: E402
from tests import make_mnasnet_fixtures as mk  # noqa: E402
from tests import mnasnet_reference as mr  # noqa: E402
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
    """Plan, forward, backward: (hook features, input gradient, depthwise launches, dense-kernel launches)."""
    N = x.shape[0]
    net = eng.build_net(g, sd, hooks, N)
    g0, c0 = stat(eng, b"dwconv_launches"), stat(eng, b"conv_launches")
    net.forward(dev(x))
    feats = [net.read_tensor(t, N).cpu() for t in hooks]
    write_hook_grads(net, [torch.ones_like(f) for f in feats64], gated, N)       # (the gradients are gated already: gate of ones)
    gx = torch.empty(N, 3, x.shape[2], x.shape[3], device="cuda:0")
    net.backward(gx)
    torch.cuda.synchronize()
    out = feats, gx.cpu(), stat(eng, b"dwconv_launches") - g0, stat(eng, b"conv_launches") - c0
    net.close()
    return out


_REF = {}


def reference(tag, g, sd, hooks, frames):
    """Inputs and the float64 results of a case, computed once per module run."""
    if tag not in _REF:
        x, hg = mr.case_inputs(tag, g, frames, hooks)
        ref = mr.FamilyRef(g, sd, hooks, torch.float64)
        f64, _ = ref.run(x)
        gated = [h * (f > 0).to(h.dtype) if g.tensors[t].post_relu else h for h, f, t in zip(hg, f64, hooks)]
        _, g64 = ref.run(x, gated)
        _REF[tag] = (x, gated, f64, g64)
    return _REF[tag]


def check_case(eng, monkeypatch, tag, g, sd, hooks, frames):
    monkeypatch.setenv("I2V_AUTOTUNE", "0")
    n_dw = mr.n_depthwise(g, hooks)
    assert n_dw >= 1
    x, gated, f64, g64 = reference(tag, g, sd, hooks, frames)
    monkeypatch.delenv("I2V_DWCONV", raising=False)
    a = run_net(eng, g, sd, hooks, x, gated, f64)
    b = run_net(eng, g, sd, hooks, x, gated, f64)
    monkeypatch.setenv("I2V_DWCONV", "0")
    d = run_net(eng, g, sd, hooks, x, gated, f64)
    assert a[2] == 2 * n_dw and b[2] == 2 * n_dw, (a[2], n_dw)                     # one launch per node and pass
    assert d[2] == 0                                                               # the dense route: no depthwise launch ...
    assert d[3] > a[3] and a[3] == b[3]                                            # ... its nodes ran on the dense kernels instead
    for i in range(len(hooks)):
        assert torch.equal(a[0][i], b[0][i])                                       # the same bits every run
        e_k, e_d, bd = mr.rel_l2(a[0][i], f64[i]), mr.rel_l2(d[0][i], f64[i]), bound(FP32[tag]["hooks"][i])
        print(f"{tag} hook {i}: kernel {e_k:.3e} dense {e_d:.3e} fp32-cpu {FP32[tag]['hooks'][i]:.3e} bound {bd:.3e}")
        assert e_k <= bd and e_d <= bd
        assert mr.rel_l2(a[0][i], d[0][i]) <= bd
    assert torch.equal(a[1], b[1])
    e_k, e_d, bd = mr.rel_l2(a[1], g64), mr.rel_l2(d[1], g64), bound(FP32[tag]["gx"])
    print(f"{tag} gx: kernel {e_k:.3e} dense {e_d:.3e} fp32-cpu {FP32[tag]['gx']:.3e} bound {bd:.3e}")
    assert e_k <= bd and e_d <= bd
    assert mr.rel_l2(a[1], d[1]) <= bd


@pytest.mark.parametrize("case", mr.NODE_CASES, ids=mr.case_id)
def test_depthwise_node_alone(eng, monkeypatch, case):
    C, k, plane, stride, frames = case
    g = mr.node_alone_graph(C, k, plane, stride)
    check_case(eng, monkeypatch, mr.case_id(case), g, weights.synthetic_state_dict(g, 7), [g.hooks[1]], frames)


def test_tiny_twin(eng, monkeypatch):
    g = graphs.build_tiny("mnasnet_tiny", (64, 64))
    check_case(eng, monkeypatch, "mnasnet_tiny", g, weights.synthetic_state_dict(g, 7), [g.hooks[d] for d in (1, 2, 3, 4)], 3)


@pytest.mark.parametrize("name", ["mnasnet1_0", "mnasnet0_5"])
def test_full_size(eng, monkeypatch, name):
    g = graphs.build(name, (224, 224))
    hooks = [g.hooks[d] for d in (1, 2, 3, 4)]
    assert mr.n_depthwise(g, hooks) == 17
    check_case(eng, monkeypatch, name, g, weights.synthetic_state_dict(g, 7), hooks, 2)


def test_gates_off_agrees_with_the_default(eng, monkeypatch):
    monkeypatch.setenv("I2V_AUTOTUNE", "0")
    g = graphs.build_tiny("mnasnet_tiny", (64, 64))
    sd, hooks = weights.synthetic_state_dict(g, 7), [g.hooks[d] for d in (1, 2, 3, 4)]
    x, gated, f64, _ = reference("mnasnet_tiny", g, sd, hooks, 3)
    a = run_net(eng, g, sd, hooks, x, gated, f64)
    monkeypatch.setenv("I2V_GATES", "0")
    b = run_net(eng, g, sd, hooks, x, gated, f64)
    n_dw = mr.n_depthwise(g, hooks)
    assert a[2] == 2 * n_dw and b[2] == 2 * n_dw
    assert all(torch.equal(p, q) for p, q in zip(a[0], b[0])) and torch.equal(a[1], b[1])


def test_i2v_trajectory_ten_steps(eng):
    torch.manual_seed(11)
    vid = torch.randn(1, 3, 4, 64, 64)
    atk = attacks.ImageGuidedFMDirection_Adam(["mnasnet_tiny"], depth=3, step_size=0.005, steps=10, graph_builder=graphs.build_tiny, weight_seed=0)
    adv = atk(vid, torch.zeros(1, dtype=torch.long), ["t"])
    torch.cuda.synchronize()
    g = graphs.build_tiny("mnasnet_tiny", (64, 64))
    dg, dsd = mr.dense_twin(g, weights.synthetic_state_dict(g, 0))
    ref = restate.run_attack([restate.OracleNet(dg, dsd, [dg.hooks[3]])], vid, steps=10, step_size=0.005)
    np.testing.assert_allclose(atk.last_costs, ref["costs"], rtol=2e-4)
    assert float((adv.cpu() - ref["adv"]).abs().mean()) < 5e-3


#: i2v_net_workspace_bytes of mnasnet1_0 planned for 128 frames of 224 x 224 at depth 3 (DESIGN.md section 16 records the same figure and
#: how it is derived: the host simulation's plan of the same net, less the dense packings of the depthwise nodes, plus the compact
#: operands k_dwconv reads).  It does not depend on the autotuner.
MNASNET1_0_D3_128_BYTES = 5010735200


def test_mnasnet1_0_plans(eng, monkeypatch):
    """The plan only: 128 frames at depth 3; the workspace equals the recorded figure, on both calls."""
    monkeypatch.setenv("I2V_AUTOTUNE", "0")
    g = graphs.build("mnasnet1_0", (224, 224))
    sd = weights.synthetic_state_dict(g.truncated([g.hooks[3]]), 0)
    sizes = []
    for _ in range(2):
        net = eng.build_net(g, sd, [g.hooks[3]], 128)
        sizes.append(int(net.workspace_bytes()))
        net.close()
    print("mnasnet1_0 depth 3, 128 frames: workspace bytes", sizes)
    assert sizes[0] == sizes[1] == MNASNET1_0_D3_128_BYTES


def test_aens_mnasnet_tiny_with_tiny_resnet_and_tiny_vit_matches_the_oracle():
    """AENS over mnasnet_tiny + the tiny ResNet + the tiny ViT: the depthwise net through the ensemble path (accumulated input gradients,
    the coefficient kernels) against the oracle's costs and coefficients.  The oracle gets the dense twin of mnasnet_tiny.  Bounds as
    tests/test_gpu_resnet_family.py::test_aens_grouped_net_with_tiny_resnet_and_tiny_vit_matches_the_oracle."""
    from tests.vit_reference import VitReference
    gen = torch.Generator().manual_seed(24)
    u8 = torch.randint(0, 256, (1, 3, 4, 64, 64), generator=gen, dtype=torch.uint8)
    vid = (u8.float() / 255 - torch.tensor(restate.MEAN).view(1, 3, 1, 1, 1)) / torch.tensor(restate.STD).view(1, 3, 1, 1, 1)
    vit = graphs.VIT_NAME
    depths = {"mnasnet_tiny": [2, 3], "resnet": [2, 3], vit: [1, 2]}
    atk = attacks.AENS_I2V_MF(["mnasnet_tiny", "resnet", vit], depths=depths, step_size=0.005, steps=4, momentum=0.5,
                              graph_builder=graphs.build_tiny, weight_seed=0)
    adv, _, costs = atk(vid, torch.zeros(1, dtype=torch.long), ["a"])
    assert atk.engine.capi.i2v_backend() == b"hip:gfx950"
    ms, rs, vs = (graphs.build_tiny(n, (64, 64)) for n in ("mnasnet_tiny", "resnet", vit))
    dg, dsd = mr.dense_twin(ms, weights.synthetic_state_dict(ms, 0))
    nets = [restate.OracleNet(dg, dsd, [dg.hook_for(d, True) for d in depths["mnasnet_tiny"]], dtype=torch.float64),
            restate.OracleNet(rs, weights.synthetic_state_dict(rs, 0), [rs.hook_for(d, True) for d in depths["resnet"]], dtype=torch.float64),
            VitReference(vs, weights.synthetic_state_dict(vs, 0), [vs.hook_for(d) for d in depths[vit]], dtype=torch.float64)]
    ref = restate.run_attack(nets, vid, steps=4, step_size=0.005, mode="aens", coeffs=torch.ones(6, dtype=torch.float64), momentum=0.5)
    np.testing.assert_allclose(costs, ref["costs"], rtol=2e-4)
    w = np.stack(atk.weights)
    np.testing.assert_allclose(w, np.stack(ref["weights"]), rtol=1e-4, atol=1e-6)
    np.testing.assert_allclose(atk.coeffs.cpu().numpy(), ref["coeffs"].float().numpy(), rtol=1e-4)
    assert np.abs(w[-1] - 1 / 6).max() > 1e-4                        # the coefficients moved off uniform
