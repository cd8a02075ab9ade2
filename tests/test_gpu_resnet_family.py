"""GPU: the grouped 3x3 convolution kernel (k_gconv) alone and inside the ResNet-family nets, against the float64 CPU reference of
tests/resnet_family_reference.py.

The bound is relative L2 against float64: the larger of 1e-5 -- what tests/test_gpu_parity.py::test_conv_property_based allows a 3x3
layer (max |err| <= 1e-5 max |ref|) -- and 4 x the error of the float32 CPU run of the same reference on the same inputs, read from
tests/golden/resnet_family_fp32_cpu_errors.json (tests/make_resnet_family_fixtures.py), never from the device run.  A correct fp32
kernel with another summation order sits within a small multiple of the CPU's own fp32 error."""
import json

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from i2v_amd import attacks, graphs, weights  # noqa: E402
from oracle import restate  # noqa: E402
from tests import make_resnet_family_fixtures as mk  # noqa: E402
from tests import resnet_family_reference as rf  # noqa: E402
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
    """Plan, forward, backward: (hook features, input gradient, grouped launches, dense-kernel launches)."""
    N = x.shape[0]
    net = eng.build_net(g, sd, hooks, N)
    g0, c0 = stat(eng, b"gconv_launches"), stat(eng, b"conv_launches")
    net.forward(dev(x))
    feats = [net.read_tensor(t, N).cpu() for t in hooks]
    write_hook_grads(net, [torch.ones_like(f) for f in feats64], gated, N)       # (the gradients are gated already: gate of ones)
    gx = torch.empty(N, 3, x.shape[2], x.shape[3], device="cuda:0")
    net.backward(gx)
    torch.cuda.synchronize()
    out = feats, gx.cpu(), stat(eng, b"gconv_launches") - g0, stat(eng, b"conv_launches") - c0
    net.close()
    return out


def check_case(eng, monkeypatch, tag, g, sd, hooks, frames, n_grouped):
    monkeypatch.setenv("I2V_AUTOTUNE", "0")
    x, hg = rf.case_inputs(tag, g, frames, hooks)
    ref = rf.FamilyRef(g, sd, hooks, torch.float64)
    f64, _ = ref.run(x)
    gated = [h * (f > 0).to(h.dtype) if g.tensors[t].post_relu else h for h, f, t in zip(hg, f64, hooks)]
    _, g64 = ref.run(x, gated)
    monkeypatch.delenv("I2V_GCONV", raising=False)
    a = run_net(eng, g, sd, hooks, x, gated, f64)
    b = run_net(eng, g, sd, hooks, x, gated, f64)
    monkeypatch.setenv("I2V_GCONV", "0")
    d = run_net(eng, g, sd, hooks, x, gated, f64)
    assert a[2] == 2 * n_grouped and b[2] == 2 * n_grouped, (a[2], n_grouped)     # one launch per node and pass
    assert d[2] == 0                                                               # the dense route: no grouped launch ...
    if n_grouped:
        assert d[3] > a[3] and a[3] == b[3]                                        # ... its nodes ran on the dense kernels instead
    else:
        assert d[3] == a[3]
    for i in range(len(hooks)):
        assert torch.equal(a[0][i], b[0][i])                                       # the same bits every run
        e_k, e_d = rf.rel_l2(a[0][i], f64[i]), rf.rel_l2(d[0][i], f64[i])
        print(f"{tag} hook {i}: kernel {e_k:.3e} dense {e_d:.3e} fp32-cpu {FP32[tag]['hooks'][i]:.3e} bound {bound(FP32[tag]['hooks'][i]):.3e}")
        assert e_k <= bound(FP32[tag]["hooks"][i]) and e_d <= bound(FP32[tag]["hooks"][i])
        assert rf.rel_l2(a[0][i], d[0][i]) <= bound(FP32[tag]["hooks"][i])
    assert torch.equal(a[1], b[1])
    e_k, e_d = rf.rel_l2(a[1], g64), rf.rel_l2(d[1], g64)
    print(f"{tag} gx: kernel {e_k:.3e} dense {e_d:.3e} fp32-cpu {FP32[tag]['gx']:.3e} bound {bound(FP32[tag]['gx']):.3e}")
    assert e_k <= bound(FP32[tag]["gx"]) and e_d <= bound(FP32[tag]["gx"])
    assert rf.rel_l2(a[1], d[1]) <= bound(FP32[tag]["gx"])


@pytest.mark.parametrize("case", rf.NODE_CASES, ids=rf.case_id)
def test_grouped_node_alone(eng, monkeypatch, case):
    C, groups, plane, stride, frames = case
    g = rf.node_alone_graph(C, groups, plane, stride)
    check_case(eng, monkeypatch, rf.case_id(case), g, weights.synthetic_state_dict(g, 7), [g.hooks[1]], frames, 1)


@pytest.mark.parametrize("name,n_grouped", [("resnext_tiny", 6), ("resnet_basic_tiny", 0)])
def test_twins(eng, monkeypatch, name, n_grouped):
    g = graphs.build_tiny(name, (64, 64))
    check_case(eng, monkeypatch, name, g, weights.synthetic_state_dict(g, 7), [g.hooks[d] for d in (1, 2, 3, 4)], 3, n_grouped)


@pytest.mark.parametrize("name,n_grouped", [("resnext50_32x4d", 16), ("resnet18", 0)])
def test_full_size(eng, monkeypatch, name, n_grouped):
    g = graphs.build(name, (224, 224))
    check_case(eng, monkeypatch, name, g, weights.synthetic_state_dict(g, 7), [g.hooks[d] for d in (1, 2, 3, 4)], 2, n_grouped)


def test_gates_off_agrees_with_the_default(eng, monkeypatch):
    monkeypatch.setenv("I2V_AUTOTUNE", "0")
    g = graphs.build_tiny("resnext_tiny", (64, 64))
    sd, hooks = weights.synthetic_state_dict(g, 7), [g.hooks[d] for d in (1, 2, 3, 4)]
    x, hg = rf.case_inputs("resnext_tiny", g, 3, hooks)
    f64, _ = rf.FamilyRef(g, sd, hooks, torch.float64).run(x)
    gated = [h * (f > 0).to(h.dtype) for h, f in zip(hg, f64)]
    a = run_net(eng, g, sd, hooks, x, gated, f64)
    monkeypatch.setenv("I2V_GATES", "0")
    b = run_net(eng, g, sd, hooks, x, gated, f64)
    assert a[2] == 12 and b[2] == 12
    assert all(torch.equal(p, q) for p, q in zip(a[0], b[0])) and torch.equal(a[1], b[1])


@pytest.mark.parametrize("name", ["resnext_tiny", "resnet_basic_tiny"])
def test_i2v_trajectory_ten_steps(eng, name):
    torch.manual_seed(11)
    vid = torch.randn(1, 3, 4, 64, 64)
    atk = attacks.ImageGuidedFMDirection_Adam([name], depth=3, step_size=0.005, steps=10, graph_builder=graphs.build_tiny, weight_seed=0)
    adv = atk(vid, torch.zeros(1, dtype=torch.long), ["t"])
    torch.cuda.synchronize()
    g = graphs.build_tiny(name, (64, 64))
    dg, dsd = rf.dense_twin(g, weights.synthetic_state_dict(g, 0))
    ref = restate.run_attack([restate.OracleNet(dg, dsd, [dg.hooks[3]])], vid, steps=10, step_size=0.005)
    np.testing.assert_allclose(atk.last_costs, ref["costs"], rtol=2e-4)
    assert float((adv.cpu() - ref["adv"]).abs().mean()) < 5e-3


#: i2v_net_workspace_bytes of resnext101_32x8d planned for 128 frames of 224 x 224 at depth 3 (DESIGN.md section 15 records the same
#: figure; the engine has no Python restatement of its arena).  It does not depend on the autotuner.  Derived from the host
#: simulation's plan of the same net -- the arena is the same on both routes -- with the dense packings of the grouped nodes
#: replaced by the compact operands k_gconv reads.
RESNEXT101_32X8D_D3_128_BYTES = 32037179232


def test_resnext101_32x8d_plans(eng, monkeypatch):
    """The plan only: 128 frames at depth 3; the workspace equals the recorded figure, on both calls."""
    monkeypatch.setenv("I2V_AUTOTUNE", "0")
    g = graphs.build("resnext101_32x8d", (224, 224))
    sd = weights.synthetic_state_dict(g.truncated([g.hooks[3]]), 0)
    sizes = []
    for _ in range(2):
        net = eng.build_net(g, sd, [g.hooks[3]], 128)
        sizes.append(int(net.workspace_bytes()))
        net.close()
    print("resnext101_32x8d depth 3, 128 frames: workspace bytes", sizes)
    assert sizes[0] == sizes[1] == RESNEXT101_32X8D_D3_128_BYTES


def test_aens_grouped_net_with_tiny_resnet_and_tiny_vit_matches_the_oracle():
    """AENS over resnext_tiny + the tiny ResNet + the tiny ViT: the grouped net through the ensemble path (accumulated input gradients,
    the coefficient kernels) against the oracle's costs and coefficients.  The oracle gets the dense twin of resnext_tiny."""
    from tests.vit_reference import VitReference
    gen = torch.Generator().manual_seed(24)
    u8 = torch.randint(0, 256, (1, 3, 4, 64, 64), generator=gen, dtype=torch.uint8)
    vid = (u8.float() / 255 - torch.tensor(restate.MEAN).view(1, 3, 1, 1, 1)) / torch.tensor(restate.STD).view(1, 3, 1, 1, 1)
    vit = graphs.VIT_NAME
    depths = {"resnext_tiny": [2, 3], "resnet": [2, 3], vit: [1, 2]}
    atk = attacks.AENS_I2V_MF(["resnext_tiny", "resnet", vit], depths=depths, step_size=0.005, steps=4, momentum=0.5,
                              graph_builder=graphs.build_tiny, weight_seed=0)
    adv, _, costs = atk(vid, torch.zeros(1, dtype=torch.long), ["a"])
    xs, rs, vs = (graphs.build_tiny(n, (64, 64)) for n in ("resnext_tiny", "resnet", vit))
    dg, dsd = rf.dense_twin(xs, weights.synthetic_state_dict(xs, 0))
    nets = [restate.OracleNet(dg, dsd, [dg.hook_for(d, True) for d in depths["resnext_tiny"]], dtype=torch.float64),
            restate.OracleNet(rs, weights.synthetic_state_dict(rs, 0), [rs.hook_for(d, True) for d in depths["resnet"]], dtype=torch.float64),
            VitReference(vs, weights.synthetic_state_dict(vs, 0), [vs.hook_for(d) for d in depths[vit]], dtype=torch.float64)]
    ref = restate.run_attack(nets, vid, steps=4, step_size=0.005, mode="aens", coeffs=torch.ones(6, dtype=torch.float64), momentum=0.5)
    np.testing.assert_allclose(costs, ref["costs"], rtol=2e-4)
    w = np.stack(atk.weights)
    np.testing.assert_allclose(w, np.stack(ref["weights"]), rtol=1e-4, atol=1e-6)
    np.testing.assert_allclose(atk.coeffs.cpu().numpy(), ref["coeffs"].float().numpy(), rtol=1e-4)
    assert np.abs(w[-1] - 1 / 6).max() > 1e-4                        # the coefficients moved off uniform
