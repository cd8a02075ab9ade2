"""CPU: torchvision's MNASNet family in the graph IR (names, key / shape contract, hooks, MACs) and the depthwise convolution through the
planner on the host simulation, which runs depthwise nodes on the dense route (block-diagonal weight through the ordinary packings)."""
import ctypes as C
import json

import numpy as np
import pytest
import torch

from i2v_amd import attacks, graphs, lib, weights
from oracle import restate
from tests import make_mnasnet_fixtures as mk
from tests import mnasnet_reference as mr
from tests.hostsim_util import hostsim_engine
from tests.test_planner_hostsim import write_hook_grads

NAMES = tuple(mk.TV)


def test_names_are_the_issue_s():
    assert set(NAMES) == set(graphs.MNASNET_MODELS) == {"mnasnet0_5", "mnasnet0_75", "mnasnet1_0", "mnasnet1_3"}
    for name in NAMES:
        assert graphs.build(name).arch == name


@pytest.mark.parametrize("name", NAMES)
def test_param_shapes_equal_the_fixture(name):
    want = {k: tuple(v) for k, v in mk.expand_keys(json.load(open(mk.KEYS))[name]).items()}
    assert want == {k: tuple(v) for k, v in mk.torchvision_keys(mk.TV[name]).items()}          # the fixture is what the stated rule gives
    assert graphs.build(name, (224, 224)).param_shapes() == want


def test_spot_shapes():
    x = graphs.build("mnasnet1_0").param_shapes()
    assert x["layers.0.weight"] == (32, 3, 3, 3) and x["layers.3.weight"] == (32, 1, 3, 3) and x["layers.6.weight"] == (16, 32, 1, 1)
    assert x["layers.8.0.layers.0.weight"] == (48, 16, 1, 1) and x["layers.8.0.layers.3.weight"] == (48, 1, 3, 3)
    assert x["layers.12.1.layers.3.weight"] == (1152, 1, 5, 5) and x["layers.13.0.layers.6.weight"] == (320, 1152, 1, 1)
    assert graphs.mnasnet_depths(0.5) == [16, 8, 16, 24, 40, 48, 96, 160] and graphs.mnasnet_depths(1.3) == [40, 24, 32, 56, 104, 128, 248, 416]
    g = graphs.build("mnasnet1_0")
    dw = [(nd.cin, nd.kh, nd.stride, g.tensors[nd.dst].H) for nd in g.nodes if nd.groups > 1]
    assert len(dw) == 17 and all(nd.groups == nd.cin == nd.cout for nd in g.nodes if nd.groups > 1)
    assert dw[0] == (32, 3, 1, 112) and dw[1] == (48, 3, 2, 56) and dw[-1] == (1152, 3, 1, 7) and (1152, 5, 1, 7) in dw
    t = graphs.build_tiny("mnasnet_tiny", (64, 64))
    tw = [(nd.kh, nd.stride, t.tensors[nd.src].H, t.tensors[nd.dst].H) for nd in t.nodes if nd.groups > 1]
    assert {(k, s) for k, s, _, _ in tw} == {(3, 1), (3, 2), (5, 1), (5, 2)}
    assert (5, 1, 2, 2) in tw and tw[-1][3] == 2 and t.tensors[t.hooks[4]].H == 2            # a 5x5 filter on a 2 x 2 plane; the last plane
    assert sum(1 for nd in t.nodes if nd.op == "conv" and nd.residual is not None) >= 1       # identity blocks


@pytest.mark.parametrize("name", NAMES)
def test_hook_shapes_at_depths_1_to_4(name):
    g = graphs.build(name, (224, 224))
    want = mk.hook_shapes(mk.TV[name])
    for d in (1, 2, 3, 4):
        t = g.tensors[g.hook_for(d)]
        assert (t.C, t.H, t.W) == want[d] and not t.post_relu
    if name == "mnasnet1_0":
        assert want == {1: (24, 56, 56), 2: (40, 28, 28), 3: (96, 14, 14), 4: (320, 7, 7)}


@pytest.mark.parametrize("name", NAMES)
def test_macs_count_depthwise_nodes_by_their_real_products(name):
    g = graphs.build(name, (224, 224))
    assert g.macs_per_frame() == mk.reference_macs(mk.TV[name])
    dw = sum(g.tensors[nd.dst].H * g.tensors[nd.dst].W * nd.cout * nd.kh * nd.kw for nd in g.nodes if nd.groups > 1)
    dense = sum(g.tensors[nd.dst].H * g.tensors[nd.dst].W * nd.cout * nd.cin * nd.kh * nd.kw for nd in g.nodes if nd.groups == 1)
    assert g.macs_per_frame() == dw + dense


def test_refused_names_list_the_served_ones():
    for name in ("mnasnet2_0", "mnasnet", "mnasnet1_0_v1"):
        with pytest.raises(ValueError, match="mnasnet0_5, mnasnet0_75, mnasnet1_0, mnasnet1_3"):
            graphs.build(name)
    for name, word in (("mobilenet_v2", "ReLU6"), ("mobilenet_v3_large", "hard-swish"), ("shufflenet_v2_x1_0", "shuffle"), ("efficientnet_b0", "squeeze-excite")):
        with pytest.raises(ValueError, match=word) as e:
            graphs.build(name)
        assert "mnasnet1_0" in str(e.value)


def test_checkpoint_loads_and_a_dense_weight_is_refused(tmp_path, monkeypatch):
    g = graphs.build("mnasnet0_5", (224, 224))
    full = {k: torch.zeros(*shp) for k, shp in mk.torchvision_keys(0.5).items()}
    full.update({"layers.14.weight": torch.zeros(1280, 160, 1, 1), "classifier.1.bias": torch.zeros(1000), "layers.1.num_batches_tracked": torch.tensor(0)})
    monkeypatch.setenv("I2V_WEIGHTS_DIR", str(tmp_path))
    torch.save(full, tmp_path / "mnasnet0_5.pth")
    sd = weights.load_state_dict(g)
    assert set(sd) == set(g.param_shapes()) and sd["layers.9.0.layers.3.weight"].shape == (48, 1, 5, 5)
    bad = dict(full); bad["layers.9.0.layers.3.weight"] = torch.zeros(48, 48, 5, 5)
    torch.save(bad, tmp_path / "mnasnet0_5.pth")
    with pytest.raises(ValueError, match="layers.9.0.layers.3.weight"):
        weights.load_state_dict(g)
    syn = weights.synthetic_state_dict(g, 1)
    assert {k: tuple(v.shape) for k, v in syn.items()} == g.param_shapes()


def test_tiny_twin_on_the_host_simulation_matches_float64():
    """Hooks d = 1..4 and the input gradient, 2 frames of 64 x 64, at the bounds tests/test_resnet_family_cpu.py uses for resnext_tiny."""
    eng = hostsim_engine()
    g = graphs.build_tiny("mnasnet_tiny", (64, 64))
    sd = weights.synthetic_state_dict(g, 3)
    hooks = [g.hooks[d] for d in (1, 2, 3, 4)]
    N = 2
    net = eng.build_net(g, sd, hooks, N)
    x, hg = mr.case_inputs("mnasnet_tiny", g, N, hooks)
    ref = mr.FamilyRef(g, sd, hooks, torch.float64)
    feats, _ = ref.run(x)
    net.forward(x)
    for t, want in zip(hooks, feats):
        got = net.read_tensor(t, N).double()
        assert torch.allclose(got, want, rtol=1e-4, atol=max(1e-5, 1e-6 * float(want.abs().max())))
    write_hook_grads(net, feats, hg, N)
    _, want = ref.run(x, hg)                     # the hooked tensors are linear: no gate on the hook gradients
    gx = torch.empty(N, 3, 64, 64)
    net.backward(gx)
    err = (gx.double() - want).abs().max() / want.abs().max()
    assert err < 1e-4, err


def _attempt(cin, cout, k=3, stride=1, pad=None, residual=-1, kw=None):
    eng = hostsim_engine()
    capi, h = eng.capi, eng.h
    pad = k // 2 if pad is None else pad
    kw = k if kw is None else kw
    nid = C.c_int(); assert capi.i2v_net_create(h, C.byref(nid)) == 0
    b0, b1, t0, t1 = C.c_int(), C.c_int(), C.c_int(), C.c_int()
    ho, wo = (8 + 2 * pad - k) // stride + 1, (8 + 2 * pad - kw) // stride + 1
    assert capi.i2v_net_add_buffer(h, nid.value, cin, 8, 8, C.byref(b0)) == 0 and capi.i2v_net_add_buffer(h, nid.value, cout, ho, wo, C.byref(b1)) == 0
    assert capi.i2v_net_add_tensor(h, nid.value, b0.value, 0, cin, 0, C.byref(t0)) == 0 and capi.i2v_net_add_tensor(h, nid.value, b1.value, 0, cout, 1, C.byref(t1)) == 0
    d = lib.ConvDesc(t0.value, t1.value, cin, cout, k, kw, stride, pad, 1, t1.value if residual >= 0 else -1)
    w = np.zeros((cout, 1, k, kw), np.float32); s = np.ones(cout, np.float32)
    rc = capi.i2v_net_add_conv_depthwise(h, nid.value, C.byref(d), w.ctypes.data, s.ctypes.data, s.ctypes.data)
    msg = capi.i2v_last_error().decode() if rc else ""
    capi.i2v_net_destroy(h, nid.value)
    return rc, msg


def test_depthwise_entry_refuses_what_it_does_not_serve():
    assert _attempt(16, 16)[0] == 0 and _attempt(16, 16, 5, 2)[0] == 0 and _attempt(5, 5, 5, 1)[0] == 0 and _attempt(16, 16, 3, 2)[0] == 0
    for kwargs, word in ((dict(cin=16, cout=32), "as many out as in"), (dict(cin=16, cout=16, k=3, kw=5), "square"), (dict(cin=16, cout=16, k=7), "3x3 and 5x5"),
                         (dict(cin=16, cout=16, k=1), "3x3 and 5x5"), (dict(cin=16, cout=16, k=5, pad=1), "padding"), (dict(cin=16, cout=16, k=3, pad=0), "padding"),
                         (dict(cin=16, cout=16, stride=3), "stride"), (dict(cin=16, cout=16, residual=0), "residual")):
        rc, msg = _attempt(**kwargs)
        assert rc != 0 and word in msg and "i2v_net_add_conv_depthwise" in msg, (kwargs, msg)


def test_grouped_entry_still_refuses_group_width_one():
    eng = hostsim_engine()
    capi, h = eng.capi, eng.h
    nid = C.c_int(); assert capi.i2v_net_create(h, C.byref(nid)) == 0
    b0, b1, t0, t1 = C.c_int(), C.c_int(), C.c_int(), C.c_int()
    assert capi.i2v_net_add_buffer(h, nid.value, 16, 8, 8, C.byref(b0)) == 0 and capi.i2v_net_add_buffer(h, nid.value, 16, 8, 8, C.byref(b1)) == 0
    assert capi.i2v_net_add_tensor(h, nid.value, b0.value, 0, 16, 0, C.byref(t0)) == 0 and capi.i2v_net_add_tensor(h, nid.value, b1.value, 0, 16, 1, C.byref(t1)) == 0
    d = lib.ConvDesc(t0.value, t1.value, 16, 16, 3, 3, 1, 1, 1, -1)
    w = np.zeros((16, 1, 3, 3), np.float32); s = np.ones(16, np.float32)
    assert capi.i2v_net_add_conv_grouped(h, nid.value, C.byref(d), 16, w.ctypes.data, s.ctypes.data, s.ctypes.data) != 0
    assert "group width" in capi.i2v_last_error().decode()
    capi.i2v_net_destroy(h, nid.value)


def test_plan_refuses_a_second_consumer_of_the_depthwise_input():
    """stem -> a; a feeds the depthwise node AND a 1x1 convolution: the depthwise input gradient would have to be accumulated."""
    g = graphs.Graph("dw_two_consumers", (8, 8))
    x = g.new_tensor(3, 8, 8, False, "input")
    g.input = x
    a = g.conv(x, 8, 3, 1, 1, "stem.weight", bn="stem_bn", relu=True, name="stem")
    y = g.conv(a, 8, 3, 1, 1, "dw.weight", bn="dw_bn", relu=True, name="dw", groups=8)
    z = g.conv(a, 8, 1, 1, 0, "side.weight", bn="side_bn", relu=False, residual=y, name="side")
    g.hooks[1] = z
    with pytest.raises(lib.I2VError, match="only consumer"):
        hostsim_engine().build_net(g, weights.synthetic_state_dict(g, 0), [z], 1)


def test_i2v_trajectory_on_mnasnet_tiny_matches_the_oracle():
    """3 steps of the I2V attack.  `oracle.restate` has no `groups`; it is handed the dense twin of the graph (every depthwise
    convolution as a dense one on the block-diagonal weight: the same function) and runs its own loop unchanged.  The depthwise
    convention itself is pinned by test_tiny_twin_on_the_host_simulation_matches_float64, against F.conv2d(groups=C)."""
    torch.manual_seed(5)
    vid = torch.randn(1, 3, 2, 64, 64)
    atk = attacks.ImageGuidedFMDirection_Adam(["mnasnet_tiny"], depth=3, step_size=0.005, steps=3, engine=hostsim_engine(),
                                              graph_builder=graphs.build_tiny, weight_seed=0)
    adv = atk(vid, torch.zeros(1, dtype=torch.long), ["t"])
    g = graphs.build_tiny("mnasnet_tiny", (64, 64))
    dg, dsd = mr.dense_twin(g, weights.synthetic_state_dict(g, 0))
    ref = restate.run_attack([restate.OracleNet(dg, dsd, [dg.hooks[3]])], vid, steps=3, step_size=0.005)
    np.testing.assert_allclose(atk.last_costs, ref["costs"], rtol=2e-4)
    assert float((adv - ref["adv"]).abs().mean()) < 5e-3
