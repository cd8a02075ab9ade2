"""CPU: the torchvision ResNet family in the graph IR (names, key / shape contract, MACs, checkpoints) and the grouped convolution through
the planner on the host simulation, which runs grouped nodes on the dense route (block-diagonal weight through the ordinary packings)."""
import json
import os

import numpy as np
import pytest
import torch

from i2v_amd import attacks, graphs, weights
from oracle import restate
from tests import graph_dump_util as gd
from tests import make_resnet_family_fixtures as mk
from tests import resnet_family_reference as rf
from tests.hostsim_util import hostsim_engine
from tests.test_planner_hostsim import write_hook_grads

NEW_NAMES = tuple(mk.TV)


def test_new_names_are_the_issue_s():
    assert set(NEW_NAMES) == set(graphs.RESNET_FAMILY) == {"resnet18", "resnet34", "resnet152", "wide_resnet50_2", "wide_resnet101_2",
                                                            "resnext50_32x4d", "resnext101_32x8d"}
    for name in NEW_NAMES:
        assert graphs.build(name).arch == name


@pytest.mark.parametrize("name", NEW_NAMES)
def test_param_shapes_equal_the_torchvision_fixture(name):
    want = {k: tuple(v) for k, v in mk.expand_keys(json.load(open(mk.KEYS))[name]).items()}
    assert want == {k: tuple(v) for k, v in mk.torchvision_keys(*mk.TV[name]).items()}       # the fixture is what the stated rule gives
    assert graphs.build(name, (224, 224)).param_shapes() == want


def test_spot_shapes():
    x = graphs.build("resnext50_32x4d").param_shapes()
    assert x["layer1.0.conv2.weight"] == (128, 4, 3, 3)
    assert x["layer4.2.conv2.weight"] == (1024, 32, 3, 3)
    assert x["layer4.2.conv3.weight"] == (2048, 1024, 1, 1)
    assert graphs.build("wide_resnet50_2").param_shapes()["layer1.0.conv2.weight"] == (128, 128, 3, 3)
    r = graphs.build("resnet18").param_shapes()
    assert not any(k.startswith("layer1.0.downsample") for k in r)
    assert r["layer2.0.downsample.0.weight"] == (128, 64, 1, 1)
    widths = sorted({(nd.cin // nd.groups) for nd in graphs.build("resnext101_32x8d").nodes if nd.op == "conv" and nd.groups > 1})
    assert widths == [8, 16, 32, 64]
    t = graphs.build_tiny("resnext_tiny", (64, 64))
    gn = [(nd.cin // nd.groups, nd.stride, t.tensors[nd.dst].H) for nd in t.nodes if nd.op == "conv" and nd.groups > 1]
    assert gn == [(4, 1, 16), (4, 1, 16), (8, 2, 8), (16, 2, 4), (16, 1, 4), (32, 2, 2)]


@pytest.mark.parametrize("name", NEW_NAMES)
def test_macs_equal_the_reference_count(name):
    assert graphs.build(name, (224, 224)).macs_per_frame() == mk.reference_macs(*mk.TV[name])
    if name == "resnext50_32x4d":
        assert abs(graphs.build(name).macs_per_frame() / 4.26e9 - 1) < 0.01


def test_existing_names_build_the_graphs_they_built():
    want = json.load(open(gd.DUMP_PATH))
    got = gd.dump_all()
    assert sorted(got) == sorted(want)
    for key in want:
        assert got[key] == want[key], key
    for name in gd.EXISTING_NAMES:
        for g in (graphs.build(name), graphs.build_tiny(name)):
            assert all(getattr(nd, f) == v for nd in g.nodes for f, v in gd.NEW_FIELDS.items() if hasattr(nd, f)), name


def test_checkpoint_loads_and_a_bad_grouped_weight_is_refused(tmp_path, monkeypatch):
    g = graphs.build("resnext50_32x4d", (224, 224))
    full = {k: torch.zeros(*shp) for k, shp in mk.torchvision_keys(*mk.TV["resnext50_32x4d"]).items()}
    full.update({"fc.weight": torch.zeros(1000, 2048), "fc.bias": torch.zeros(1000), "bn1.num_batches_tracked": torch.tensor(0)})
    monkeypatch.setenv("I2V_WEIGHTS_DIR", str(tmp_path))
    torch.save(full, tmp_path / "resnext50_32x4d.pth")
    sd = weights.load_state_dict(g)
    assert set(sd) == set(g.param_shapes()) and sd["layer3.0.conv2.weight"].shape == (512, 16, 3, 3)
    bad = dict(full); bad["layer3.0.conv2.weight"] = torch.zeros(512, 512, 3, 3)        # a dense weight where the grouped one belongs
    torch.save(bad, tmp_path / "resnext50_32x4d.pth")
    with pytest.raises(ValueError, match="layer3.0.conv2.weight"):
        weights.load_state_dict(g)
    bad = dict(full); del bad["layer3.0.conv2.weight"]
    torch.save(bad, tmp_path / "resnext50_32x4d.pth")
    with pytest.raises(KeyError, match="layer3.0.conv2.weight"):
        weights.load_state_dict(g)
    syn = weights.synthetic_state_dict(g, 1)
    assert {k: tuple(v.shape) for k, v in syn.items()} == g.param_shapes()


@pytest.mark.parametrize("name", ["resnext_tiny", "resnet_basic_tiny"])
def test_twins_on_the_host_simulation_match_float64(name):
    """Hooks d = 1..4 and the input gradient, 2 frames of 64 x 64, at the bounds tests/test_planner_hostsim.py uses for resnet_tiny."""
    eng = hostsim_engine()
    g = graphs.build_tiny(name, (64, 64))
    sd = weights.synthetic_state_dict(g, 3)
    hooks = [g.hooks[d] for d in (1, 2, 3, 4)]
    N = 2
    net = eng.build_net(g, sd, hooks, N)
    x, hg = rf.case_inputs(name, g, N, hooks)
    ref = rf.FamilyRef(g, sd, hooks, torch.float64)
    feats, _ = ref.run(x)
    net.forward(x)
    for t, want in zip(hooks, feats):
        got = net.read_tensor(t, N).double()
        assert torch.allclose(got, want, rtol=1e-4, atol=max(1e-5, 1e-6 * float(want.abs().max())))
    write_hook_grads(net, feats, hg, N)
    gated = [h * (f > 0).to(h.dtype) for h, f in zip(hg, feats)]
    _, want = ref.run(x, gated)
    gx = torch.empty(N, 3, 64, 64)
    net.backward(gx)
    err = (gx.double() - want).abs().max() / want.abs().max()
    assert err < 1e-4, err


def test_grouped_entry_refuses_what_it_does_not_serve():
    import ctypes as C
    from i2v_amd import lib
    eng = hostsim_engine()
    capi, h = eng.capi, eng.h

    def attempt(cin, cout, groups, k=3, stride=1, pad=1, residual=-1):
        nid = C.c_int(); assert capi.i2v_net_create(h, C.byref(nid)) == 0
        b0, b1, t0, t1 = C.c_int(), C.c_int(), C.c_int(), C.c_int()
        ho = (8 + 2 * pad - k) // stride + 1
        assert capi.i2v_net_add_buffer(h, nid.value, cin, 8, 8, C.byref(b0)) == 0 and capi.i2v_net_add_buffer(h, nid.value, cout, ho, ho, C.byref(b1)) == 0
        assert capi.i2v_net_add_tensor(h, nid.value, b0.value, 0, cin, 0, C.byref(t0)) == 0 and capi.i2v_net_add_tensor(h, nid.value, b1.value, 0, cout, 1, C.byref(t1)) == 0
        d = lib.ConvDesc(t0.value, t1.value, cin, cout, k, k, stride, pad, 1, t1.value if residual >= 0 else -1)
        w = np.zeros((cout, max(1, cin // max(groups, 1)), k, k), np.float32); s = np.ones(cout, np.float32)
        rc = capi.i2v_net_add_conv_grouped(h, nid.value, C.byref(d), groups, w.ctypes.data, s.ctypes.data, s.ctypes.data)
        msg = capi.i2v_last_error().decode() if rc else ""
        capi.i2v_net_destroy(h, nid.value)
        return rc, msg
    assert attempt(16, 16, 2)[0] == 0 and attempt(16, 16, 1)[0] == 0 and attempt(16, 16, 2, stride=2)[0] == 0
    for args, word in (((18, 16, 4), "divisible"), ((16, 18, 4), "divisible"), ((16, 16, 2, 1, 1, 0), "3x3"), ((16, 16, 2, 3, 3, 1), "3x3"),
                       ((16, 16, 16), "group width"), ((24, 24, 2), "group width"), ((16, 32, 2), "group width"), ((16, 16, 2, 3, 1, 1, 0), "residual")):
        rc, msg = attempt(*args)
        assert rc != 0 and word in msg, (args, msg)


def test_i2v_trajectory_on_resnext_tiny_matches_the_oracle():
    """3 steps of the I2V attack.  `oracle.restate` has no `groups`; it is handed the dense twin of the graph (every grouped convolution
    as a dense one on the block-diagonal weight: the same function) and runs its own loop unchanged.  On the host simulation the
    engine runs the block-diagonal route too, so both sides share the expansion: this test pins the attack loop, not the grouping
    convention.  That is pinned by test_twins_on_the_host_simulation_match_float64, against F.conv2d(groups=)."""
    torch.manual_seed(5)
    vid = torch.randn(1, 3, 2, 64, 64)
    atk = attacks.ImageGuidedFMDirection_Adam(["resnext_tiny"], depth=3, step_size=0.005, steps=3, engine=hostsim_engine(),
                                              graph_builder=graphs.build_tiny, weight_seed=0)
    adv = atk(vid, torch.zeros(1, dtype=torch.long), ["t"])
    g = graphs.build_tiny("resnext_tiny", (64, 64))
    dg, dsd = rf.dense_twin(g, weights.synthetic_state_dict(g, 0))
    ref = restate.run_attack([restate.OracleNet(dg, dsd, [dg.hooks[3]])], vid, steps=3, step_size=0.005)
    np.testing.assert_allclose(atk.last_costs, ref["costs"], rtol=2e-4)
    assert float((adv - ref["adv"]).abs().mean()) < 5e-3
