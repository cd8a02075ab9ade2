"""CPU: timm's SE-ResNet / SE-ResNeXt family in the graph IR (names, key / shape contract, hooks, MACs, checkpoints) and the
squeeze-and-excitation node through the planner on the host simulation, which runs the node as scalar code with the kernels' arithmetic
order (csrc/i2v_se_host.h).

The bound is relative L2 against float64: the larger of 1e-5 and 4 x the error of the float32 CPU run of the same reference on the same
inputs, read from tests/golden/seresnet_fp32_cpu_errors.json (tests/make_seresnet_fixtures.py) -- DESIGN.md sections 14 to 17."""
import json

import numpy as np
import pytest
import torch

from i2v_amd import attacks, graphs, lib, weights
from oracle import restate
from tests import graph_dump_util as gd
from tests import make_seresnet_fixtures as mk
from tests import seresnet_reference as sr
from tests.hostsim_util import hostsim_engine
from tests.test_planner_hostsim import write_hook_grads

NAMES = tuple(mk.TIMM)
FP32 = json.load(open(mk.ERRS))
FLOOR = 1e-5
SERVED = "seresnet18, seresnet34, seresnet50, seresnet101, seresnet152, seresnext50_32x4d, seresnext101_32x4d, seresnext101_32x8d"


def bound(fp32_err):
    return max(FLOOR, 4.0 * fp32_err)


def test_names_are_the_issue_s():
    assert ", ".join(NAMES) == ", ".join(graphs.SERESNET_FAMILY) == SERVED
    for name in NAMES:
        assert graphs.build(name).arch == name


@pytest.mark.parametrize("name", NAMES)
def test_param_shapes_equal_the_fixture(name):
    want = {k: tuple(v) for k, v in mk.expand_keys(json.load(open(mk.KEYS))[name]).items()}
    assert want == {k: tuple(v) for k, v in mk.timm_keys(name).items()}          # the fixture is what the stated rule gives
    assert graphs.build(name, (224, 224)).param_shapes() == want


def test_spot_shapes_and_reduced_widths():
    assert [graphs.se_reduced_width(c) for c in (64, 128, 256, 512, 1024, 2048)] == [8, 8, 16, 32, 64, 128]
    assert [mk.se_rd(c) for c in (64, 128, 256, 512, 1024, 2048)] == [8, 8, 16, 32, 64, 128]
    x = graphs.build("seresnet50").param_shapes()
    assert x["layer1.0.se.fc1.weight"] == (16, 256, 1, 1) and x["layer1.0.se.fc1.bias"] == (16,)
    assert x["layer4.2.se.fc2.weight"] == (2048, 128, 1, 1) and x["layer4.2.se.fc2.bias"] == (2048,)
    assert x["layer2.0.downsample.0.weight"] == (512, 256, 1, 1) and x["layer2.0.conv2.weight"] == (128, 128, 3, 3)
    assert graphs.build("seresnext50_32x4d").param_shapes()["layer1.0.conv2.weight"] == (128, 4, 3, 3)
    assert graphs.build("seresnet18").param_shapes()["layer1.0.se.fc1.weight"] == (8, 64, 1, 1)
    g = graphs.build("seresnet50")
    assert sum(1 for nd in g.nodes if nd.op == "se") == 16
    for nd in g.nodes:          # the node sits behind the block's last, linear, convolution and carries the shortcut and the ReLU
        if nd.op == "se":
            assert not g.tensors[nd.src].post_relu and g.tensors[nd.dst].post_relu and nd.relu and nd.residual is not None
    for tiny in ("seresnet_tiny", "seresnext_tiny"):
        t = graphs.build_tiny(tiny, (64, 64))
        assert t.tensors[t.hooks[4]].H == 2 and sum(1 for nd in t.nodes if nd.op == "se") == 6
    assert any(nd.op == "conv" and nd.groups == 4 for nd in graphs.build_tiny("seresnext_tiny").nodes)


@pytest.mark.parametrize("name", NAMES)
def test_hook_shapes_at_depths_1_to_4(name):
    g = graphs.build(name, (224, 224))
    want = mk.hook_shapes(name)
    for d in (1, 2, 3, 4):
        t = g.tensors[g.hook_for(d)]
        assert (t.C, t.H, t.W) == want[d] and t.post_relu
        assert g.truncated([g.hook_for(d)]).nodes[-1].op == "se"
    if name == "seresnet50":
        assert want == {1: (256, 56, 56), 2: (512, 28, 28), 3: (1024, 14, 14), 4: (2048, 7, 7)}


@pytest.mark.parametrize("name", NAMES)
def test_macs_equal_the_reference_count(name):
    g = graphs.build(name, (224, 224))
    assert g.macs_per_frame() == mk.reference_macs(name)
    plain = {"seresnet50": "resnet50", "seresnet18": "resnet18", "seresnext50_32x4d": "resnext50_32x4d"}.get(name)
    if plain:                   # the plain net's count plus 2 C rd per node, nothing per position
        assert g.macs_per_frame() == graphs.build(plain).macs_per_frame() + sum(2 * nd.C * nd.rd for nd in g.nodes if nd.op == "se")


def test_refused_names_list_the_served_ones():
    for name, word in (("seresnet50d", "three-convolution stem"), ("seresnext26d_32x4d", "average-pool downsample"), ("seresnext26t_32x4d", "deep-stem"),
                       ("seresnet152d", "deep-stem"), ("legacy_senet154", "group width 8"), ("senet154", "group width 8"), ("legacy_seresnet50", "legacy_se"),
                       ("seresnet200", "not served"), ("seresnext101_64x4d", "not served")):
        with pytest.raises(ValueError, match=word) as e:
            graphs.build(name)
        assert SERVED in str(e.value), name
    with pytest.raises(ValueError, match="SiLU and squeeze-excite"):         # still true: SiLU is missing
        graphs.build("efficientnet_b0")


def test_checkpoint_loads_and_a_bad_se_weight_is_refused(tmp_path, monkeypatch):
    g = graphs.build("seresnet50", (224, 224))
    full = {k: torch.zeros(*shp) for k, shp in mk.timm_keys("seresnet50").items()}
    full.update({"fc.weight": torch.zeros(1000, 2048), "fc.bias": torch.zeros(1000), "bn1.num_batches_tracked": torch.tensor(0)})
    monkeypatch.setenv("I2V_WEIGHTS_DIR", str(tmp_path))
    torch.save(full, tmp_path / "seresnet50.pth")
    sd = weights.load_state_dict(g)
    assert set(sd) == set(g.param_shapes()) and sd["layer3.0.se.fc1.weight"].shape == (64, 1024, 1, 1)
    bad = dict(full); bad["layer3.0.se.fc1.weight"] = torch.zeros(1024 // 16 + 8, 1024, 1, 1)
    torch.save(bad, tmp_path / "seresnet50.pth")
    with pytest.raises(ValueError, match="layer3.0.se.fc1.weight"):
        weights.load_state_dict(g)
    syn = weights.synthetic_state_dict(g, 1)
    assert {k: tuple(v.shape) for k, v in syn.items()} == g.param_shapes()


def test_existing_names_build_the_graphs_they_built():
    want = json.load(open(gd.DUMP_PATH))
    got = gd.dump_all()
    assert sorted(got) == sorted(want)
    for key in want:
        assert got[key] == want[key], key
    for name in ("resnet18", "resnext50_32x4d", "mnasnet1_0"):
        assert all(nd.op != "se" for nd in graphs.build(name).nodes)


# ---- the host simulation ----
CASES = [mk.node_case(c) for c in sr.NODE_CASES] + [mk.net_case("seresnet_tiny"), mk.net_case("seresnext_tiny")]
_REF = {}


def reference(tag, g, sd, hooks, frames):
    """Inputs and float64 results of a case, computed once per module run: (x, gated hook gradients, features, input gradient)."""
    if tag not in _REF:
        x, hg = sr.case_inputs(tag, g, frames, hooks)
        f64, gated, g64, _ = sr.reference(g, sd, hooks, x, hg)
        _REF[tag] = (x, gated, f64, g64)
    return _REF[tag]


def run_net(eng, g, sd, hooks, x, gated, f64):
    N = x.shape[0]
    net = eng.build_net(g, sd, hooks, N)
    net.forward(x)
    feats = [net.read_tensor(t, N).clone() for t in hooks]
    write_hook_grads(net, [torch.ones_like(f) for f in f64], gated, N)       # (the gradients are gated already: gate of ones)
    gx = torch.empty(N, 3, x.shape[2], x.shape[3])
    net.backward(gx)
    net.close()
    return feats, gx


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_inputs_keep_a_dead_gate_from_passing(case):
    """The condition on the inputs, in the reference alone: gates of constant 0.5 miss the true features by more than 100 x the bound,
    and the true gates span at least 0.2 .. 0.8."""
    tag, g, sd, hooks, frames = case
    x, _, _, _ = reference(tag, g, sd, hooks, frames)
    dist, lo, hi = sr.gate_condition(g, sd, hooks, x)
    print(tag, "constant-gate distance", dist, "gates", lo, hi)
    for i, d in enumerate(dist):
        assert d > 100.0 * bound(FP32[tag]["hooks"][i]), (tag, i, d)
    assert lo <= 0.2 and hi >= 0.8, (lo, hi)


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_host_simulation_matches_float64(case, monkeypatch):
    """Features and input gradient within the bound; a rerun has the same bits; frame 0 of the run has the bits of a 1-frame run."""
    monkeypatch.setenv("I2V_AUTOTUNE", "0")
    tag, g, sd, hooks, frames = case
    assert sr.n_se(g, hooks) >= 1
    eng = hostsim_engine()
    x, gated, f64, g64 = reference(tag, g, sd, hooks, frames)
    a = run_net(eng, g, sd, hooks, x, gated, f64)
    b = run_net(eng, g, sd, hooks, x, gated, f64)
    one = run_net(eng, g, sd, hooks, x[:1], [h[:1] for h in gated], [f[:1] for f in f64])
    for i in range(len(hooks)):
        e, bd = sr.rel_l2(a[0][i], f64[i]), bound(FP32[tag]["hooks"][i])
        print(f"{tag} hook {i}: host {e:.3e} fp32-cpu {FP32[tag]['hooks'][i]:.3e} bound {bd:.3e}")
        assert e <= bd
        assert torch.equal(a[0][i], b[0][i]) and torch.equal(a[0][i][:1], one[0][i])
    e, bd = sr.rel_l2(a[1], g64), bound(FP32[tag]["gx"])
    print(f"{tag} gx: host {e:.3e} fp32-cpu {FP32[tag]['gx']:.3e} bound {bd:.3e}")
    assert e <= bd
    assert torch.equal(a[1], b[1]) and torch.equal(a[1][:1], one[1])


def test_i2v_trajectory_on_seresnet_tiny_matches_the_reference():
    """4 steps of the I2V attack at depth 3 against `restate.run_attack` on the float32 reference net (costs at rtol 2e-4, as the
    MNASNet test)."""
    torch.manual_seed(5)
    vid = torch.randn(1, 3, 2, 64, 64)
    atk = attacks.ImageGuidedFMDirection_Adam(["seresnet_tiny"], depth=3, step_size=0.005, steps=4, engine=hostsim_engine(),
                                              graph_builder=graphs.build_tiny, weight_seed=0)
    adv = atk(vid, torch.zeros(1, dtype=torch.long), ["t"])
    g = graphs.build_tiny("seresnet_tiny", (64, 64))
    ref = restate.run_attack([sr.SeRef(g, weights.synthetic_state_dict(g, 0), [g.hooks[3]], dtype=torch.float32)], vid, steps=4, step_size=0.005)
    np.testing.assert_allclose(atk.last_costs, ref["costs"], rtol=2e-4)
    assert float((adv - ref["adv"]).abs().mean()) < 5e-3


def test_plan_refuses_a_second_consumer_of_the_se_source():
    """stem -> a -> b (linear); b feeds the SE node AND a 1x1 convolution: the node writes b's gradient, it cannot accumulate."""
    g = graphs.Graph("se_two_consumers", (8, 8))
    x = g.new_tensor(3, 8, 8, False, "input")
    g.input = x
    a = g.conv(x, 8, 3, 1, 1, "stem.weight", bn="stem_bn", relu=True, name="stem")
    b = g.conv(a, 8, 1, 1, 0, "lin.weight", bn="lin_bn", relu=False, name="lin")
    y = g.se(b, 8, "se", relu=True, residual=a, name="out")
    z = g.conv(b, 8, 1, 1, 0, "side.weight", bn="side_bn", relu=False, residual=y, name="side")
    g.hooks[1] = z
    with pytest.raises(lib.I2VError, match=f"tensor {b}\\) must have the node as its only consumer"):
        hostsim_engine().build_net(g, weights.synthetic_state_dict(g, 0), [z], 1)


def test_se_entry_refuses_what_it_does_not_serve():
    import ctypes as C
    eng = hostsim_engine()
    capi, h = eng.capi, eng.h

    def attempt(C_=16, rd=8, dst_c=16, dst_hw=8, res_c=None, T=1, src_relu=0):
        nid = C.c_int(); assert capi.i2v_net_create(h, C.byref(nid)) == 0
        ids = []
        for ch, hw, relu in ((16, 8, src_relu), (dst_c, dst_hw, 1), (res_c or 16, 8, 0)):
            b, t = C.c_int(), C.c_int()
            assert capi.i2v_net_add_buffer3d(h, nid.value, ch, T, hw, hw, C.byref(b)) == 0
            assert capi.i2v_net_add_tensor(h, nid.value, b.value, 0, ch, relu, C.byref(t)) == 0
            ids.append(t.value)
        d = lib.SeDesc(ids[0], ids[1], ids[2] if res_c else -1, C_, rd, 1)
        w1, w2 = np.zeros((max(rd, 1), C_), np.float32), np.zeros((C_, max(rd, 1)), np.float32)
        b1, b2 = np.zeros(max(rd, 1), np.float32), np.zeros(C_, np.float32)
        rc = capi.i2v_net_add_se(h, nid.value, C.byref(d), w1.ctypes.data, b1.ctypes.data, w2.ctypes.data, b2.ctypes.data)
        msg = capi.i2v_last_error().decode() if rc else ""
        capi.i2v_net_destroy(h, nid.value)
        return rc, msg

    assert attempt()[0] == 0 and attempt(res_c=16)[0] == 0
    for kwargs, word in ((dict(C_=32), "channels"), (dict(dst_c=32), "channels"), (dict(rd=0), "rd = 0"), (dict(dst_hw=4), "differ"),
                         (dict(res_c=8), "residual shape"), (dict(T=2), "video"), (dict(src_relu=1), "linear output")):
        rc, msg = attempt(**kwargs)
        assert rc != 0 and word in msg and "i2v_net_add_se" in msg, (kwargs, msg)
