"""Planner side of the shortcut pair (`mark_fusable` -> `k_conv_scpair`), on the host simulation: which pairs ResNet-50 to layer3 gets,
that running them changes no bit of any hooked feature or of the input gradient, and what the timing records say about them.  The host
backend runs a pair as its two launches and then POISONS the intermediate with NaN, as the device kernel never stores it: a reader
the planner overlooked would show up here as a non-finite result."""
import pytest
import torch

from i2v_amd import graphs, weights
from tests.hostsim_util import hostsim_engine
from tests.test_planner_hostsim import write_hook_grads


def tensor_named(g, suffix):
    return next(i for i, t in enumerate(g.tensors) if (t.name or "").endswith(suffix))


@pytest.fixture(scope="module")
def resnet50():
    g = graphs.build("resnet50", (32, 32))
    return g, weights.synthetic_state_dict(g, 0)


def run(eng, g, sd, hooks, timing=False):
    """Plan for 2 frames, forward and backward: (features per hook, input gradient, pair info, fusion info, shortcut read-back, timing)."""
    x = torch.randn(2, 3, 32, 32, generator=torch.Generator().manual_seed(0))
    net = eng.build_net(g, sd, hooks, 2)
    info, fusion = net.scpair_info(), net.fusion_info()
    if timing:
        eng.timing_enable(True)
    net.forward(x)
    feats = [net.save_hook(i, 2).clone() for i in range(len(hooks))]
    write_hook_grads(net, feats, [torch.randn(f.shape, generator=torch.Generator().manual_seed(1 + i)) for i, f in enumerate(feats)], 2)
    gx = torch.empty(2, 3, 32, 32)
    net.backward(gx)
    kt = eng.timing_collect() if timing else None
    if timing:
        eng.timing_enable(False)
    shortcut = net.read_tensor(tensor_named(g, "layer1.0.downsample"), 2).clone()
    net.close()
    return feats, gx, info, fusion, shortcut, kt


def test_pairs_of_resnet50_are_found_and_change_nothing(resnet50, monkeypatch):
    """Forward: the first bottleneck of layer1, layer2 and layer3 (shortcut + expand).  Backward: layer1.0 alone, where the shortcut's
    input gradient is conv1's plain addend on the same grid; the strided blocks' shortcut gradients are compact addends and stay launches."""
    eng = hostsim_engine()
    g, sd = resnet50
    hooks = [g.hooks[1], g.hooks[2], g.hooks[3]]
    monkeypatch.delenv("I2V_SCPAIR", raising=False)
    fused = run(eng, g, sd, hooks)
    monkeypatch.setenv("I2V_SCPAIR", "0")
    plain = run(eng, g, sd, hooks)
    assert fused[2] == (3, 1, 3, 1) and plain[2] == (0, 0, 0, 0), (fused[2], plain[2])
    assert fused[3] == plain[3] == (6, 6, 0, 0)                       # the 3x3 -> pointwise pairs: untouched
    for a, b in zip(fused[0], plain[0]):
        assert torch.equal(a, b) and bool(torch.isfinite(a).all())
    assert torch.equal(fused[1], plain[1]) and bool(torch.isfinite(fused[1]).all())
    # the forward shortcut's output is never stored (here: poisoned), yet reads back -- produced on demand -- with the same bits
    assert torch.equal(fused[4], plain[4]) and bool(torch.isfinite(fused[4]).all())


def test_a_hook_on_the_shortcut_output_keeps_its_pair_out(resnet50, monkeypatch):
    eng = hostsim_engine()
    g, sd = resnet50
    monkeypatch.delenv("I2V_SCPAIR", raising=False)
    t_sc = tensor_named(g, "layer1.0.downsample")
    net = eng.build_net(g, sd, [g.hooks[3], t_sc], 2)
    assert net.scpair_info()[0] == 2
    assert net.fusion_info()[:2] == (6, 6)
    x = torch.randn(2, 3, 32, 32, generator=torch.Generator().manual_seed(0))
    net.forward(x)
    assert bool(torch.isfinite(net.save_hook(1, 2)).all())
    net.close()


def test_pairs_run_together_with_forced_3x3_pairs(resnet50, monkeypatch):
    """layer1.0's expand convolution is also the second half of a 3x3 -> pointwise pair: where that pair is forced, it runs and the
    shortcut stays a launch of its own; results are the same bits either way."""
    eng = hostsim_engine()
    g, sd = resnet50
    monkeypatch.delenv("I2V_SCPAIR", raising=False)
    base = run(eng, g, sd, [g.hooks[3]])
    monkeypatch.setenv("I2V_FORCE_FUSE", "1")
    both = run(eng, g, sd, [g.hooks[3]])
    assert both[3] == (6, 6, 6, 6) and both[2][:2] == (3, 1)
    assert torch.equal(base[0][0], both[0][0]) and torch.equal(base[1], both[1])
    assert bool(torch.isfinite(both[0][0]).all()) and bool(torch.isfinite(both[1]).all())


def test_a_pair_is_timed_once_with_both_halves(resnet50, monkeypatch):
    """Timing mode: a pair is ONE launch of its kind carrying the flops of both halves and the algorithmic bytes without the
    intermediate, which the two launches write once and read once."""
    eng = hostsim_engine()
    g, sd = resnet50
    monkeypatch.delenv("I2V_SCPAIR", raising=False)
    fused = run(eng, g, sd, [g.hooks[3]], timing=True)[5]
    monkeypatch.setenv("I2V_SCPAIR", "0")
    plain = run(eng, g, sd, [g.hooks[3]], timing=True)[5]
    # intermediates at 32 x 32 input, 2 frames: layer1.0 256 x 8 x 8, layer2.0 512 x 4 x 4, layer3.0 1024 x 2 x 2; backward 64 x 8 x 8
    inter = {"conv_igemm_fwd": 2 * (256 * 64 + 512 * 16 + 1024 * 4), "conv_igemm_dgrad": 2 * 64 * 64}
    pairs = {"conv_igemm_fwd": 3, "conv_igemm_dgrad": 1}
    for kind in inter:
        assert int(plain[kind]["launches"]) - int(fused[kind]["launches"]) == pairs[kind]
        assert fused[kind]["flops"] == plain[kind]["flops"]
        assert plain[kind]["bytes"] - fused[kind]["bytes"] == 2 * 4 * inter[kind]
