"""CPU: the oracle against what the IMPORTED reference classes returned (oracle/ref_shim.py) for hook depths and AENS cases
outside the other fixtures -- captured by oracle/make_ref_live.py into tests/golden/ref_live_i2v.npz / ref_live_aens.npz."""
import numpy as np
import pytest
import torch

from oracle import restate
from tests import golden_util as gu

def live_hw(model):
    """Frame size of the single-frame hook-depth cases: 48 px, AlexNet 64 (the smallest its full feature stack accepts)."""
    return 64 if model == "alexnet" else 48


def _clip(seed, b, f, hw, dtype):
    from oracle.make_golden import make_clip, normalise
    return normalise(make_clip(seed, b, f, hw), dtype)


@pytest.mark.parametrize("model,depth", [("resnet", 1), ("resnet", 4), ("vgg", 3), ("vgg", 4),
                                         ("alexnet", 1), ("alexnet", 4), ("squeezenet", 1),
                                         ("squeezenet", 4)])
def test_i2v_live_f64(model, depth):
    """Hook depths not covered by the committed fixtures."""
    hw = live_hw(model)
    vid = _clip(31, 1, 1, hw, torch.float64)
    REF, k = gu.ref_live("i2v"), f"i2v_live/{model}_{depth}/"
    ref_cost, grad0, delta_last = REF[k + "cost"], torch.from_numpy(REF[k + "grad0"]), torch.from_numpy(REF[k + "delta_last"])
    adv = torch.from_numpy(REF[k + "adv"]).double()
    fx = dict(models=[model], depth=depth, hw=hw, wseed=5)
    (g, sd, hooks), = gu.hook_lists(fx)
    net = restate.OracleNet(g, sd, hooks, dtype=torch.float64)
    out = restate.run_attack([net], vid, steps=3, step_size=0.004, trace=True)
    np.testing.assert_allclose(out["costs"], ref_cost, rtol=2e-6)
    assert (grad0.double() - out["grad0"]).abs().max() <= 2e-6 * grad0.abs().max()
    assert (delta_last.double() - out["deltas"][-1]).abs().max() < 5e-6
    assert (adv - out["adv"]).abs().max() < 5e-5
    assert tuple(REF[k + "adv_shape"]) == vid.shape                                  # (b,3,f,h,w), image_attacks.py:362-363


def test_aens_coeffs_persist_across_calls():
    """`self.coeffs` lives on the object (TPAMI_attack.py:165,265)."""
    vid = _clip(41, 1, 2, 64, torch.float64)
    depths = {"resnet": [2, 3], "squeezenet": [2, 3]}
    REF = gu.ref_live("aens")
    w1, w2 = REF["aens_persist/w1"], REF["aens_persist/w2"]           # the reference object's weights after its 1st and 2nd call
    fx = dict(models=["resnet", "squeezenet"], depth=depths, hw=64, wseed=0)
    nets = [restate.OracleNet(g, sd, h, dtype=torch.float64) for g, sd, h in gu.hook_lists(fx)]
    c = torch.ones(4, dtype=torch.float64)
    o1 = restate.run_attack(nets, vid, steps=2, step_size=0.005, mode="aens", coeffs=c, momentum=1.0)
    o2 = restate.run_attack(nets, vid, steps=2, step_size=0.005, mode="aens", coeffs=o1["coeffs"],
                            momentum=1.0)
    np.testing.assert_allclose(np.stack(o1["weights"]), w1, rtol=1e-6)
    np.testing.assert_allclose(np.stack(o2["weights"]), w2, rtol=1e-6)


def test_aens_squeezenet_hooks_whole_fire_module_live():
    """With LIST depths the adaptive attack hooks `features[idx]` itself -- cat(expand1x1, expand3x3) -- not the 3x3
    branch the scalar-depth lookup takes (TPAMI_attack.py:195-199).  Gradient and output of the imported reference
    class against the oracle on the product's graph (`Graph.hook_for(d, whole_module=True)`); the coefficient
    weights alone would not notice the difference while cos ~ 1."""
    vid = _clip(52, 2, 1, 64, torch.float64)
    depths = {"squeezenet": [2, 3], "alexnet": [2, 3]}
    REF = gu.ref_live("aens")
    cost_saved, grad0 = REF["aens_squeezenet/cost_saved"], torch.from_numpy(REF["aens_squeezenet/grad0"])
    adv, ref_weights = torch.from_numpy(REF["aens_squeezenet/adv"]).double(), REF["aens_squeezenet/weights"]
    shapes = [tuple(s) for s in REF["aens_squeezenet/hook_shapes"]]          # last model's hooks: alexnet
    fx = dict(models=["squeezenet", "alexnet"], depth=depths, hw=64, wseed=3)
    lists = gu.hook_lists(fx)
    g, _, hooks = lists[0]
    e1 = g.tensors[g.hooks[2]].C
    assert [g.tensors[h].C for h in hooks] == [2 * e1, 2 * g.tensors[g.hooks[3]].C]      # both Fire branches
    nets = [restate.OracleNet(gg, sd, h, dtype=torch.float64) for gg, sd, h in lists]
    out = restate.run_attack(nets, vid, steps=3, step_size=0.005, mode="aens", coeffs=torch.ones(4, dtype=torch.float64),
                             momentum=0.5, trace=True)
    np.testing.assert_allclose(out["costs"], cost_saved, rtol=2e-6)
    assert (grad0.double() - out["grad0"]).abs().max() <= 2e-6 * grad0.abs().max()
    assert (adv - out["adv"]).abs().max() < 5e-5
    np.testing.assert_allclose(np.stack(out["weights"]), ref_weights, rtol=1e-6)
    assert len(shapes) == 2
