"""GPU (-m gpu): timm's CaiT on the MI355X (include/i2v_cait.h) -- the talking-heads attention kernel on its own,
forward and backward, against float64 autograd on the six shapes of tests/make_cait_fixtures.ATTN_CASES; the test-size twin,
cait_xxs24_224 and cait_s24_224 against the float64 reference (tests/cait_reference.py); repeatability; frame 0 of an n-frame call
against a 1-frame call; a 10-step I2V trajectory and an AENS ensemble against `oracle.restate.run_attack`; the workspace figure.

Bound: relative L2 against float64, at most the larger of the floor for that kind of case (attention entries 1e-6 forward and 1e-5
backward; nets 1e-5) and 4 x the error of the float32 CPU run of the same reference on the same inputs
(tests/golden/cait_fp32_cpu_errors.json, tests/make_cait_fixtures.py).  A case without a recorded error fails (KeyError)."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from i2v_amd import attacks, graphs, weights
from oracle import restate
from tests import make_cait_fixtures as mk
from tests.cait_reference import CaitReference
from tests.family_harness import bound, check_net, check_trajectory, hooks_and_grad, rand as _rand, rel as _rel, run_net as _run, stat, video as _video

pytestmark = pytest.mark.gpu
S24, XXS = "cait_s24_224", "cait_xxs24_224"
FP32 = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cait_fp32_cpu_errors.json")))
NET_FLOOR, FWD_FLOOR, BWD_FLOOR = 1e-5, 1e-6, 1e-5
COUNTER = b"cait_attention_launches"
TRAJECTORY_RTOL = 2e-4      # of the trajectory's costs against the float64 run


@pytest.fixture(scope="module")
def eng():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return attacks.get_engine("cuda:0")


def run_attn(eng, d):
    """(out, probs (F, H, T, T), dqkv) of an attention case through the two C entries, back on the host."""
    c = {k: (v.float().cuda().contiguous() if torch.is_tensor(v) else v) for k, v in d.items()}
    out, probs = eng.cait_attention(c["qkv"], c["heads"], c["scale"], c["wl"], c["bl"], c["ww"], c["bw"])
    dqkv = eng.cait_attention_bwd(c["qkv"], probs, c["dout"], c["heads"], c["scale"], c["wl"], c["ww"], c["bw"])
    torch.cuda.synchronize()
    return out.cpu(), probs[..., :c["qkv"].shape[1]].cpu(), dqkv.cpu()


@pytest.mark.parametrize("F,T,H,dh", mk.ATTN_CASES)
def test_attention_kernel_against_float64_autograd(eng, F, T, H, dh):
    d = mk.attn_case(F, T, H, dh)
    s0 = stat(eng, COUNTER)
    out, probs, dqkv = run_attn(eng, d)
    assert stat(eng, COUNTER) - s0 == 3                                            # one launch forward, two backward
    want, want_p, want_g = mk.attn_reference(d)
    fp = FP32["attention"][mk.case_key(F, T, H, dh)]
    e_f, e_p, e_b = _rel(out, want), _rel(probs, want_p), _rel(dqkv, want_g)
    print(f"attention F {F} T {T} H {H} dh {dh}: out {e_f:.3e} (fp32 CPU {fp['fwd']:.3e}) probs {e_p:.3e} ({fp['probs']:.3e}) "
          f"dqkv {e_b:.3e} ({fp['bwd']:.3e})")
    assert e_f < bound(fp["fwd"], FWD_FLOOR) and e_p < bound(fp["probs"], FWD_FLOOR) and e_b < bound(fp["bwd"], BWD_FLOOR)
    out2, probs2, dqkv2 = run_attn(eng, d)
    assert torch.equal(out, out2) and torch.equal(probs, probs2) and torch.equal(dqkv, dqkv2)      # reruns: the same bits
    if F > 1:                                                             # frame 0 of the F-frame call: the bits of a 1-frame call
        o1, p1, g1 = run_attn(eng, {k: (v[:1] if torch.is_tensor(v) and v.dim() == 3 else v) for k, v in d.items()})
        assert torch.equal(out[:1], o1) and torch.equal(probs[:1], p1) and torch.equal(dqkv[:1], g1)


def test_the_launch_refuses_what_it_cannot_run(eng):
    z = torch.zeros(4096, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())      # noqa: E731
    capi = eng.capi
    s0 = stat(eng, COUNTER)
    fwd = lambda *, frames=1, T=4, H=2, dh=8: capi.i2v_cait_attention_f32(p(z), frames, T, H, dh, 0.5, p(z), p(z), p(z), p(z), p(z), p(z), None)      # noqa: E731
    for kw, why in ((dict(dh=6), b"multiple of 4"), (dict(H=17, dh=4), b"LDS budget"), (dict(T=400, H=8, dh=4), b"LDS budget"),
                    (dict(frames=70000), b"65535"), (dict(frames=40000, T=196, H=8, dh=48), b"2^31")):
        assert fwd(**kw) != 0
        err = capi.i2v_last_error()
        assert b"cait_attention" in err and b"hipErrorInvalidValue" in err and why in err, err
    assert capi.i2v_cait_attention_bwd_f32(p(z), p(z), p(z), 1, 4, 2, 6, 0.5, p(z), p(z), p(z), p(z), p(z), p(z), None) != 0
    assert b"multiple of 4" in capi.i2v_last_error()
    assert stat(eng, COUNTER) == s0                                                # nothing was launched


def _hooks_and_grad(eng, spec, sd, blocks, x, max_frames=None):
    launches = 3 * (max(blocks) + 1)      # per block: one attention launch forward, two backward
    return hooks_and_grad(eng, spec, sd, blocks, x, max_frames, launches=(COUNTER, launches))


def _check(label, feats, gx, ref, x, hg):
    check_net(label, feats, gx, ref.forward(x), ref.backward(hg), FP32[label], NET_FLOOR)


@pytest.mark.parametrize("label", sorted(mk.TWINS))
def test_twin_hooks_at_depths_1_to_4_and_input_gradient(eng, label):
    side = mk.TWINS[label][0]
    spec = graphs.build_tiny(S24, (side, side))
    sd = weights.synthetic_state_dict(spec, 0)
    x = mk.twin_input(label)
    blocks = [spec.hook_for(d) for d in (1, 2, 3, 4)]
    assert blocks == mk.TWIN_HOOKS
    (feats, gx), hg = _hooks_and_grad(eng, spec, sd, blocks, x)
    _check(label, feats, gx, CaitReference(spec, sd, blocks), x, hg)
    (feats2, gx2), _ = _hooks_and_grad(eng, spec, sd, blocks, x, max_frames=5)     # a second net, planned for more frames: the same bits
    assert all(torch.equal(a, b) for a, b in zip(feats, feats2)) and torch.equal(gx, gx2)
    net = eng.build_cait_net(spec, sd, blocks, 1)                                  # frame 0 of the n-frame run against a 1-frame run
    f1, g1, _ = _run(net, spec, blocks, x[:1], [h[:1] for h in hg])
    net.close()
    assert all(torch.equal(a[:1], b) for a, b in zip(feats, f1)) and torch.equal(gx[:1], g1)
    (fa, _), _ = _hooks_and_grad(eng, spec, sd, [blocks[1]], x)                    # a single mid-stack hook: the net is truncated there
    assert torch.equal(fa[0], feats[1])


@pytest.mark.parametrize("name", [XXS, S24])
def test_full_size_model_at_224_depths_1_to_4_against_float64(eng, name):
    spec = graphs.build(name)
    sd = weights.synthetic_state_dict(spec, 0)
    x = _rand(2, 3, 224, 224, seed=22)
    blocks = [spec.hook_for(d) for d in (1, 2, 3, 4)]
    assert blocks == mk.FULL[name]
    (feats, gx), hg = _hooks_and_grad(eng, spec, sd, blocks, x)
    _check(name, feats, gx, CaitReference(spec, sd, blocks), x, hg)


def test_i2v_trajectory_on_the_twin_matches_the_float64_trajectory():
    vid = _video(2, 4, 64, 23)
    atk = attacks.ImageGuidedFMDirection_Adam([S24], depth=3, step_size=0.005, steps=10, graph_builder=graphs.build_tiny, weight_seed=0)
    adv = atk(vid, torch.zeros(2, dtype=torch.long), ["a", "b"]).cpu()
    spec = graphs.build_tiny(S24, (64, 64))
    check_trajectory(atk, adv, CaitReference(spec, weights.synthetic_state_dict(spec, 0), [spec.hook_for(3)], dtype=torch.float64), vid, rtol=TRAJECTORY_RTOL)


def test_aens_of_the_twin_with_tiny_resnet_matches_the_oracle():
    vid = _video(1, 4, 64, 24)
    depths = {S24: [1, 4], "resnet": [2, 3]}
    atk = attacks.AENS_I2V_MF([S24, "resnet"], depths=depths, step_size=0.005, steps=4, momentum=0.5, graph_builder=graphs.build_tiny,
                              weight_seed=0)
    adv, _, costs = atk(vid, torch.zeros(1, dtype=torch.long), ["a"])
    cs, rs = (graphs.build_tiny(n, (64, 64)) for n in (S24, "resnet"))
    nets = [CaitReference(cs, weights.synthetic_state_dict(cs, 0), [cs.hook_for(d) for d in depths[S24]], dtype=torch.float64),
            restate.OracleNet(rs, weights.synthetic_state_dict(rs, 0), [rs.hook_for(d, True) for d in depths["resnet"]], dtype=torch.float64)]
    ref = restate.run_attack(nets, vid, steps=4, step_size=0.005, mode="aens", coeffs=torch.ones(4, dtype=torch.float64), momentum=0.5)
    np.testing.assert_allclose(costs, ref["costs"], rtol=2e-4)


def test_workspace_of_cait_s24_at_128_frames_depth_3(eng):
    """The plan the device holds equals the formula the host simulation's plan is checked against (tests/test_cait_cpu.py) and the
    figure of DESIGN.md section 21."""
    spec = graphs.build(S24)
    net = eng.build_cait_net(spec, weights.synthetic_state_dict(spec, 0), [spec.hook_for(3)], 128)
    got = net.workspace_bytes()
    net.close()
    assert got == spec.workspace_bytes([17], 128) == 10_027_172_480
