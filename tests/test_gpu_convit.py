"""GPU (-m gpu): timm's ConViT on the MI355X (include/i2v_convit.h) -- the gated positional attention kernel on its
own, forward, probs and backward, against float64 autograd on the shapes of tests/make_convit_fixtures.ATTN_CASES with a random
non-negative table (and without one behind the join); both test-size twins, convit_tiny and convit_small against the float64 reference
(tests/convit_reference.py, timm's literal arithmetic); repeatability; frame 0 of an n-frame call against a 1-frame call; the launch
counter; a 10-step I2V trajectory and an AENS ensemble against `oracle.restate.run_attack`; refusals; the workspace figure.

Bound: relative L2 against float64, at most the larger of the floor for that kind of case (attention entries 1e-6 forward and on probs,
1e-5 backward; nets 1e-5) and 4 x the error of the float32 CPU run of the same reference on the same inputs
(tests/golden/convit_fp32_cpu_errors.json, tests/make_convit_fixtures.py).  A case without a recorded error fails (KeyError)."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from i2v_amd import attacks, graphs, weights
from oracle import restate
from tests import make_convit_fixtures as mk
from tests.convit_reference import ConvitReference
from tests.family_harness import bound, check_net, check_trajectory, hooks_and_grad, rand as _rand, rel as _rel, run_net as _run, stat, video as _video

pytestmark = pytest.mark.gpu
TINY, SMALL = "convit_tiny", "convit_small"
FP32 = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "convit_fp32_cpu_errors.json")))
NET_FLOOR, FWD_FLOOR, BWD_FLOOR = 1e-5, 1e-6, 1e-5
COUNTER = b"convit_attention_launches"
TRAJECTORY_RTOL = 2e-4      # of the trajectory's costs against the float64 run


@pytest.fixture(scope="module")
def eng():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return attacks.get_engine("cuda:0")


def _pad(table):
    """(H, T, T) -> (H, T, ld) float32 on the device, rows zero-padded"""
    if table is None:
        return None
    H, T, _ = table.shape
    out = torch.zeros(H, T, (T + 3) // 4 * 4, dtype=torch.float32)
    out[:, :, :T] = table.float()
    return out.cuda().contiguous()


def run_attn(eng, d):
    """(out, probs (F, H, T, T), dqkv) of an attention case through the two C entries, back on the host."""
    f = lambda v: v.float().cuda().contiguous()      # noqa: E731
    qkv, c, table = f(d["qkv"]), (None if d["c"] is None else f(d["c"])), _pad(d["table"])
    out, probs = eng.convit_attention(qkv, d["heads"], d["scale"], c, table)
    dqkv = eng.convit_attention_bwd(qkv, probs, f(d["dout"]), d["heads"], d["scale"], c, table)
    torch.cuda.synchronize()
    return out.cpu(), probs[..., :qkv.shape[1]].cpu(), dqkv.cpu()


@pytest.mark.parametrize("F,T,H,dh,gated", mk.ATTN_CASES)
def test_attention_kernel_against_float64_autograd(eng, F, T, H, dh, gated):
    d = mk.attn_case(F, T, H, dh, gated)
    s0 = stat(eng, COUNTER)
    out, probs, dqkv = run_attn(eng, d)
    assert stat(eng, COUNTER) - s0 == 3                                            # one launch forward, two backward
    want, want_p, want_g = mk.attn_reference(d)
    fp = FP32["attention"][mk.case_key(F, T, H, dh, gated)]
    e_f, e_p, e_b = _rel(out, want), _rel(probs, want_p), _rel(dqkv, want_g)
    print(f"attention F {F} T {T} H {H} dh {dh} gated {gated}: out {e_f:.3e} (fp32 CPU {fp['fwd']:.3e}) probs {e_p:.3e} ({fp['probs']:.3e}) "
          f"dqkv {e_b:.3e} ({fp['bwd']:.3e})")
    assert e_f < bound(fp["fwd"], FWD_FLOOR) and e_p < bound(fp["probs"], FWD_FLOOR) and e_b < bound(fp["bwd"], BWD_FLOOR)
    out2, probs2, dqkv2 = run_attn(eng, d)
    assert torch.equal(out, out2) and torch.equal(probs, probs2) and torch.equal(dqkv, dqkv2)      # reruns: the same bits
    if F > 1:                                                             # frame 0 of the F-frame call: the bits of a 1-frame call
        o1, p1, g1 = run_attn(eng, dict(d, qkv=d["qkv"][:1], dout=d["dout"][:1]))
        assert torch.equal(out[:1], o1) and torch.equal(probs[:1], p1) and torch.equal(dqkv[:1], g1)


def test_the_launch_refuses_what_it_cannot_run(eng):
    z = torch.zeros(8192, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())      # noqa: E731
    capi = eng.capi
    s0 = stat(eng, COUNTER)
    fwd = lambda *, q=p(z), frames=1, T=4, H=2, dh=8, c=p(z), tab=p(z): capi.i2v_convit_attention_f32(q, frames, T, H, dh, 0.5, c, tab, p(z), p(z), None)      # noqa: E731
    off = C.c_void_p(z.data_ptr() + 4)
    for kw, why in ((dict(q=None), b"null"), (dict(dh=6), b"multiple of 4"), (dict(c=None), b"go together"), (dict(tab=None), b"go together"),
                    (dict(T=4000, H=1, dh=4), b"LDS budget"), (dict(frames=70000), b"65535"),
                    (dict(frames=40000, T=196, H=8, dh=48), b"2^31"), (dict(q=off), b"alignment")):
        assert fwd(**kw) != 0
        err = capi.i2v_last_error()
        assert b"convit_attention" in err and b"hipErrorInvalidValue" in err and why in err, err
    assert capi.i2v_convit_attention_bwd_f32(p(z), p(z), p(z), 1, 4, 2, 6, 0.5, p(z), p(z), p(z), p(z), None) != 0
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
    spec = graphs.build_tiny(SMALL, (side, side))
    sd = weights.synthetic_state_dict(spec, 0)
    x = mk.twin_input(label)
    blocks = [spec.hook_for(d) for d in (1, 2, 3, 4)]
    assert blocks == mk.TWIN_HOOKS
    (feats, gx), hg = _hooks_and_grad(eng, spec, sd, blocks, x)
    _check(label, feats, gx, ConvitReference(spec, sd, blocks), x, hg)
    (feats2, gx2), _ = _hooks_and_grad(eng, spec, sd, blocks, x, max_frames=5)     # a second net, planned for more frames: the same bits
    assert all(torch.equal(a, b) for a, b in zip(feats, feats2)) and torch.equal(gx, gx2)
    net = eng.build_convit_net(spec, sd, blocks, 1)                                # frame 0 of the n-frame run against a 1-frame run
    f1, g1, _ = _run(net, spec, blocks, x[:1], [h[:1] for h in hg])
    net.close()
    assert all(torch.equal(a[:1], b) for a, b in zip(feats, f1)) and torch.equal(gx[:1], g1)
    (fa, _), _ = _hooks_and_grad(eng, spec, sd, [blocks[2]], x)                    # a single hook at the last GPSA block: no join is planned
    assert torch.equal(fa[0], feats[2])


@pytest.mark.parametrize("name", [TINY, SMALL])
def test_full_size_model_at_224_depths_1_to_4_against_float64(eng, name):
    spec = graphs.build(name)
    sd = weights.synthetic_state_dict(spec, 0)
    x = _rand(2, 3, 224, 224, seed=22)
    blocks = [spec.hook_for(d) for d in (1, 2, 3, 4)]
    assert blocks == mk.FULL[name]
    (feats, gx), hg = _hooks_and_grad(eng, spec, sd, blocks, x)
    assert feats[3].shape[1] == 197 * spec.dim
    _check(name, feats, gx, ConvitReference(spec, sd, blocks), x, hg)


def test_i2v_trajectory_on_the_twin_matches_the_float64_trajectory():
    vid = _video(2, 4, 64, 23)
    atk = attacks.ImageGuidedFMDirection_Adam([SMALL], depth=4, step_size=0.005, steps=10, graph_builder=graphs.build_tiny, weight_seed=0)
    adv = atk(vid, torch.zeros(2, dtype=torch.long), ["a", "b"]).cpu()
    spec = graphs.build_tiny(SMALL, (64, 64))
    check_trajectory(atk, adv, ConvitReference(spec, weights.synthetic_state_dict(spec, 0), [spec.hook_for(4)], dtype=torch.float64), vid, rtol=TRAJECTORY_RTOL)


def test_aens_of_the_twin_with_tiny_resnet_matches_the_oracle():
    vid = _video(1, 4, 64, 24)
    depths = {SMALL: [1, 4], "resnet": [2, 3]}
    atk = attacks.AENS_I2V_MF([SMALL, "resnet"], depths=depths, step_size=0.005, steps=4, momentum=0.5, graph_builder=graphs.build_tiny,
                              weight_seed=0)
    adv, _, costs = atk(vid, torch.zeros(1, dtype=torch.long), ["a"])
    cs, rs = (graphs.build_tiny(n, (64, 64)) for n in (SMALL, "resnet"))
    nets = [ConvitReference(cs, weights.synthetic_state_dict(cs, 0), [cs.hook_for(d) for d in depths[SMALL]], dtype=torch.float64),
            restate.OracleNet(rs, weights.synthetic_state_dict(rs, 0), [rs.hook_for(d, True) for d in depths["resnet"]], dtype=torch.float64)]
    ref = restate.run_attack(nets, vid, steps=4, step_size=0.005, mode="aens", coeffs=torch.ones(4, dtype=torch.float64), momentum=0.5)
    np.testing.assert_allclose(costs, ref["costs"], rtol=2e-4)


def test_workspace_of_convit_base_at_128_frames_depth_3(eng):
    """The plan the device holds equals the formula the host simulation's plan is checked against (tests/test_convit_cpu.py) and the
    figure of DESIGN.md section 22."""
    spec = graphs.build("convit_base")
    net = eng.build_convit_net(spec, weights.synthetic_state_dict(spec, 0), [spec.hook_for(3)], 128)
    got = net.workspace_bytes()
    net.close()
    assert got == spec.workspace_bytes([8], 128) == mk.WORKSPACE_BASE_D3
