"""GPU (-m gpu): timm's PiT on the MI355X (include/i2v_pit.h) -- the streaming attention kernel on its own, forward
and backward, against float64 autograd on the shapes of tests/make_pit_fixtures.ATTN_CASES (a single key; one tile and one token past it;
ragged across key tiles; PiT's head widths 48 and 64 at 730 and 963 tokens; T around the kernel's tile of 64; three cases that force the
online rescale), out, lse, dq, dk and dv each at its own bound; reruns and frame 0 of an n-frame call bit for bit; the device entries
against their scalar host twins; the pooling convolution and the overlapping patch pair against float64; the refusals, with the engine
going on afterwards; the three test-size twins and pit_s_224 against the float64 reference (tests/pit_reference.py); the shared-launch
route under I2V_PIT_ATTN=0; the launch counter; a 10-step I2V trajectory against `oracle.restate.run_attack`; the workspace figure on
both routes.

Bound: relative L2 against float64, at most the larger of the floor for that kind of case (entries 1e-6 forward, 1e-5 backward; nets
1e-5) and 4 x the error of the float32 CPU run of the same reference on the same inputs (tests/golden/pit_fp32_cpu_errors.json,
tests/make_pit_fixtures.py).  A case without a recorded error fails (KeyError)."""
import json
import os

import pytest
import torch

from i2v_amd import attacks, graphs, weights
from i2v_amd import lib as _lib
from tests import make_pit_fixtures as mk
from tests.family_harness import bound, check_net, check_trajectory, hooks_and_grad, rand as _rand, rel as _rel, run_net as _run, stat
from tests.pit_reference import PitReference
from tests.test_pit_cpu import attention_refusals, check_attn, check_patch, check_pool, run_attn, run_patch, run_pool

pytestmark = pytest.mark.gpu
FP32 = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pit_fp32_cpu_errors.json")))
NET_FLOOR, FWD_FLOOR, BWD_FLOOR = 1e-5, 1e-6, 1e-5
COUNTER = b"pit_attention_launches"
TRAJECTORY_RTOL = 2e-4      # of the trajectory's costs against the float64 run


@pytest.fixture(scope="module")
def eng():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return attacks.get_engine("cuda:0")


@pytest.fixture(scope="module")
def host():
    """The scalar host twins of the launches (csrc/i2v_pit_host.h), in the host simulation."""
    from tests.hostsim_util import hostsim_engine
    e = hostsim_engine()
    _lib.bind(e.capi, _lib._PIT_PROTOS)
    return e


def _cuda(t):
    return t.cuda()


def _sync(res):
    torch.cuda.synchronize()
    return res


@pytest.mark.parametrize("case", mk.ATTN_CASES, ids=lambda c: mk.case_key(*c))
def test_attention_kernel_against_float64_autograd(eng, host, case):
    d = mk.attn_case(*case)
    s0 = stat(eng, COUNTER)
    got = _sync(run_attn(eng, d, _cuda))
    assert stat(eng, COUNTER) - s0 == 4                                            # one launch forward; backward three: delta, dq, dk / dv
    check_attn(got, case)
    again = _sync(run_attn(eng, d, _cuda))
    assert all(torch.equal(a, b) for a, b in zip(got, again))             # reruns: the same bits
    if case[1] <= 200:                                                    # the device entries against their scalar host twins
        fp = FP32["attention"][mk.case_key(*case)]
        for k, a, b in zip(("fwd", "dq", "dk", "dv", "lse"), got, run_attn(host, d)):
            if case[1] == 1 and k in ("dq", "dk"):
                assert float((a - b).abs().max()) <= 1e-6
            else:
                assert _rel(a, b) < bound(fp[k], FWD_FLOOR if k in ("fwd", "lse") else BWD_FLOOR), k


def test_frame_0_of_a_3_frame_call_has_the_bits_of_a_1_frame_call(eng):
    d = mk.attn_case(3, 130, 3, 48)
    got = _sync(run_attn(eng, d, _cuda))
    one = _sync(run_attn(eng, dict(d, qkv=d["qkv"][:1], dout=d["dout"][:1]), _cuda))
    assert all(torch.equal(a[:1], b) for a, b in zip(got, one))


@pytest.mark.parametrize("case", mk.POOL_CASES, ids=lambda c: "x".join(map(str, c)))
def test_pool_kernels_against_float64(eng, case):
    check_pool(_sync(run_pool(eng, mk.pool_case(*case), _cuda)), case)


@pytest.mark.parametrize("case", mk.PATCH_CASES, ids=lambda c: "x".join(map(str, c)))
def test_patch_kernels_against_float64(eng, case):
    check_patch(_sync(run_patch(eng, mk.patch_case(*case), _cuda)), case)


def test_refusals_launch_nothing_and_the_engine_goes_on(eng):
    s0 = stat(eng, COUNTER)
    attention_refusals(eng, _cuda)
    assert stat(eng, COUNTER) - s0 == 1                                            # only the call that follows the refusals


def _hooks_and_grad(eng, spec, sd, hooks, x, max_frames=None, composed=False):
    launches = 0 if composed else 4 * (max(hooks) + 1)      # per block: one attention launch forward, three backward
    return hooks_and_grad(eng, spec, sd, hooks, x, max_frames, launches=(COUNTER, launches), composed=composed)


def _reference(spec, sd, hooks, x, hg):
    ref = PitReference(spec, sd, hooks)
    return ref.forward(x), ref.backward(hg)


@pytest.mark.parametrize("label", sorted(mk.TWINS))
def test_twin_hooks_at_depths_1_to_4_and_input_gradient(eng, label):
    name, side, _ = mk.TWINS[label]
    spec = graphs.build_tiny(name, (side, side))
    assert spec.arch == label
    sd = weights.synthetic_state_dict(spec, 0)
    x = mk.twin_input(label)
    hooks = [spec.hook_for(d) for d in (1, 2, 3, 4)]
    (feats, gx), hg = _hooks_and_grad(eng, spec, sd, hooks, x)
    check_net(label, feats, gx, *_reference(spec, sd, hooks, x, hg), FP32[label], NET_FLOOR)
    (feats2, gx2), _ = _hooks_and_grad(eng, spec, sd, hooks, x, max_frames=5)      # a second net, planned for more frames: the same bits
    assert all(torch.equal(a, b) for a, b in zip(feats, feats2)) and torch.equal(gx, gx2)
    net = eng.build_pit_net(spec, sd, hooks, 1)                                    # frame 0 of the n-frame run against a 1-frame run
    f1, g1, _ = _run(net, spec, hooks, x[:1], [h[:1] for h in hg])
    net.close()
    assert all(torch.equal(a[:1], b) for a, b in zip(feats, f1)) and torch.equal(gx[:1], g1)
    for i in range(4):                                                             # a single hook: the net is truncated there
        (fa, ga), _ = _hooks_and_grad(eng, spec, sd, [hooks[i]], x)
        assert torch.equal(fa[0], feats[i])
        ref1 = PitReference(spec, sd, [hooks[i]])
        ref1.forward(x)
        assert _rel(ga, ref1.backward([_rand(*fa[0].shape, seed=30)])) < bound(FP32[label]["grad"], NET_FLOOR)


@pytest.mark.parametrize("label", sorted(mk.TWINS))
def test_twin_on_the_shared_launch_route(eng, label, monkeypatch):
    """I2V_PIT_ATTN=0, read when the net is planned: the core on vit_gemm + vit_softmax + vit_gemm with P kept, backward the softmax
    backward and four products.  The same bound against float64; no attention launch is counted; the plan equals the formula under the
    switch."""
    name, side, _ = mk.TWINS[label]
    spec = graphs.build_tiny(name, (side, side))
    sd, x = weights.synthetic_state_dict(spec, 0), mk.twin_input(label)
    hooks = [spec.hook_for(d) for d in (1, 2, 3, 4)]
    monkeypatch.setenv("I2V_PIT_ATTN", "0")
    (feats, gx), hg = _hooks_and_grad(eng, spec, sd, hooks, x, composed=True)
    check_net(label, feats, gx, *_reference(spec, sd, hooks, x, hg), FP32[label], NET_FLOOR)


@pytest.mark.parametrize("name", mk.FULL)
def test_full_size_model_at_224_depths_1_to_4_against_float64(eng, name):
    spec = graphs.build_surrogate(name)
    sd = weights.synthetic_state_dict(spec, 0)
    x = mk.full_input()
    hooks = [spec.hook_for(d) for d in (1, 2, 3, 4)]
    (feats, gx), hg = _hooks_and_grad(eng, spec, sd, hooks, x)
    assert [f.shape[1] for f in feats] == [730 * 144, 197 * 288, 197 * 288, 50 * 576]
    check_net(name, feats, gx, *_reference(spec, sd, hooks, x, hg), FP32[name], NET_FLOOR)


def test_i2v_trajectory_on_the_twin_matches_the_float64_trajectory():
    """10 steps at the depth and on the twin of `make_pit_fixtures.TRAJECTORY`, costs within the 2e-4 the XCiT, Twins and BEiT trajectory
    tests hold.  The float32 reference itself stays under that bound there, measured on the CPU with `restate.run_attack` in float32
    against float64 (tests/golden/pit_fp32_cpu_errors.json, "trajectory")."""
    label, depth = mk.TRAJECTORY
    name, side, _ = mk.TWINS[label]
    clip = mk.TRAJECTORY_CLIPS[label]
    assert FP32["trajectory"][label][str(depth)] < 2e-4 / 4               # the float32 reference itself is comfortably inside there
    vid = mk.video(*clip)
    atk = attacks.ImageGuidedFMDirection_Adam([name], depth=depth, step_size=0.005, steps=10, graph_builder=graphs.build_tiny, weight_seed=0)
    adv = atk(vid, torch.zeros(clip[0], dtype=torch.long), ["a", "b"]).cpu()
    spec = graphs.build_tiny(name, (side, side))
    assert spec.arch == label
    check_trajectory(atk, adv, PitReference(spec, weights.synthetic_state_dict(spec, 0), [spec.hook_for(depth)], dtype=torch.float64), vid, rtol=TRAJECTORY_RTOL)


@pytest.mark.parametrize("composed", [False, True])
def test_workspace_of_pit_s_at_128_frames_depth_3(eng, composed, monkeypatch):
    """The plan the device holds equals the formula the host simulation's plan is checked against (tests/test_pit_cpu.py), on both
    routes."""
    if composed:
        monkeypatch.setenv("I2V_PIT_ATTN", "0")
    else:
        monkeypatch.delenv("I2V_PIT_ATTN", raising=False)
    spec = graphs.build_surrogate("pit_s_224")
    net = eng.build_pit_net(spec, weights.synthetic_state_dict(spec, 0), [spec.hook_for(3)], 128)
    got = net.workspace_bytes()
    net.close()
    assert got == spec.workspace_bytes([7], 128, composed=composed)
