"""GPU (-m gpu): timm's TNT on the MI355X (include/i2v_tnt.h) -- the batched short-sequence attention launches on
their own, forward and backward, against float64 autograd on the shapes of tests/make_tnt_fixtures.ATTN_CASES (one sequence; one fewer
and one more than a workgroup's worth; a single token; T 9; head widths 1, 3, 6, 10 and 16; 1 and 8 heads; one full frame of tnt_s; two
cases that stress the softmax), out, dq, dk and dv each at its own bound; reruns and sequence 0 of a 3-sequence call bit for bit; the
device entries against their scalar host twins; the launch counter; the pixel pair against float64, as an exact transpose and
accumulating; the refusals, with the engine going on afterwards; both test-size twins and tnt_s_patch16_224 against the float64 reference
(tests/tnt_reference.py); a 10-step I2V trajectory against `oracle.restate.run_attack`; the workspace figure.

Bound: relative L2 against float64, at most the larger of the floor for that kind of case (entries 1e-6 forward, 1e-5 backward; nets
1e-5) and 4 x the error of the float32 CPU run of the same reference on the same inputs (tests/golden/tnt_fp32_cpu_errors.json,
tests/make_tnt_fixtures.py).  A case without a recorded error fails (KeyError)."""
import json
import os

import pytest
import torch

from i2v_amd import attacks, graphs, weights
from i2v_amd import lib as _lib
from tests import make_tnt_fixtures as mk
from tests.family_harness import bound, check_net, check_trajectory, hooks_and_grad, rand as _rand, rel as _rel, run_net as _run, stat
from tests.test_tnt_cpu import FWD_PARTS, check_attn, check_pixels, entry_refusals, run_attn, run_pixels
from tests.tnt_reference import TntReference

pytestmark = pytest.mark.gpu
FP32 = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tnt_fp32_cpu_errors.json")))
FWD_FLOOR, BWD_FLOOR, NET_FLOOR = 1e-6, 1e-5, 1e-5
COUNTER = b"tnt_attention_launches"


@pytest.fixture(scope="module")
def eng():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return attacks.get_engine("cuda:0")


@pytest.fixture(scope="module")
def host():
    """The scalar host twins of the launches (csrc/i2v_tnt_host.h), in the host simulation."""
    from tests.hostsim_util import hostsim_engine
    e = hostsim_engine()
    _lib.bind(e.capi, _lib._TNT_PROTOS)
    return e


def _cuda(t):
    return t.cuda()


def _sync(res):
    torch.cuda.synchronize()
    return res


def test_the_fixture_brackets_a_workgroups_worth_of_sequences(eng):
    assert eng.tnt_attention_group(16, 4, 6) == mk.GROUP


@pytest.mark.parametrize("case", mk.ATTN_CASES, ids=lambda c: mk.case_key(*c))
def test_attention_kernels_against_float64_autograd(eng, host, case):
    d = mk.attn_case(*case)
    s0 = stat(eng, COUNTER)
    got = _sync(run_attn(eng, d, _cuda))
    assert stat(eng, COUNTER) - s0 == 2                                            # one launch forward, one backward
    check_attn(got, case)
    again = _sync(run_attn(eng, d, _cuda))
    assert all(torch.equal(a, b) for a, b in zip(got, again))             # reruns: the same bits
    fp = FP32["attention"][mk.case_key(*case)]                            # the device entries against their scalar host twins, which add
    for k, a, b in zip(mk.ATTN_PARTS, got, run_attn(host, d)):            # in the device's order but call the host's expf: the bound
        if case[1] == 1 and k in ("dq", "dk"):
            assert float((a - b).abs().max()) <= 1e-6
        else:
            assert _rel(a, b) < bound(fp[k], FWD_FLOOR if k in FWD_PARTS else BWD_FLOOR), k


def test_sequence_0_of_a_3_sequence_call_has_the_bits_of_a_1_sequence_call(eng):
    d = mk.attn_case(3, 16, 4, 6)
    got = _sync(run_attn(eng, d, _cuda))
    one = _sync(run_attn(eng, dict(d, qkv=d["qkv"][:1], dout=d["dout"][:1]), _cuda))
    assert all(torch.equal(a[:1], b) for a, b in zip(got, one))
    many = mk.attn_case(4 * mk.GROUP + 1, 16, 4, 6)                       # ... and whichever sequences share its workgroup
    g2 = _sync(run_attn(eng, dict(many, qkv=torch.cat((d["qkv"][:1], many["qkv"][1:])), dout=torch.cat((d["dout"][:1], many["dout"][1:]))), _cuda))
    assert all(torch.equal(a[:1], b) for a, b in zip(g2, one))


@pytest.mark.parametrize("case", mk.PIXEL_CASES, ids=lambda c: mk.case_key(*c))
def test_pixel_kernels_against_float64(eng, host, case):
    d = mk.pixel_case(*case)
    got = _sync(run_pixels(eng, d, _cuda))
    check_pixels(got, case)
    assert all(torch.equal(a, b) for a, b in zip(got, run_pixels(host, d)))      # the host twin adds in the device's order: the same bits


def test_refusals_launch_nothing_and_the_engine_goes_on(eng):
    s0 = stat(eng, COUNTER)
    entry_refusals(eng, _cuda)
    assert stat(eng, COUNTER) - s0 == 1                                            # only the forward that follows the refusals


def _hooks_and_grad(eng, spec, sd, hooks, x, max_frames=None):
    launches = 2 * (max(hooks) + 1)      # per block: one inner attention launch forward, one backward
    return hooks_and_grad(eng, spec, sd, hooks, x, max_frames, launches=(COUNTER, launches))


def _reference(spec, sd, hooks, x, hg):
    ref = TntReference(spec, sd, hooks)
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
    net = eng.build_tnt_net(spec, sd, hooks, 1)                                    # frame 0 of the n-frame run against a 1-frame run
    f1, g1, _ = _run(net, spec, hooks, x[:1], [h[:1] for h in hg])
    net.close()
    assert all(torch.equal(a[:1], b) for a, b in zip(feats, f1)) and torch.equal(gx[:1], g1)
    for i in (0, 2):                                                               # a single hook: the net is truncated there
        (fa, ga), _ = _hooks_and_grad(eng, spec, sd, [hooks[i]], x)
        assert torch.equal(fa[0], feats[i])
        ref1 = TntReference(spec, sd, [hooks[i]])
        ref1.forward(x)
        assert _rel(ga, ref1.backward([_rand(*fa[0].shape, seed=30)])) < bound(FP32[label]["grad"], NET_FLOOR)


@pytest.mark.parametrize("name", mk.FULL)
def test_full_size_model_at_224_depths_1_to_4_against_float64(eng, name):
    spec = graphs.build_surrogate(name)
    sd = weights.synthetic_state_dict(spec, 0)
    x = mk.full_input()
    hooks = [spec.hook_for(d) for d in (1, 2, 3, 4)]
    (feats, gx), hg = _hooks_and_grad(eng, spec, sd, hooks, x)
    assert [f.shape[1] for f in feats] == [197 * 384] * 4
    check_net(name, feats, gx, *_reference(spec, sd, hooks, x, hg), FP32[name], NET_FLOOR)
    net = eng.build_tnt_net(spec, sd, hooks, 2)                                    # one frame of the two: the same bits
    f1, g1, _ = _run(net, spec, hooks, x[:1], [h[:1] for h in hg])
    net.close()
    assert all(torch.equal(a[:1], b) for a, b in zip(feats, f1)) and torch.equal(gx[:1], g1)


def test_i2v_trajectory_on_the_twin_matches_the_float64_trajectory():
    """10 steps on tnt_test at depth 3, the costs against the float64 trajectory of `restate.run_attack` within max(1e-5, 4 x the
    float32 reference's own relative cost error on the same clip) (tests/golden/tnt_fp32_cpu_errors.json, "trajectory")."""
    label, depth = "tnt_test", mk.TRAJECTORY_DEPTH
    name, side, _ = mk.TWINS[label]
    clip = mk.TRAJECTORY_CLIP
    rtol = bound(FP32["trajectory"][label][str(depth)], NET_FLOOR)
    vid = mk.video(*clip)
    atk = attacks.ImageGuidedFMDirection_Adam([name], depth=depth, step_size=0.005, steps=10, graph_builder=graphs.build_tiny, weight_seed=0)
    adv = atk(vid, torch.zeros(clip[0], dtype=torch.long), ["a", "b"]).cpu()
    spec = graphs.build_tiny(name, (side, side))
    assert spec.arch == label
    check_trajectory(atk, adv, TntReference(spec, weights.synthetic_state_dict(spec, 0), [spec.hook_for(depth)], dtype=torch.float64), vid, rtol=rtol)


def test_workspace_of_tnt_s_at_128_frames_depth_3(eng):
    """The plan the device holds equals the formula the host simulation's plan is checked against (tests/test_tnt_cpu.py)."""
    spec = graphs.build_surrogate("tnt_s_patch16_224")
    net = eng.build_tnt_net(spec, weights.synthetic_state_dict(spec, 0), [spec.hook_for(3)], 128)
    got = net.workspace_bytes()
    net.close()
    assert got == spec.workspace_bytes([8], 128)
