"""GPU (-m gpu): timm's Twins on the MI355X (include/i2v_twins.h) -- the sub-sampled attention kernel on its own,
forward and backward, against float64 autograd of timm's literal arithmetic on the shapes of tests/make_twins_fixtures.ATTN_CASES (a hot
case with scores of magnitude ~30; a single key; Tk at the limit of 64); the device entries against their scalar host twins; the window
host twin against the Swin window kernel; the block gather and scatter, exact; the refusals, with the engine going on afterwards; the
three test-size twins, twins_pcpvt_small and twins_svt_small against the float64 reference (tests/twins_reference.py); repeatability;
frame 0 of a 3-frame call against a 1-frame call; the launch counter; a 10-step I2V trajectory (depth 3, on the SVT twin) and an AENS
ensemble against `oracle.restate.run_attack`; the workspace figure.

Bound: relative L2 against float64, at most the larger of the floor for that kind of case (entries 1e-6 forward, 1e-5 backward; nets
1e-5) and 4 x the error of the float32 CPU run of the same reference on the same inputs (tests/golden/twins_fp32_cpu_errors.json,
tests/make_twins_fixtures.py).  A case without a recorded error fails (KeyError)."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from i2v_amd import attacks, graphs, weights
from i2v_amd import lib as _lib
from oracle import restate
from tests import make_twins_fixtures as mk
from tests.family_harness import bound, check_net, check_trajectory, hooks_and_grad, rand as _rand, rel as _rel, run_net as _run, stat
from tests.twins_reference import TwinsReference

pytestmark = pytest.mark.gpu
PCPVT, SVT = "twins_pcpvt_small", "twins_svt_small"
FP32 = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "twins_fp32_cpu_errors.json")))
NET_FLOOR, FWD_FLOOR, BWD_FLOOR = 1e-5, 1e-6, 1e-5
COUNTER = b"twins_attention_launches"
TRAJECTORY_RTOL = 2e-4      # of the trajectory's costs against the float64 run


@pytest.fixture(scope="module")
def eng():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return attacks.get_engine("cuda:0")


@pytest.fixture(scope="module")
def host():
    """The scalar host twins of the launches (csrc/i2v_twins_host.h), in the host simulation."""
    from tests.hostsim_util import hostsim_engine
    e = hostsim_engine()
    _lib.bind(e.capi, _lib._TWINS_PROTOS)
    return e


def _dev(v):
    return v.float().cuda().contiguous()


def run_attn(eng, d):
    """(out, dq, dkv) of an attention case through the two C entries, back on the host."""
    q, kv = _dev(d["q"]), _dev(d["kv"])
    out = eng.twins_attention(q, kv, d["heads"])
    dq, dkv = eng.twins_attention_bwd(q, kv, _dev(d["dout"]), d["heads"])
    torch.cuda.synchronize()
    return out.cpu(), dq.cpu(), dkv.cpu()


@pytest.mark.parametrize("F,Tq,Tk,H,dh,kind", mk.ATTN_CASES)
def test_attention_kernel_against_float64_autograd(eng, host, F, Tq, Tk, H, dh, kind):
    d = mk.attn_case(F, Tq, Tk, H, dh, kind)
    s0 = stat(eng, COUNTER)
    out, dq, dkv = run_attn(eng, d)
    assert stat(eng, COUNTER) - s0 == 3                                            # one launch forward; backward two: dq, then dk / dv
    want, want_q, want_kv = mk.attn_reference(d)
    fp = FP32["attention"][mk.case_key(F, Tq, Tk, H, dh, kind)]
    e_f, e_kv = _rel(out, want), _rel(dkv, want_kv)
    print(f"gsa F {F} Tq {Tq} Tk {Tk} H {H} dh {dh} {kind}: out {e_f:.3e} (fp32 CPU {fp['fwd']:.3e}) dkv {e_kv:.3e} ({fp['dkv']:.3e})")
    assert e_f < bound(fp["fwd"], FWD_FLOOR) and e_kv < bound(fp["dkv"], BWD_FLOOR)
    if Tk == 1:                                                           # a single key: P = 1 exactly, so dS = 0 and dq = 0
        assert float(dq.abs().max()) == 0.0
    else:
        e_q = _rel(dq, want_q)
        print(f"    dq {e_q:.3e} ({fp['dq']:.3e})")
        assert e_q < bound(fp["dq"], BWD_FLOOR)
    out2, dq2, dkv2 = run_attn(eng, d)
    assert torch.equal(out, out2) and torch.equal(dq, dq2) and torch.equal(dkv, dkv2)       # reruns: the same bits
    if F > 1:                                                             # frame 0 of the F-frame call: the bits of a 1-frame call
        o1, q1, k1 = run_attn(eng, dict(d, q=d["q"][:1], kv=d["kv"][:1], dout=d["dout"][:1]))
        assert torch.equal(out[:1], o1) and torch.equal(dq[:1], q1) and torch.equal(dkv[:1], k1)
    f = lambda v: v.float().contiguous()      # noqa: E731
    ho = host.twins_attention(f(d["q"]), f(d["kv"]), H)                   # the device entries against their scalar host twins
    hq, hkv = host.twins_attention_bwd(f(d["q"]), f(d["kv"]), f(d["dout"]), H)
    assert _rel(out, ho) < bound(fp["fwd"], FWD_FLOOR) and _rel(dkv, hkv) < bound(fp["dkv"], BWD_FLOOR)
    assert torch.equal(dq, hq) if Tk == 1 else _rel(dq, hq) < bound(fp["dq"], BWD_FLOOR)


def test_window_host_twin_agrees_with_the_device_window_kernel(eng, host):
    d = mk.window_case()
    g, ws, H = d["grid"], d["window"], d["heads"]
    out = eng.twins_window_attention(_dev(d["qkv"]), g, ws, H).cpu()
    dqkv = eng.twins_window_attention(_dev(d["qkv"]), g, ws, H, dout=_dev(d["dout"])).cpu()
    want, want_g = mk.window_reference(d)
    fp = FP32["window"]
    assert _rel(out, want) < bound(fp["fwd"], FWD_FLOOR) and _rel(dqkv, want_g) < bound(fp["bwd"], BWD_FLOOR)
    ho = host.twins_window_attention(d["qkv"].float().contiguous(), g, ws, H)
    hg = host.twins_window_attention(d["qkv"].float().contiguous(), g, ws, H, dout=d["dout"].float().contiguous())
    assert _rel(ho, out) < bound(fp["fwd"], FWD_FLOOR) and _rel(hg, dqkv) < bound(fp["bwd"], BWD_FLOOR)


@pytest.mark.parametrize("s,H,W", mk.BLOCK_CASES)
def test_block_gather_and_scatter_are_exact(eng, s, H, W):
    d = mk.block_case(s, H, W)
    shape = tuple(d["x"].shape)
    assert torch.equal(eng.twins_block_gather(d["x"].cuda(), s).cpu(), mk.gather_reference(d["x"], s))
    want = mk.scatter_reference(d["drows"], shape, s)
    assert torch.equal(eng.twins_block_scatter(d["drows"].cuda(), shape, s).cpu(), want)
    assert torch.equal(eng.twins_block_scatter(d["drows"].cuda(), shape, s, into=d["base"].cuda()).cpu(), d["base"] + want)


def test_the_launches_refuse_what_they_cannot_run(eng):
    z = torch.zeros(16384, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())      # noqa: E731
    capi = eng.capi
    s0 = stat(eng, COUNTER)
    fwd = lambda *, q=p(z), kv=p(z), frames=1, Tq=4, Tk=4, H=2, dh=8: capi.i2v_twins_attention_f32(q, kv, frames, Tq, Tk, H, dh, 0.5, p(z), None)      # noqa: E731
    off = C.c_void_p(z.data_ptr() + 4)
    for kw, why in ((dict(Tk=65), b"more than 64 keys"), (dict(H=1, dh=68), b"wider than 64"), (dict(dh=6), b"multiple of 4"), (dict(q=None), b"null"),
                    (dict(kv=None), b"null"), (dict(q=off), b"alignment"), (dict(kv=off), b"alignment")):
        assert fwd(**kw) != 0
        err = capi.i2v_last_error()
        assert b"twins_attention" in err and b"hipErrorInvalidValue" in err and why in err, err
    for kw, why in ((dict(Tk=65), b"more than 64 keys"), (dict(dh=68, H=1), b"wider than 64"), (dict(dh=6), b"multiple of 4")):
        a = dict(dict(Tk=4, H=2, dh=8), **kw)
        assert capi.i2v_twins_attention_bwd_f32(p(z), p(z), p(z), 1, 4, a["Tk"], a["H"], a["dh"], 0.5, p(z), p(z), None) != 0
        assert b"twins_attention_bwd" in capi.i2v_last_error() and why in capi.i2v_last_error()
    assert capi.i2v_twins_attention_bwd_f32(p(z), p(z), p(z), 1, 4, 4, 2, 8, 0.5, None, p(z), None) != 0 and b"null" in capi.i2v_last_error()
    y = C.c_void_p(z.data_ptr() + 32768)
    assert capi.i2v_twins_block_gather_f32(p(z), y, 1, 4, 4, 8, 3, None) != 0 and b"2, 4 or 8" in capi.i2v_last_error()
    assert capi.i2v_twins_block_scatter_f32(p(z), y, 1, 6, 4, 8, 4, 0, None) != 0 and b"whole number of blocks" in capi.i2v_last_error()
    assert capi.i2v_twins_block_gather_f32(p(z), None, 1, 4, 4, 8, 2, None) != 0 and b"null" in capi.i2v_last_error()
    assert stat(eng, COUNTER) == s0                                                # nothing was launched
    spec = graphs.build_tiny(PCPVT, (64, 64))
    sd = weights.synthetic_state_dict(spec, 0)
    with pytest.raises(_lib.I2VError, match="hooked twice"):
        eng.build_twins_net(spec, sd, [1, 1], 2)
    with pytest.raises(_lib.I2VError, match="outside"):
        eng.build_twins_net(spec, sd, [4], 2)
    net = eng.build_twins_net(spec, sd, [0], 2)
    with pytest.raises(_lib.I2VError, match="planned for"):
        net.forward(torch.zeros(3, 3, 64, 64, device="cuda"))
    net.forward(torch.zeros(2, 3, 64, 64, device="cuda"))                 # the engine goes on
    torch.cuda.synchronize()
    net.close()
    d = mk.attn_case(2, 4, 4, 2, 8)
    assert _rel(run_attn(eng, d)[0], mk.attn_reference(d)[0]) < 1e-6


def _gsa_blocks(spec, stages):
    return sum(not spec.is_lsa(k, j) for k in range(max(stages) + 1) for j in range(spec.depths[k]))


def _hooks_and_grad(eng, spec, sd, stages, x, max_frames=None):
    launches = 3 * _gsa_blocks(spec, stages)      # per GSA block: one attention launch forward, two backward
    return hooks_and_grad(eng, spec, sd, stages, x, max_frames, launches=(COUNTER, launches))


def _check(label, feats, gx, ref, x, hg):
    check_net(label, feats, gx, ref.forward(x), ref.backward(hg), FP32[label], NET_FLOOR)


@pytest.mark.parametrize("label", sorted(mk.TWINS))
def test_twin_hooks_at_depths_1_to_4_and_input_gradient(eng, label):
    name, side, _ = mk.TWINS[label]
    spec = graphs.build_tiny(name, (side, side))
    assert spec.arch == label
    sd = weights.synthetic_state_dict(spec, 0)
    x = mk.twin_input(label)
    stages = [spec.hook_for(d) for d in (1, 2, 3, 4)]
    assert stages == mk.HOOKS
    (feats, gx), hg = _hooks_and_grad(eng, spec, sd, stages, x)
    _check(label, feats, gx, TwinsReference(spec, sd, stages), x, hg)
    (feats2, gx2), _ = _hooks_and_grad(eng, spec, sd, stages, x, max_frames=5)     # a second net, planned for more frames: the same bits
    assert all(torch.equal(a, b) for a, b in zip(feats, feats2)) and torch.equal(gx, gx2)
    net = eng.build_twins_net(spec, sd, stages, 1)                                 # frame 0 of the n-frame run against a 1-frame run
    f1, g1, _ = _run(net, spec, stages, x[:1], [h[:1] for h in hg])
    net.close()
    assert all(torch.equal(a[:1], b) for a, b in zip(feats, f1)) and torch.equal(gx[:1], g1)
    (fa, _), _ = _hooks_and_grad(eng, spec, sd, [stages[2]], x)                    # a single hook: the net is truncated there
    assert torch.equal(fa[0], feats[2])


@pytest.mark.parametrize("label", ["twins_pcpvt_test_96", "twins_svt_test"])
def test_twin_on_the_shared_launch_route(eng, label, monkeypatch):
    """I2V_TWINS_ATTN=0, read when the net is planned: the GSA core on vit_gemm + vit_softmax + vit_gemm with P kept, backward the
    softmax backward and four products.  The same bound against float64; no attention launch is counted; the plan equals the formula
    under the switch; frame 0 has the bits of a 1-frame run."""
    name, side, _ = mk.TWINS[label]
    spec = graphs.build_tiny(name, (side, side))
    sd, x = weights.synthetic_state_dict(spec, 0), mk.twin_input(label)
    monkeypatch.setenv("I2V_TWINS_ATTN", "0")
    net = eng.build_twins_net(spec, sd, mk.HOOKS, x.shape[0])
    assert net.workspace_bytes() == spec.workspace_bytes(mk.HOOKS, x.shape[0]) > spec.workspace_bytes(mk.HOOKS, x.shape[0], composed=False)
    s0 = stat(eng, COUNTER)
    feats, gx, hg = _run(net, spec, mk.HOOKS, x)
    assert stat(eng, COUNTER) == s0
    net.close()
    _check(label, feats, gx, TwinsReference(spec, sd, mk.HOOKS), x, hg)
    net = eng.build_twins_net(spec, sd, mk.HOOKS, 1)
    f1, g1, _ = _run(net, spec, mk.HOOKS, x[:1], [h[:1] for h in hg])
    net.close()
    assert all(torch.equal(a[:1], b) for a, b in zip(feats, f1)) and torch.equal(gx[:1], g1)


@pytest.mark.parametrize("name", mk.FULL)
def test_full_size_model_at_224_depths_1_to_4_against_float64(eng, name):
    spec = graphs.build(name)
    sd = weights.synthetic_state_dict(spec, 0)
    x = _rand(2, 3, 224, 224, seed=22)
    stages = [spec.hook_for(d) for d in (1, 2, 3, 4)]
    (feats, gx), hg = _hooks_and_grad(eng, spec, sd, stages, x)
    assert feats[0].shape[1] == 3136 * spec.dims[0] and feats[3].shape[1] == 49 * spec.dims[3]
    _check(name, feats, gx, TwinsReference(spec, sd, stages), x, hg)


def test_i2v_trajectory_on_the_twin_matches_the_float64_trajectory():
    """10 steps at depth 3 on the SVT twin, costs within the 2e-4 the XCiT trajectory test holds.  The twin is chosen by the reference's
    own float32 error on this clip, measured on the CPU with `restate.run_attack` in float32 against float64
    (tests/golden/twins_fp32_cpu_errors.json, "trajectory"): on the SVT twin it stays under the bound at every depth, at depth 3
    included; on the two PCPVT twins it is 1.1e-3 and 2.2e-3 at depth 3 -- there the ten Adam steps amplify float32 rounding past 2e-4,
    whatever computes the costs, and could not tell a right kernel from a wrong one.  (Their single passes are held to float64 in the
    twin tests above.)"""
    name, clip = mk.TRAJECTORY
    assert FP32["trajectory"]["3"] < 2e-4                                 # the float32 reference itself holds the bound there
    vid = mk.video(*clip)
    atk = attacks.ImageGuidedFMDirection_Adam([name], depth=3, step_size=0.005, steps=10, graph_builder=graphs.build_tiny, weight_seed=0)
    adv = atk(vid, torch.zeros(clip[0], dtype=torch.long), ["a", "b"]).cpu()
    spec = graphs.build_tiny(name, (clip[2], clip[2]))
    check_trajectory(atk, adv, TwinsReference(spec, weights.synthetic_state_dict(spec, 0), [spec.hook_for(3)], dtype=torch.float64), vid, rtol=TRAJECTORY_RTOL)


def test_aens_of_the_twin_with_tiny_resnet_matches_the_oracle():
    vid = mk.video(1, 4, 64, 24)
    depths = {PCPVT: [1, 4], "resnet": [2, 3]}
    atk = attacks.AENS_I2V_MF([PCPVT, "resnet"], depths=depths, step_size=0.005, steps=4, momentum=0.5, graph_builder=graphs.build_tiny,
                              weight_seed=0)
    adv, _, costs = atk(vid, torch.zeros(1, dtype=torch.long), ["a"])
    cs, rs = (graphs.build_tiny(n, (64, 64)) for n in (PCPVT, "resnet"))
    nets = [TwinsReference(cs, weights.synthetic_state_dict(cs, 0), [cs.hook_for(d) for d in depths[PCPVT]], dtype=torch.float64),
            restate.OracleNet(rs, weights.synthetic_state_dict(rs, 0), [rs.hook_for(d, True) for d in depths["resnet"]], dtype=torch.float64)]
    ref = restate.run_attack(nets, vid, steps=4, step_size=0.005, mode="aens", coeffs=torch.ones(4, dtype=torch.float64), momentum=0.5)
    np.testing.assert_allclose(costs, ref["costs"], rtol=2e-4)


def test_workspace_of_twins_pcpvt_small_at_128_frames_depth_3(eng):
    """The plan the device holds equals the formula the host simulation's plan is checked against (tests/test_twins_cpu.py)."""
    spec = graphs.build(PCPVT)
    net = eng.build_twins_net(spec, weights.synthetic_state_dict(spec, 0), [spec.hook_for(3)], 128)
    got = net.workspace_bytes()
    net.close()
    assert got == spec.workspace_bytes([2], 128)
