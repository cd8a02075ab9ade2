"""GPU (-m gpu): timm's XCiT on the MI355X (include/i2v_xcit.h) -- the cross-covariance attention kernel on its own,
forward, probs and backward, against float64 autograd of timm's literal arithmetic on the shapes of tests/make_xcit_fixtures.ATTN_CASES
(a temperature of 30; an all-zero q column and k column); the depthwise 3 x 3 launch with and without its transform, residual and output
multiply; the stem's gather and scatter on odd and even planes; both test-size twins, xcit_nano_12_p16_224 and xcit_tiny_12_p16_224
against the float64 reference (tests/xcit_reference.py); repeatability; frame 0 of a 3-frame call against a 1-frame call; the launch
counter; the refusals, with the engine going on afterwards; a 10-step I2V trajectory (depth 3) and an AENS ensemble against
`oracle.restate.run_attack`; the workspace figure.

Bound: relative L2 against float64, at most the larger of the floor for that kind of case (entries 1e-6 forward and on probs, 1e-5
backward; nets 1e-5) and 4 x the error of the float32 CPU run of the same reference on the same inputs
(tests/golden/xcit_fp32_cpu_errors.json, tests/make_xcit_fixtures.py).  A case without a recorded error fails (KeyError)."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from i2v_amd import attacks, graphs, weights
from i2v_amd import lib as _lib
from oracle import restate
from tests import make_xcit_fixtures as mk
from tests.family_harness import bound, check_net, check_trajectory, hooks_and_grad, rand as _rand, rel as _rel, run_net as _run, stat, video as _video
from tests.xcit_reference import XcitReference

pytestmark = pytest.mark.gpu
NANO, TINY = "xcit_nano_12_p16_224", "xcit_tiny_12_p16_224"
FP32 = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "xcit_fp32_cpu_errors.json")))
NET_FLOOR, FWD_FLOOR, BWD_FLOOR = 1e-5, 1e-6, 1e-5
COUNTER = b"xcit_attention_launches"
TRAJECTORY_RTOL = 2e-4      # of the trajectory's costs against the float64 run


@pytest.fixture(scope="module")
def eng():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return attacks.get_engine("cuda:0")


def _dev(v):
    return None if v is None else v.float().cuda().contiguous()


def run_attn(eng, d):
    """(out, probs, dqkv) of an attention case through the two C entries, back on the host."""
    qkv, temp = _dev(d["qkv"]), _dev(d["temperature"])
    out, probs, gram = eng.xcit_attention(qkv, d["heads"], temp)
    dqkv = eng.xcit_attention_bwd(qkv, gram, probs, _dev(d["dout"]), d["heads"], temp)
    torch.cuda.synchronize()
    return out.cpu(), probs.cpu(), dqkv.cpu()


@pytest.mark.parametrize("F,T,H,dh,kind", mk.ATTN_CASES)
def test_attention_kernel_against_float64_autograd(eng, F, T, H, dh, kind):
    d = mk.attn_case(F, T, H, dh, kind)
    s0 = stat(eng, COUNTER)
    out, probs, dqkv = run_attn(eng, d)
    assert stat(eng, COUNTER) - s0 == 2                                            # one launch forward, one backward
    want, want_p, want_g = mk.attn_reference(d)
    fp = FP32["attention"][mk.case_key(F, T, H, dh, kind)]
    e_f, e_p = _rel(out, want), _rel(probs, want_p)
    print(f"xca F {F} T {T} H {H} dh {dh} {kind}: out {e_f:.3e} (fp32 CPU {fp['fwd']:.3e}) probs {e_p:.3e} ({fp['probs']:.3e})")
    assert e_f < bound(fp["fwd"], FWD_FLOOR) and e_p < bound(fp["probs"], FWD_FLOOR)
    if kind == "zero":                                                    # the reference's own gradient is of order 1 / eps there
        assert float((probs[:, 0, 3] - 1.0 / dh).abs().max()) < 1e-7 and bool(torch.isfinite(dqkv).all())
    else:
        e_b = _rel(dqkv, want_g)
        print(f"    dqkv {e_b:.3e} ({fp['bwd']:.3e})")
        assert e_b < bound(fp["bwd"], BWD_FLOOR)
    out2, probs2, dqkv2 = run_attn(eng, d)
    assert torch.equal(out, out2) and torch.equal(probs, probs2) and torch.equal(dqkv, dqkv2)      # reruns: the same bits
    if F > 1:                                                             # frame 0 of the F-frame call: the bits of a 1-frame call
        o1, p1, g1 = run_attn(eng, dict(d, qkv=d["qkv"][:1], dout=d["dout"][:1]))
        assert torch.equal(out[:1], o1) and torch.equal(probs[:1], p1) and torch.equal(dqkv[:1], g1)


@pytest.mark.parametrize("P,Cn,variant", mk.DW3_CASES)
def test_depthwise_launch_against_float64(eng, P, Cn, variant):
    d = mk.dw3_case(P, Cn, variant)
    run = lambda c: eng.xcit_dw3(*[_dev(c[k]) for k in ("x", "w", "b", "ta", "ts", "add", "ma", "mu")]).cpu()      # noqa: E731
    y = run(d)
    e = _rel(y, mk.dw3_reference(d))
    cpu = FP32["dw3"][mk.dw3_key(P, Cn, variant)]
    print(f"dw3 {P} x {P} x {Cn} {variant}: {e:.3e} (fp32 CPU {cpu:.3e})")
    assert e < bound(cpu, FWD_FLOOR)
    assert torch.equal(y, run(d)) and torch.equal(y[:1], run({k: (v[:1] if k in ("x", "add", "mu") and v is not None else v) for k, v in d.items()}))


@pytest.mark.parametrize("P,Cn,nchw", mk.STEM_CASES)
def test_stem_gather_and_scatter(eng, P, Cn, nchw):
    d = mk.stem_case(P, Cn, nchw)
    rows = eng.xcit_stem_gather(_dev(d["src"]), nchw).cpu()
    assert torch.equal(rows, mk.gather_reference(d["src"].float(), nchw))                    # a copy: exact
    got = eng.xcit_stem_scatter(_dev(d["drows"]), tuple(d["src"].shape), _dev(d["pre"]), nchw).cpu()
    e = _rel(got, mk.scatter_reference(d))
    cpu = FP32["scatter"][mk.stem_key(P, Cn, nchw)]
    print(f"scatter {P} x {P} x {Cn} image {nchw}: {e:.3e} (fp32 CPU {cpu:.3e})")
    assert e < bound(cpu, BWD_FLOOR)
    if nchw:                                                                                 # accumulate adds to what is there
        base = _rand(*d["src"].shape, seed=16).float()
        acc = eng.xcit_stem_scatter(_dev(d["drows"]), tuple(d["src"].shape), None, True, into=base.cuda()).cpu()
        assert torch.equal(acc, base + got)


def test_the_launches_refuse_what_they_cannot_run(eng):
    z = torch.zeros(8192, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())      # noqa: E731
    capi = eng.capi
    s0 = stat(eng, COUNTER)
    fwd = lambda *, q=p(z), frames=1, T=4, H=2, dh=8, t=p(z): capi.i2v_xcit_attention_f32(q, frames, T, H, dh, t, p(z), p(z), p(z), None)      # noqa: E731
    off = C.c_void_p(z.data_ptr() + 4)
    for kw, why in ((dict(q=None), b"null"), (dict(t=None), b"null"), (dict(dh=6), b"multiple of 4"), (dict(H=1, dh=68), b"wider than 64"),
                    (dict(frames=70000), b"65535"), (dict(frames=40000, T=196, H=8, dh=48), b"2^31"), (dict(q=off), b"alignment")):
        assert fwd(**kw) != 0
        err = capi.i2v_last_error()
        assert b"xcit_attention" in err and b"hipErrorInvalidValue" in err and why in err, err
    assert capi.i2v_xcit_attention_bwd_f32(p(z), p(z), p(z), p(z), 1, 4, 2, 6, p(z), p(z), None) != 0
    assert b"xcit_attention_bwd" in capi.i2v_last_error() and b"multiple of 4" in capi.i2v_last_error()
    dw = lambda *, Cn=8, ts=p(z), y=C.c_void_p(z.data_ptr() + 4096): capi.i2v_xcit_dw3_f32(p(z), 1, 2, 2, Cn, p(z), None, p(z), ts, None, None, None, y, None)      # noqa: E731
    for kw, why in ((dict(Cn=6), b"multiple of 4"), (dict(ts=None), b"both of its arrays"), (dict(y=p(z)), b"overlap")):
        assert dw(**kw) != 0
        assert b"xcit_dw3" in capi.i2v_last_error() and why in capi.i2v_last_error(), capi.i2v_last_error()
    assert capi.i2v_xcit_stem_gather_f32(p(z), None, 1, 5, 5, 3, 1, None) != 0 and b"null" in capi.i2v_last_error()
    assert capi.i2v_xcit_stem_scatter_f32(p(z), p(z), p(z), 1, 5, 5, 3, 1, 0, None) != 0 and b"pre-activation" in capi.i2v_last_error()
    assert stat(eng, COUNTER) == s0                                                # nothing was launched
    spec = graphs.build_tiny(NANO, (64, 64))
    sd = weights.synthetic_state_dict(spec, 0)
    with pytest.raises(_lib.I2VError, match="hooked twice"):
        eng.build_xcit_net(spec, sd, [1, 1], 2)
    with pytest.raises(_lib.I2VError, match="outside"):
        eng.build_xcit_net(spec, sd, [8], 2)
    net = eng.build_xcit_net(spec, sd, [0], 2)
    with pytest.raises(_lib.I2VError, match="planned for"):
        net.forward(torch.zeros(3, 3, 64, 64, device="cuda"))
    net.forward(torch.zeros(2, 3, 64, 64, device="cuda"))                 # the engine goes on
    torch.cuda.synchronize()
    net.close()
    d = mk.attn_case(2, 4, 2, 8)
    assert _rel(run_attn(eng, d)[0], mk.attn_reference(d)[0]) < 1e-6


def _hooks_and_grad(eng, spec, sd, blocks, x, max_frames=None):
    launches = 2 * (max(blocks) + 1)      # per block: one attention launch forward, one backward
    return hooks_and_grad(eng, spec, sd, blocks, x, max_frames, launches=(COUNTER, launches))


def _check(label, feats, gx, ref, x, hg):
    check_net(label, feats, gx, ref.forward(x), ref.backward(hg), FP32[label], NET_FLOOR)


@pytest.mark.parametrize("label", sorted(mk.TWINS))
def test_twin_hooks_at_depths_1_to_4_and_input_gradient(eng, label):
    side = mk.TWINS[label][0]
    spec = graphs.build_tiny(TINY, (side, side))
    assert spec.arch == label
    sd = weights.synthetic_state_dict(spec, 0)
    x = mk.twin_input(label)
    blocks = [spec.hook_for(d) for d in (1, 2, 3, 4)]
    assert blocks == mk.TWIN_HOOKS
    (feats, gx), hg = _hooks_and_grad(eng, spec, sd, blocks, x)
    _check(label, feats, gx, XcitReference(spec, sd, blocks), x, hg)
    (feats2, gx2), _ = _hooks_and_grad(eng, spec, sd, blocks, x, max_frames=5)     # a second net, planned for more frames: the same bits
    assert all(torch.equal(a, b) for a, b in zip(feats, feats2)) and torch.equal(gx, gx2)
    net = eng.build_xcit_net(spec, sd, blocks, 1)                                  # frame 0 of the n-frame run against a 1-frame run
    f1, g1, _ = _run(net, spec, blocks, x[:1], [h[:1] for h in hg])
    net.close()
    assert all(torch.equal(a[:1], b) for a, b in zip(feats, f1)) and torch.equal(gx[:1], g1)
    (fa, _), _ = _hooks_and_grad(eng, spec, sd, [blocks[2]], x)                    # a single hook: the net is truncated there
    assert torch.equal(fa[0], feats[2])


@pytest.mark.parametrize("name", [NANO, TINY])
def test_full_size_model_at_224_depths_1_to_4_against_float64(eng, name):
    spec = graphs.build(name)
    sd = weights.synthetic_state_dict(spec, 0)
    x = _rand(2, 3, 224, 224, seed=22)
    blocks = [spec.hook_for(d) for d in (1, 2, 3, 4)]
    assert blocks == mk.FULL[name]
    (feats, gx), hg = _hooks_and_grad(eng, spec, sd, blocks, x)
    assert feats[3].shape[1] == 196 * spec.dim
    _check(name, feats, gx, XcitReference(spec, sd, blocks), x, hg)


def test_i2v_trajectory_on_the_twin_matches_the_float64_trajectory():
    """10 steps at depth 3.  The depth is chosen by the reference's own float32 error on this clip, measured on the CPU with
    `restate.run_attack` in float32 against float64: 7.2e-6 / 5.8e-5 / 4.0e-5 at depths 1 / 2 / 3, but 2.4e-4 at depth 4 -- there the
    ten Adam steps amplify float32 rounding past the 2e-4 this test holds the costs to, whatever computes them, so depth 4 cannot tell a
    right kernel from a wrong one.  (The single passes at depth 4 are held to float64 in the twin tests above.)"""
    vid = _video(2, 4, 64, 23)
    atk = attacks.ImageGuidedFMDirection_Adam([TINY], depth=3, step_size=0.005, steps=10, graph_builder=graphs.build_tiny, weight_seed=0)
    adv = atk(vid, torch.zeros(2, dtype=torch.long), ["a", "b"]).cpu()
    spec = graphs.build_tiny(TINY, (64, 64))
    check_trajectory(atk, adv, XcitReference(spec, weights.synthetic_state_dict(spec, 0), [spec.hook_for(3)], dtype=torch.float64), vid, rtol=TRAJECTORY_RTOL)


def test_aens_of_the_twin_with_tiny_resnet_matches_the_oracle():
    vid = _video(1, 4, 64, 24)
    depths = {TINY: [1, 4], "resnet": [2, 3]}
    atk = attacks.AENS_I2V_MF([TINY, "resnet"], depths=depths, step_size=0.005, steps=4, momentum=0.5, graph_builder=graphs.build_tiny,
                              weight_seed=0)
    adv, _, costs = atk(vid, torch.zeros(1, dtype=torch.long), ["a"])
    cs, rs = (graphs.build_tiny(n, (64, 64)) for n in (TINY, "resnet"))
    nets = [XcitReference(cs, weights.synthetic_state_dict(cs, 0), [cs.hook_for(d) for d in depths[TINY]], dtype=torch.float64),
            restate.OracleNet(rs, weights.synthetic_state_dict(rs, 0), [rs.hook_for(d, True) for d in depths["resnet"]], dtype=torch.float64)]
    ref = restate.run_attack(nets, vid, steps=4, step_size=0.005, mode="aens", coeffs=torch.ones(4, dtype=torch.float64), momentum=0.5)
    np.testing.assert_allclose(costs, ref["costs"], rtol=2e-4)


def test_workspace_of_xcit_small_at_128_frames_depth_3(eng):
    """The plan the device holds equals the formula the host simulation's plan is checked against (tests/test_xcit_cpu.py) and the figure
    of DESIGN.md section 23."""
    spec = graphs.build("xcit_small_12_p16_224")
    net = eng.build_xcit_net(spec, weights.synthetic_state_dict(spec, 0), [spec.hook_for(3)], 128)
    got = net.workspace_bytes()
    net.close()
    assert got == spec.workspace_bytes([8], 128) == mk.WORKSPACE_SMALL_D3
