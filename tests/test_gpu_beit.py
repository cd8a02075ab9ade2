"""GPU (-m gpu): timm's BEiT on the MI355X (include/i2v_beit.h) -- the biased global attention kernel on its own,
forward and backward, against float64 autograd of timm's literal arithmetic on the shapes of tests/make_beit_fixtures.ATTN_CASES (a single
key; one tile and one key past it; a ragged T; the workload's shape; the limit of 208; a hot case; a null bias), out, dq, dk and dv each
at its own bound; the device entries against their scalar host twins; the refusals, with the engine going on afterwards; the three
test-size twins and beit_base_patch16_224 against the float64 reference (tests/beit_reference.py); the shared-launch route under
I2V_BEIT_ATTN=0; repeatability; frame 0 of an n-frame call against a 1-frame call; the launch counter; a 10-step I2V trajectory against
`oracle.restate.run_attack`; the workspace figure.

Bound: relative L2 against float64, at most the larger of the floor for that kind of case (entries 1e-6 forward, 1e-5 backward; nets
1e-5) and 4 x the error of the float32 CPU run of the same reference on the same inputs (tests/golden/beit_fp32_cpu_errors.json,
tests/make_beit_fixtures.py).  A case without a recorded error fails (KeyError)."""
import ctypes as C
import json
import os

import pytest
import torch

from i2v_amd import attacks, graphs, weights
from i2v_amd import lib as _lib
from tests import make_beit_fixtures as mk
from tests.beit_reference import BeitReference
from tests.family_harness import bound, check_net, check_trajectory, hooks_and_grad, rand as _rand, rel as _rel, run_net as _run, stat

pytestmark = pytest.mark.gpu
BASE = "beit_base_patch16_224"
FP32 = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "beit_fp32_cpu_errors.json")))
NET_FLOOR, FWD_FLOOR, BWD_FLOOR = 1e-5, 1e-6, 1e-5
COUNTER = b"beit_attention_launches"
TRAJECTORY_RTOL = 2e-4      # of the trajectory's costs against the float64 run


@pytest.fixture(scope="module")
def eng():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return attacks.get_engine("cuda:0")


@pytest.fixture(scope="module")
def host():
    """The scalar host twins of the launches (csrc/i2v_beit_host.h), in the host simulation."""
    from tests.hostsim_util import hostsim_engine
    e = hostsim_engine()
    _lib.bind(e.capi, _lib._BEIT_PROTOS)
    return e


def _dev(v):
    return None if v is None else v.float().cuda().contiguous()


def _f(v):
    return None if v is None else v.float().contiguous()


def _split(out, dqkv):
    Cn = dqkv.shape[2] // 3
    return out, dqkv[:, :, :Cn], dqkv[:, :, Cn:2 * Cn], dqkv[:, :, 2 * Cn:]


def run_attn(eng, d):
    """(out, dq, dk, dv) of an attention case through the two C entries, back on the host."""
    qkv, bias = _dev(d["qkv"]), _dev(d["bias"])
    out = eng.beit_attention(qkv, bias, d["heads"])
    dqkv = eng.beit_attention_bwd(qkv, bias, _dev(d["dout"]), d["heads"])
    torch.cuda.synchronize()
    return _split(out.cpu(), dqkv.cpu())


@pytest.mark.parametrize("F,T,H,dh,kind", mk.ATTN_CASES)
def test_attention_kernel_against_float64_autograd(eng, host, F, T, H, dh, kind):
    d = mk.attn_case(F, T, H, dh, kind)
    s0 = stat(eng, COUNTER)
    got = run_attn(eng, d)
    assert stat(eng, COUNTER) - s0 == 3                                            # one launch forward; backward two: dq, then dk / dv
    want = mk.attn_reference(d)
    fp = FP32["attention"][mk.case_key(F, T, H, dh, kind)]
    errs = {"fwd": _rel(got[0], want[0]), "dv": _rel(got[3], want[3])}
    if T == 1:                                                            # a single key: P = 1 exactly, so dS = 0: dq and dk are exactly 0
        assert float(got[1].abs().max()) == 0.0 and float(got[2].abs().max()) == 0.0
    else:
        errs.update({"dq": _rel(got[1], want[1]), "dk": _rel(got[2], want[2])})
    print(f"beit attention F {F} T {T} H {H} dh {dh} {kind}: " + ", ".join(f"{k} {v:.3e} (fp32 CPU {fp[k]:.3e})" for k, v in errs.items()))
    for k, v in errs.items():
        assert v < bound(fp[k], FWD_FLOOR if k == "fwd" else BWD_FLOOR), (k, v, fp[k])
    again = run_attn(eng, d)
    assert all(torch.equal(a, b) for a, b in zip(got, again))             # reruns: the same bits
    if F > 1:                                                             # frame 0 of the F-frame call: the bits of a 1-frame call
        one = run_attn(eng, dict(d, qkv=d["qkv"][:1], dout=d["dout"][:1]))
        assert all(torch.equal(a[:1], b) for a, b in zip(got, one))
    ho = host.beit_attention(_f(d["qkv"]), _f(d["bias"]), H)              # the device entries against their scalar host twins
    hg = _split(ho, host.beit_attention_bwd(_f(d["qkv"]), _f(d["bias"]), _f(d["dout"]), H))
    for k, a, b in zip(("fwd", "dq", "dk", "dv"), got, hg):
        if T == 1 and k in ("dq", "dk"):
            assert torch.equal(a, b)
        else:
            assert _rel(a, b) < bound(fp[k], FWD_FLOOR if k == "fwd" else BWD_FLOOR), k


@pytest.mark.parametrize("F,H,T", [(1, 1, 1), (3, 2, 37), (2, 3, 197)])
def test_bias_add_launch_is_exact(eng, F, H, T):
    """One element, a ragged shape of more than one block, and the workload's rows: S += bias, bit for bit, padding columns included."""
    ld = (T + 3) // 4 * 4
    S, b = _rand(F, H, T, ld, seed=1).float(), _rand(H, T, ld, seed=2).float()
    got = eng.beit_bias_add(S.cuda(), b.cuda())
    torch.cuda.synchronize()
    assert torch.equal(got.cpu(), S + b)


def test_the_launches_refuse_what_they_cannot_run(eng):
    z = torch.zeros(65536, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())      # noqa: E731
    capi = eng.capi
    s0 = stat(eng, COUNTER)
    fwd = lambda *, qkv=p(z), bias=p(z), frames=1, T=4, H=2, dh=8, out=p(z): capi.i2v_beit_attention_f32(qkv, bias, frames, T, H, dh, 0.5, out, None)      # noqa: E731
    off = C.c_void_p(z.data_ptr() + 4)
    for kw, why in ((dict(T=209, H=1), b"more than 208 tokens"), (dict(H=1, dh=68), b"wider than 64"), (dict(dh=6), b"multiple of 4"),
                    (dict(frames=70000), b"65535"), (dict(H=70000, dh=4), b"65535"), (dict(frames=60000, T=197, H=3, dh=64), b"2^31"),
                    (dict(qkv=None), b"null"), (dict(out=None), b"null"), (dict(qkv=off), b"alignment"), (dict(bias=off), b"alignment"),
                    (dict(out=off), b"alignment")):
        assert fwd(**kw) != 0
        err = capi.i2v_last_error()
        assert b"beit_attention" in err and b"hipErrorInvalidValue" in err and why in err, err
    bwd = lambda *, dh=8, T=4, g=p(z), dqkv=p(z): capi.i2v_beit_attention_bwd_f32(p(z), p(z), g, 1, T, 2, dh, 0.5, dqkv, None)      # noqa: E731
    for kw, why in ((dict(T=209), b"more than 208 tokens"), (dict(dh=68), b"wider than 64"), (dict(dh=6), b"multiple of 4"), (dict(g=None), b"null"),
                    (dict(dqkv=None), b"null"), (dict(dqkv=off), b"alignment")):
        assert bwd(**kw) != 0
        assert b"beit_attention_bwd" in capi.i2v_last_error() and why in capi.i2v_last_error()
    assert stat(eng, COUNTER) == s0                                                # nothing was launched
    spec = graphs.build_tiny(BASE, (64, 64))
    sd = weights.synthetic_state_dict(spec, 0)
    with pytest.raises(_lib.I2VError, match="hooked twice"):
        eng.build_beit_net(spec, sd, [1, 1], 2)
    with pytest.raises(_lib.I2VError, match="outside"):
        eng.build_beit_net(spec, sd, [8], 2)
    net = eng.build_beit_net(spec, sd, [1], 2)
    with pytest.raises(_lib.I2VError, match="planned for"):
        net.forward(torch.zeros(3, 3, 64, 64, device="cuda"))
    net.forward(torch.zeros(2, 3, 64, 64, device="cuda"))                 # the engine goes on
    torch.cuda.synchronize()
    net.close()
    d = mk.attn_case(2, 16, 2, 8)
    assert _rel(run_attn(eng, d)[0], mk.attn_reference(d)[0]) < 1e-6


def _hooks_and_grad(eng, spec, sd, hooks, x, max_frames=None):
    launches = 3 * (max(hooks) + 1)      # per block: one attention launch forward, two backward
    return hooks_and_grad(eng, spec, sd, hooks, x, max_frames, launches=(COUNTER, launches))


def _check(label, feats, gx, ref, x, hg):
    check_net(label, feats, gx, ref.forward(x), ref.backward(hg), FP32[label], NET_FLOOR)


@pytest.mark.parametrize("label", sorted(mk.TWINS))
def test_twin_hooks_at_depths_1_to_4_and_input_gradient(eng, label):
    name, side, _ = mk.TWINS[label]
    spec = graphs.build_tiny(name, (side, side))
    assert spec.arch == label
    sd = weights.synthetic_state_dict(spec, 0)
    x = mk.twin_input(label)
    hooks = [spec.hook_for(d) for d in (1, 2, 3, 4)]
    (feats, gx), hg = _hooks_and_grad(eng, spec, sd, hooks, x)
    _check(label, feats, gx, BeitReference(spec, sd, hooks), x, hg)
    (feats2, gx2), _ = _hooks_and_grad(eng, spec, sd, hooks, x, max_frames=5)      # a second net, planned for more frames: the same bits
    assert all(torch.equal(a, b) for a, b in zip(feats, feats2)) and torch.equal(gx, gx2)
    net = eng.build_beit_net(spec, sd, hooks, 1)                                   # frame 0 of the n-frame run against a 1-frame run
    f1, g1, _ = _run(net, spec, hooks, x[:1], [h[:1] for h in hg])
    net.close()
    assert all(torch.equal(a[:1], b) for a, b in zip(feats, f1)) and torch.equal(gx[:1], g1)
    (fa, _), _ = _hooks_and_grad(eng, spec, sd, [hooks[2]], x)                     # a single hook: the net is truncated there
    assert torch.equal(fa[0], feats[2])


@pytest.mark.parametrize("label", ["beit_test_96", "beit_test_224"])
def test_twin_on_the_shared_launch_route(eng, label, monkeypatch):
    """I2V_BEIT_ATTN=0, read when the net is planned: the core on vit_gemm + the bias add + vit_softmax + vit_gemm with P kept, backward
    the softmax backward and four products.  The same bound against float64; no attention launch is counted; the plan equals the
    formula under the switch; frame 0 has the bits of a 1-frame run."""
    name, side, _ = mk.TWINS[label]
    spec = graphs.build_tiny(name, (side, side))
    sd, x = weights.synthetic_state_dict(spec, 0), mk.twin_input(label)
    hooks = [spec.hook_for(d) for d in (1, 2, 3, 4)]
    monkeypatch.setenv("I2V_BEIT_ATTN", "0")
    net = eng.build_beit_net(spec, sd, hooks, x.shape[0])
    assert net.workspace_bytes() == spec.workspace_bytes(hooks, x.shape[0]) > spec.workspace_bytes(hooks, x.shape[0], composed=False)
    s0 = stat(eng, COUNTER)
    feats, gx, hg = _run(net, spec, hooks, x)
    assert stat(eng, COUNTER) == s0
    net.close()
    _check(label, feats, gx, BeitReference(spec, sd, hooks), x, hg)
    net = eng.build_beit_net(spec, sd, hooks, 1)
    f1, g1, _ = _run(net, spec, hooks, x[:1], [h[:1] for h in hg])
    net.close()
    assert all(torch.equal(a[:1], b) for a, b in zip(feats, f1)) and torch.equal(gx[:1], g1)


@pytest.mark.parametrize("name", mk.FULL)
def test_full_size_model_at_224_depths_1_to_4_against_float64(eng, name):
    spec = graphs.build(name)
    sd = weights.synthetic_state_dict(spec, 0)
    x = mk.full_input()
    hooks = [spec.hook_for(d) for d in (1, 2, 3, 4)]
    (feats, gx), hg = _hooks_and_grad(eng, spec, sd, hooks, x)
    assert all(f.shape[1] == 197 * spec.dim for f in feats)
    _check(name, feats, gx, BeitReference(spec, sd, hooks), x, hg)


def test_i2v_trajectory_on_the_twin_matches_the_float64_trajectory():
    """10 steps at the depth and on the twin of `make_beit_fixtures.TRAJECTORY`, costs within the 2e-4 the XCiT and Twins trajectory
    tests hold.  The float32 reference itself stays under that bound there, measured on the CPU with `restate.run_attack` in float32
    against float64 (tests/golden/beit_fp32_cpu_errors.json, "trajectory")."""
    label, depth = mk.TRAJECTORY
    name, side, _ = mk.TWINS[label]
    clip = mk.TRAJECTORY_CLIPS[label]
    assert FP32["trajectory"][label][str(depth)] < 2e-4                   # the float32 reference itself holds the bound there
    vid = mk.video(*clip)
    atk = attacks.ImageGuidedFMDirection_Adam([name], depth=depth, step_size=0.005, steps=10, graph_builder=graphs.build_tiny, weight_seed=0)
    adv = atk(vid, torch.zeros(clip[0], dtype=torch.long), ["a", "b"]).cpu()
    spec = graphs.build_tiny(name, (side, side))
    assert spec.arch == label
    check_trajectory(atk, adv, BeitReference(spec, weights.synthetic_state_dict(spec, 0), [spec.hook_for(depth)], dtype=torch.float64), vid, rtol=TRAJECTORY_RTOL)


def test_workspace_of_beit_base_at_128_frames_depth_3(eng):
    """The plan the device holds equals the formula the host simulation's plan is checked against (tests/test_beit_cpu.py)."""
    spec = graphs.build(BASE)
    net = eng.build_beit_net(spec, weights.synthetic_state_dict(spec, 0), [spec.hook_for(3)], 128)
    got = net.workspace_bytes()
    net.close()
    assert got == spec.workspace_bytes([8], 128)
