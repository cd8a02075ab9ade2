"""GPU (-m gpu): timm's ConvNeXt family on the MI355X (include/i2v_convnext.h) -- the token-major depthwise 7 x 7
kernel on its own against float64 and, bit for bit, against its host restatement; the test-size twin and convnext_tiny against the
float64 reference (tests/convnext_reference.py); the workspace formula; repeatability; an I2V trajectory and ensembles with a CNN and a
Swin against `oracle.restate.run_attack`.

Bound: relative L2 against float64, at most the larger of 1e-5 and 4 x the error of the float32 CPU run of the same reference on the same
inputs (tests/golden/convnext_fp32_cpu_errors.json, tests/make_convnext_fixtures.py)."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from i2v_amd import attacks, graphs, weights
from i2v_amd import lib as _lib
from oracle import restate
from tests import convnext_reference as cr
from tests import make_convnext_fixtures as mk
from tests.convnext_reference import ConvNextReference
from tests.family_harness import bound, check_trajectory, hooks_and_grad, rand as _rand, rel as _rel, run_net as _run, stat, video as _video
from tests.swin_reference import SwinReference

pytestmark = pytest.mark.gpu
TINY = "convnext_tiny"
SWIN = "swin_tiny_patch4_window7_224"
FP32 = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "convnext_fp32_cpu_errors.json")))
FLOOR = 1e-5
COUNTER = b"convnext_dw_launches"
TRAJECTORY_RTOL = 2e-4      # of the trajectory's costs against the float64 run


@pytest.fixture(scope="module")
def eng():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return attacks.get_engine("cuda:0")


def _node(eng, Cc, H, W, N):
    x, w, b, dy, res = (_rand(N, H, W, Cc, seed=1), _rand(49, Cc, seed=2) / 7, _rand(Cc, seed=3), _rand(N, H, W, Cc, seed=4),
                        _rand(N, H, W, Cc, seed=5))
    xd, wd, bd, dyd, rd = (t.float().cuda().contiguous() for t in (x, w, b, dy, res))
    y = eng.convnext_dw(xd, wd, bd)
    gx = eng.convnext_dw(dyd, wd.flip(0).contiguous(), None, rd)           # the input gradient: mirrored filter, + the residual path
    torch.cuda.synchronize()
    return (x, w, b, dy, res), y.cpu(), gx.cpu()


@pytest.mark.parametrize("Cc,H,W", mk.NODE_CASES)
@pytest.mark.parametrize("N", [1, 3])
def test_depthwise_kernel_against_float64_and_the_host_restatement(eng, Cc, H, W, N):
    s0 = stat(eng, COUNTER)
    (x, w, b, dy, res), y, gx = _node(eng, Cc, H, W, N)
    assert stat(eng, COUNTER) - s0 == 2
    xr = x.clone().requires_grad_(True)
    ref = cr.dwconv_token_major(xr, w, b)
    want_gx = torch.autograd.grad(ref, xr, dy)[0] + res.float().double()
    fp = FP32["nodes"][f"{Cc}x{H}x{W}x{N}"]
    e_f, e_b = _rel(y, ref.detach()), _rel(gx, want_gx)
    print(f"dw {Cc} x {H} x {W}, {N} frames: forward {e_f:.3e} (fp32 CPU {fp['fwd']:.3e}) input gradient {e_b:.3e} (fp32 CPU {fp['bwd']:.3e})")
    assert e_f < bound(fp["fwd"], FLOOR) and e_b < bound(fp["bwd"], FLOOR)
    _, y2, gx2 = _node(eng, Cc, H, W, N)
    assert torch.equal(y, y2) and torch.equal(gx, gx2)                    # reruns: the same bits
    # the host restatement (csrc/i2v_convnext_host.h): no transcendental in the launch, so bit for bit
    from tests.hostsim_util import hostsim_engine
    hs = hostsim_engine()
    _lib.bind(hs.capi, _lib.CONVNEXT_NODE_PROTOS)
    hy = hs.convnext_dw(x.float().contiguous(), w.float().contiguous(), b.float().contiguous())
    hgx = hs.convnext_dw(dy.float().contiguous(), w.float().flip(0).contiguous(), None, res.float().contiguous())
    assert torch.equal(y, hy) and torch.equal(gx, hgx)
    if N == 3:                                                            # frame 0 of the 3-frame launch: the bits of a 1-frame launch
        y1 = eng.convnext_dw(x[:1].float().cuda().contiguous(), w.float().cuda(), b.float().cuda()).cpu()
        assert torch.equal(y[:1], y1)


def test_unaligned_arrays_take_the_4_byte_path_with_the_same_bits(eng):
    Cc, H, W, N = 8, 5, 9, 2
    x, w, b = _rand(N, H, W, Cc, seed=1).float(), (_rand(49, Cc, seed=2) / 7).float(), _rand(Cc, seed=3).float()
    want = eng.convnext_dw(x.cuda(), w.cuda(), b.cuda()).cpu()
    pad = torch.empty(x.numel() + 1, device="cuda")
    pad[1:] = x.cuda().reshape(-1)
    got = eng.convnext_dw(pad[1:].reshape(N, H, W, Cc), w.cuda(), b.cuda()).cpu()      # x 4 bytes off a 16-byte boundary
    assert torch.equal(got, want)


def test_the_launch_refuses_what_it_was_not_planned_for(eng):
    z = torch.zeros(64, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())      # noqa: E731
    capi = eng.capi
    assert capi.i2v_convnext_dw_f32(p(z), p(z), None, None, p(z), 0, 1, 1, 1, None) != 0
    assert capi.i2v_convnext_dw_f32(p(z), p(z), None, None, p(z), 70000, 1, 1, 1, None) != 0          # a grid dimension over 65535
    assert b"65535" in capi.i2v_last_error()
    assert capi.i2v_convnext_dw_f32(p(z), p(z), None, None, p(z), 4096, 1024, 1024, 1, None) != 0      # more than 2^31 elements
    assert b"2^31" in capi.i2v_last_error()


def _hooks_and_grad(eng, spec, sd, stages, x):
    launches = 2 * sum(spec.depths[:max(stages) + 1])      # one depthwise launch per block and pass
    return hooks_and_grad(eng, spec, sd, stages, x, launches=(COUNTER, launches))


def test_tiny_twin_hooks_at_depths_1_to_4_and_input_gradient(eng):
    spec = graphs.build_tiny(TINY, (64, 64))
    sd = weights.synthetic_state_dict(spec, 0)
    x = _rand(3, 3, 64, 64, seed=21)
    stages = [spec.hook_for(d) for d in (1, 2, 3, 4)]
    (feats, gx), hg = _hooks_and_grad(eng, spec, sd, stages, x)
    ref = ConvNextReference(spec, sd, stages)
    rf = ref.forward(x)
    errs, gerr = [_rel(a, b) for a, b in zip(feats, rf)], _rel(gx, ref.backward(hg))
    fp = FP32["convnext_test"]
    print(f"convnext_test: HIP vs float64: hooks {errs} grad {gerr}; fp32 CPU vs float64: {fp}")
    for e, cpu in zip(errs, fp["hooks"]):
        assert e < bound(cpu, FLOOR)
    assert gerr < bound(fp["grad"], FLOOR)
    (feats2, gx2), _ = _hooks_and_grad(eng, spec, sd, stages, x)                 # repeatability: a second net, the same bits
    assert all(torch.equal(a, b) for a, b in zip(feats, feats2)) and torch.equal(gx, gx2)
    # frame 0 of the 3-frame run against a 1-frame run
    net = eng.build_convnext_net(spec, sd, stages, 1)
    f1, g1, _ = _run(net, spec, stages, x[:1], [h[:1] for h in hg])
    net.close()
    assert all(torch.equal(a[:1], b) for a, b in zip(feats, f1)) and torch.equal(gx[:1], g1)
    # a single hooked stage below the deepest possible: the net is truncated there
    (fa, _), _ = _hooks_and_grad(eng, spec, sd, [1], x)
    assert torch.equal(fa[0], feats[1])


def test_convnext_tiny_at_224_depth_3_against_float64(eng):
    spec = graphs.build(TINY)
    sd = weights.synthetic_state_dict(spec, 0)
    x = _rand(2, 3, 224, 224, seed=22)
    stages = [spec.hook_for(3)]
    (feats, gx), hg = _hooks_and_grad(eng, spec, sd, stages, x)
    ref = ConvNextReference(spec, sd, stages)
    rf = ref.forward(x)
    err, gerr = _rel(feats[0], rf[0]), _rel(gx, ref.backward(hg))
    fp = FP32["convnext_tiny"]
    print(f"convnext_tiny: HIP vs float64: hook {err} grad {gerr}; fp32 CPU vs float64: {fp}")
    assert err < bound(fp["hooks"][0], FLOOR)
    assert gerr < bound(fp["grad"], FLOOR)


def test_fewer_frames_on_a_used_handle_give_the_bits_of_a_fresh_one(eng):
    spec = graphs.build_tiny(TINY, (64, 64))
    sd = weights.synthetic_state_dict(spec, 0)
    big, small = _rand(5, 3, 64, 64, seed=41), _rand(2, 3, 64, 64, seed=42)
    hg = [_rand(2, spec.hook_dim(s), seed=43 + s) for s in (0, 3)]
    used = eng.build_convnext_net(spec, sd, [0, 3], 5)
    _run(used, spec, [0, 3], big)
    f1, g1, _ = _run(used, spec, [0, 3], small, hg)
    used.close()
    fresh = eng.build_convnext_net(spec, sd, [0, 3], 2)
    f2, g2, _ = _run(fresh, spec, [0, 3], small, hg)
    fresh.close()
    assert all(torch.equal(a, b) for a, b in zip(f1, f2)) and torch.equal(g1, g2)


def test_i2v_trajectory_on_the_tiny_twin_matches_the_float64_trajectory():
    vid = _video(2, 4, 64, 23)
    atk = attacks.ImageGuidedFMDirection_Adam([TINY], depth=3, step_size=0.005, steps=10, graph_builder=graphs.build_tiny, weight_seed=0)
    adv = atk(vid, torch.zeros(2, dtype=torch.long), ["a", "b"]).cpu()
    spec = graphs.build_tiny(TINY, (64, 64))
    check_trajectory(atk, None, ConvNextReference(spec, weights.synthetic_state_dict(spec, 0), [spec.hook_for(3)], dtype=torch.float64), vid, rtol=TRAJECTORY_RTOL)
    mean = torch.tensor(restate.MEAN).view(1, 3, 1, 1, 1)
    std = torch.tensor(restate.STD).view(1, 3, 1, 1, 1)
    a, o = adv * std + mean, vid * std + mean
    assert float((a - o).abs().max()) <= 16 / 255 + 1e-6
    assert float(a.min()) >= -1e-6 and float(a.max()) <= 1 + 1e-6


def test_aens_of_the_twin_with_tiny_resnet_and_tiny_swin_matches_the_oracle():
    vid = _video(1, 4, 64, 24)
    depths = {TINY: [1, 4], "resnet": [2, 3], SWIN: [2]}
    atk = attacks.AENS_I2V_MF([TINY, "resnet", SWIN], depths=depths, step_size=0.005, steps=4, momentum=0.5,
                              graph_builder=graphs.build_tiny, weight_seed=0)
    adv, _, costs = atk(vid, torch.zeros(1, dtype=torch.long), ["a"])
    cs, rs, ss = (graphs.build_tiny(n, (64, 64)) for n in (TINY, "resnet", SWIN))
    nets = [ConvNextReference(cs, weights.synthetic_state_dict(cs, 0), [cs.hook_for(d) for d in depths[TINY]], dtype=torch.float64),
            restate.OracleNet(rs, weights.synthetic_state_dict(rs, 0), [rs.hook_for(d, True) for d in depths["resnet"]], dtype=torch.float64),
            SwinReference(ss, weights.synthetic_state_dict(ss, 0), [ss.hook_for(d) for d in depths[SWIN]], dtype=torch.float64)]
    ref = restate.run_attack(nets, vid, steps=4, step_size=0.005, mode="aens", coeffs=torch.ones(5, dtype=torch.float64), momentum=0.5)
    np.testing.assert_allclose(costs, ref["costs"], rtol=2e-4)
    np.testing.assert_allclose(np.stack(atk.weights), np.stack(ref["weights"]), rtol=1e-4, atol=1e-6)


def test_ens_with_a_cnn_a_swin_and_a_convnext_together():
    vid = _video(1, 4, 64, 26)
    names = ["resnet", SWIN, TINY]
    atk = attacks.ImageGuidedFML2_Adam_MultiModels(names, depths={n: 2 for n in names}, steps=4, graph_builder=graphs.build_tiny, weight_seed=0)
    atk(vid, torch.zeros(1, dtype=torch.long), ["a"])
    gs = [graphs.build_tiny(n, (64, 64)) for n in names]
    sds = [weights.synthetic_state_dict(g, 0) for g in gs]
    nets = [restate.OracleNet(gs[0], sds[0], [gs[0].hook_for(2)], dtype=torch.float64),
            SwinReference(gs[1], sds[1], [gs[1].hook_for(2)], dtype=torch.float64),
            ConvNextReference(gs[2], sds[2], [gs[2].hook_for(2)], dtype=torch.float64)]
    ref = restate.run_attack(nets, vid, steps=4, step_size=0.005)
    np.testing.assert_allclose(atk.last_costs, ref["costs"], rtol=2e-4)
