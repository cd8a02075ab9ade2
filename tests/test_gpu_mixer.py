"""GPU (-m gpu): timm's MLP-Mixer and ResMLP on the MI355X (include/i2v_mixer.h) -- the fused token-mixing kernel
on its own against float64, the hidden-less cases bit for bit against the host restatement, both channel tiles with the same bits; the
test-size twins, mixer_b16_224 and resmlp_12_224 against the float64 reference (tests/mixer_reference.py); the workspace formula;
repeatability; an I2V trajectory and an ensemble with a CNN and a Swin against `oracle.restate.run_attack`.

Bound: relative L2 against float64, at most the larger of 1e-5 and 4 x the error of the float32 CPU run of the same reference on the same
inputs (tests/golden/mixer_fp32_cpu_errors.json, tests/make_mixer_fixtures.py)."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from i2v_amd import attacks, graphs, weights
from i2v_amd import lib as _lib
from oracle import restate
from tests import make_mixer_fixtures as mk
from tests.family_harness import bound, check_trajectory, hooks_and_grad, rand as _rand, rel as _rel, run_net as _run, stat, video as _video
from tests.mixer_reference import MixerReference
from tests.swin_reference import SwinReference

pytestmark = pytest.mark.gpu
MIXER, RESMLP = "mixer_b16_224", "resmlp_12_224"
SWIN = "swin_tiny_patch4_window7_224"
FP32 = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mixer_fp32_cpu_errors.json")))
FLOOR = 1e-5
COUNTER = b"mixer_tokens_launches"
TRAJECTORY_RTOL = 2e-4      # of the trajectory's costs against the float64 run
ALL_CASES = mk.HIDDEN_CASES + [(S, 0, Cn) for S, Cn in mk.LINEAR_CASES]


@pytest.fixture(scope="module")
def eng():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return attacks.get_engine("cuda:0")


def _dev(d, device):
    return {k: (None if v is None else v.float().to(device).contiguous()) for k, v in d.items()}


def run_case(e, c, tile=0):
    """(out, dz + add) of a token case (tensors on the engine's device) through the two C entries."""
    out = e.mixer_tokens(c["z"], c["residual"], c["w1"], c["b1"], c["w2"], c["b2"], c["in_scale"], c["in_shift"], c["out_scale"], tile)
    dz = e.mixer_tokens_bwd(c["z"], c["g"], c["w1"], c["b1"], c["w2"], c["in_scale"], c["in_shift"], c["out_scale"], c["add"], tile)
    return out, dz


@pytest.mark.parametrize("S,Sh,Cn", ALL_CASES)
@pytest.mark.parametrize("N", [1, 3])
def test_token_kernel_against_float64_and_the_host_restatement(eng, S, Sh, Cn, N):
    d = mk.token_case(S, Sh, Cn, N)
    c = _dev(d, "cuda")
    s0 = stat(eng, COUNTER)
    out, dz = run_case(eng, c)
    torch.cuda.synchronize()
    assert stat(eng, COUNTER) - s0 == 2                                            # one launch per pass
    out, dz = out.cpu(), dz.cpu()
    want, want_dz = mk.token_reference(d)
    fp = FP32["tokens"][mk.case_key(S, Sh, Cn, N)]
    e_f, e_b = _rel(out, want), _rel(dz, want_dz)
    print(f"tokens S {S} Sh {Sh} C {Cn}, {N} frames: forward {e_f:.3e} (fp32 CPU {fp['fwd']:.3e}) input gradient {e_b:.3e} (fp32 CPU {fp['bwd']:.3e})")
    assert e_f < bound(fp["fwd"], FLOOR) and e_b < bound(fp["bwd"], FLOOR)
    out2, dz2 = run_case(eng, c)
    assert torch.equal(out, out2.cpu()) and torch.equal(dz, dz2.cpu())    # reruns: the same bits
    # the other channel tile (where both fit the LDS): the same bits
    if (S + Sh) * 64 * 4 <= 160 * 1024:
        for tile in (32, 64):
            ot, gt = run_case(eng, c, tile)
            assert torch.equal(out, ot.cpu()) and torch.equal(dz, gt.cpu())
    if N == 3:                                                            # frame 0 of the 3-frame launch: the bits of a 1-frame launch
        o1, g1 = run_case(eng, {k: (v[:1].contiguous() if v is not None and v.dim() == 3 else v) for k, v in c.items()})
        assert torch.equal(out[:1], o1.cpu()) and torch.equal(dz[:1], g1.cpu())
    if Sh == 0:
        # the host restatement (csrc/i2v_mixer_host.h): no transcendental without a hidden layer, so bit for bit
        from tests.hostsim_util import hostsim_engine
        hs = hostsim_engine()
        _lib.bind(hs.capi, _lib.MIXER_NODE_PROTOS)
        ho, hg = run_case(hs, _dev(d, "cpu"))
        assert torch.equal(out, ho) and torch.equal(dz, hg)


def test_unaligned_input_takes_the_4_byte_path_with_the_same_bits(eng):
    S, Sh, Cn, N = 49, 24, 68, 2
    c = _dev(mk.token_case(S, Sh, Cn, N), "cuda")
    want, want_dz = run_case(eng, c)
    off = dict(c)
    for k in ("z", "g"):                                                  # 4 bytes off a 16-byte boundary
        pad = torch.empty(c[k].numel() + 1, device="cuda")
        pad[1:] = c[k].reshape(-1)
        off[k] = pad[1:].reshape(N, S, Cn)
        assert off[k].data_ptr() % 16 == 4
    got, got_dz = run_case(eng, off)
    assert torch.equal(got, want) and torch.equal(got_dz, want_dz)


def test_the_launch_refuses_what_it_was_not_planned_for(eng):
    z = torch.zeros(196 * 512, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())      # noqa: E731
    capi = eng.capi
    s0 = stat(eng, COUNTER)
    assert capi.i2v_mixer_tokens_f32(p(z), p(z), p(z), 0, 4, 0, 4, p(z), p(z), None, None, None, None, None, 0, None) != 0
    assert capi.i2v_mixer_tokens_f32(p(z), p(z), p(z), 1, 4, 0, 6, p(z), p(z), None, None, None, None, None, 0, None) != 0
    assert b"i2v_mixer_tokens_f32" in capi.i2v_last_error()
    assert capi.i2v_mixer_tokens_f32(p(z), p(z), p(z), 1, 196, 512, 64, p(z), p(z), p(z), p(z), None, None, None, 64, None) != 0
    assert b"LDS" in capi.i2v_last_error()                                # (196 + 512) rows of 64 channels: 181 248 bytes
    assert capi.i2v_mixer_tokens_f32(p(z), p(z), p(z), 70000, 4, 0, 4, p(z), p(z), None, None, None, None, None, 0, None) != 0
    assert b"65535" in capi.i2v_last_error()
    assert stat(eng, COUNTER) == s0                                                # nothing was launched


def _hooks_and_grad(eng, spec, sd, blocks, x, max_frames=None):
    launches = 2 * (max(blocks) + 1)      # one token launch per block and pass
    return hooks_and_grad(eng, spec, sd, blocks, x, max_frames, launches=(COUNTER, launches))


@pytest.mark.parametrize("twin,name", [("mixer_test", MIXER), ("resmlp_test", RESMLP)])
def test_twin_hooks_at_depths_1_to_4_and_input_gradient(eng, twin, name):
    spec = graphs.build_tiny(name, (64, 64))
    sd = weights.synthetic_state_dict(spec, 0)
    x = _rand(3, 3, 64, 64, seed=21)
    blocks = [spec.hook_for(d) for d in (1, 2, 3, 4)]
    (feats, gx), hg = _hooks_and_grad(eng, spec, sd, blocks, x)
    ref = MixerReference(spec, sd, blocks)
    rf = ref.forward(x)
    errs, gerr = [_rel(a, b) for a, b in zip(feats, rf)], _rel(gx, ref.backward(hg))
    fp = FP32[twin]
    print(f"{twin}: HIP vs float64: hooks {errs} grad {gerr}; fp32 CPU vs float64: {fp}")
    for e, cpu in zip(errs, fp["hooks"]):
        assert e < bound(cpu, FLOOR)
    assert gerr < bound(fp["grad"], FLOOR)
    (feats2, gx2), _ = _hooks_and_grad(eng, spec, sd, blocks, x, max_frames=5)     # a second net, planned for more frames: the same bits
    assert all(torch.equal(a, b) for a, b in zip(feats, feats2)) and torch.equal(gx, gx2)
    net = eng.build_mixer_net(spec, sd, blocks, 1)                                 # frame 0 of the 3-frame run against a 1-frame run
    f1, g1, _ = _run(net, spec, blocks, x[:1], [h[:1] for h in hg])
    net.close()
    assert all(torch.equal(a[:1], b) for a, b in zip(feats, f1)) and torch.equal(gx[:1], g1)
    (fa, _), _ = _hooks_and_grad(eng, spec, sd, [blocks[1]], x)                    # a single mid-stack hook: the net is truncated there
    assert torch.equal(fa[0], feats[1])


@pytest.mark.parametrize("name", [MIXER, RESMLP])
def test_full_size_model_at_224_depths_2_and_4_against_float64(eng, name):
    spec = graphs.build(name)
    sd = weights.synthetic_state_dict(spec, 0)
    x = _rand(2, 3, 224, 224, seed=22)
    blocks = [spec.hook_for(2), spec.hook_for(4)]
    assert blocks == mk.FULL[name]
    (feats, gx), hg = _hooks_and_grad(eng, spec, sd, blocks, x)
    ref = MixerReference(spec, sd, blocks)
    rf = ref.forward(x)
    errs, gerr = [_rel(a, b) for a, b in zip(feats, rf)], _rel(gx, ref.backward(hg))
    fp = FP32[name]
    print(f"{name}: HIP vs float64: hooks {errs} grad {gerr}; fp32 CPU vs float64: {fp}")
    for e, cpu in zip(errs, fp["hooks"]):
        assert e < bound(cpu, FLOOR)
    assert gerr < bound(fp["grad"], FLOOR)


def test_i2v_trajectory_on_the_mixer_twin_matches_the_float64_trajectory():
    vid = _video(2, 4, 64, 23)
    atk = attacks.ImageGuidedFMDirection_Adam([MIXER], depth=3, step_size=0.005, steps=4, graph_builder=graphs.build_tiny, weight_seed=0)
    adv = atk(vid, torch.zeros(2, dtype=torch.long), ["a", "b"]).cpu()
    spec = graphs.build_tiny(MIXER, (64, 64))
    check_trajectory(atk, adv, MixerReference(spec, weights.synthetic_state_dict(spec, 0), [spec.hook_for(3)], dtype=torch.float64), vid, rtol=TRAJECTORY_RTOL, steps=4)


def test_aens_of_the_mixer_twin_with_tiny_resnet_and_tiny_swin_matches_the_oracle():
    vid = _video(1, 4, 64, 24)
    depths = {MIXER: [1, 4], "resnet": [2, 3], SWIN: [2]}
    atk = attacks.AENS_I2V_MF([MIXER, "resnet", SWIN], depths=depths, step_size=0.005, steps=4, momentum=0.5,
                              graph_builder=graphs.build_tiny, weight_seed=0)
    adv, _, costs = atk(vid, torch.zeros(1, dtype=torch.long), ["a"])
    ms, rs, ss = (graphs.build_tiny(n, (64, 64)) for n in (MIXER, "resnet", SWIN))
    nets = [MixerReference(ms, weights.synthetic_state_dict(ms, 0), [ms.hook_for(d) for d in depths[MIXER]], dtype=torch.float64),
            restate.OracleNet(rs, weights.synthetic_state_dict(rs, 0), [rs.hook_for(d, True) for d in depths["resnet"]], dtype=torch.float64),
            SwinReference(ss, weights.synthetic_state_dict(ss, 0), [ss.hook_for(d) for d in depths[SWIN]], dtype=torch.float64)]
    ref = restate.run_attack(nets, vid, steps=4, step_size=0.005, mode="aens", coeffs=torch.ones(5, dtype=torch.float64), momentum=0.5)
    np.testing.assert_allclose(costs, ref["costs"], rtol=2e-4)
