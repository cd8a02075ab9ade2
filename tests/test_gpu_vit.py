"""GPU (-m gpu): the ViT surrogate (`vit_base_patch16_224`, include/i2v_vit.h) on the MI355X -- every new kernel against float64 torch
on awkward shapes (197 and 17 tokens, widths that are not a multiple of the 128-wide tile), the tiny and the full model's hooks and input
gradient against the float64 restatement (tests/vit_reference.py), I2V / AENS trajectories against `oracle.restate.run_attack`,
repeatability, and `image_main.py` end to end."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from i2v_amd import attacks, graphs, weights
from i2v_amd import lib as _lib
from oracle import restate
from tests.family_harness import check_trajectory, hooks_and_grad, rand as _rand, rel as _rel, video as _video
from tests.vit_reference import VitReference, gelu, layer_norm

pytestmark = pytest.mark.gpu
TRAJECTORY_RTOL = 2e-4      # of the trajectory's costs against the float64 run
VIT = graphs.VIT_NAME


@pytest.fixture(scope="module")
def eng():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return attacks.get_engine("cuda:0")


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


@pytest.mark.parametrize("M,K,N", [(2 * 197, 72, 200), (2 * 17, 768, 132), (197, 3072, 768)])
def test_linear_and_gelu_epilogues_against_float64(eng, M, K, N):
    capi, st = eng.capi, eng.stream()
    x, W, b, r = _rand(M, K, seed=1), _rand(N, K, seed=2, scale=K ** -0.5), _rand(N, seed=3), _rand(M, N, seed=4)
    d = [t.float().cuda() for t in (x, W, b, r)]
    y, g = torch.empty(M, N, device="cuda"), torch.empty(M, N, device="cuda")
    _lib.check(capi, capi.i2v_vit_linear_f32(_p(d[0]), M, K, _p(d[1]), _p(d[2]), N, _p(d[3]), _p(y), _p(g), st))
    ref = x @ W.T + b + r
    assert _rel(y, ref) < 1e-6 and _rel(g, gelu(ref)) < 1e-6
    # backward: dx = (dy W) * gelu'(pre)
    dy, pre = _rand(M, N, seed=5), _rand(M, K, seed=6)
    dd, pd = dy.float().cuda(), pre.float().cuda()
    dx = torch.empty(M, K, device="cuda")
    _lib.check(capi, capi.i2v_vit_linear_bwd_f32(_p(dd), M, N, _p(d[1]), K, _p(pd), _p(dx), st))
    pr = pre.clone().requires_grad_(True)
    gprime = torch.autograd.grad(gelu(pr).sum(), pr)[0]
    assert _rel(dx, (dy @ W) * gprime) < 1e-6


@pytest.mark.parametrize("rows,Cw", [(2 * 197, 768), (3 * 17, 72), (5, 70)])
def test_layernorm_forward_and_backward(eng, rows, Cw):
    capi, st = eng.capi, eng.stream()
    x, w, b = _rand(rows, Cw, seed=7) * 3 + 1, 1 + 0.1 * _rand(Cw, seed=8), _rand(Cw, seed=9)
    xd, wd, bd = x.float().cuda(), w.float().cuda(), b.float().cuda()
    out, mean, rstd = torch.empty(rows, Cw, device="cuda"), torch.empty(rows, device="cuda"), torch.empty(rows, device="cuda")
    _lib.check(capi, capi.i2v_vit_layernorm_f32(_p(xd), rows, Cw, _p(wd), _p(bd), 1e-6, _p(out), _p(mean), _p(rstd), st))
    xr = x.clone().requires_grad_(True)
    ref = layer_norm(xr, w, b, 1e-6)
    assert _rel(out, ref.detach()) < 1e-6
    dy, a0, a1 = _rand(rows, Cw, seed=10), _rand(rows, Cw, seed=11), _rand(rows, Cw, seed=12)
    dx, dyd, a1d = a0.float().cuda(), dy.float().cuda(), a1.float().cuda()      # dx aliases add0
    _lib.check(capi, capi.i2v_vit_layernorm_bwd_f32(_p(dyd), _p(xd), _p(mean), _p(rstd), _p(wd), rows, Cw, _p(dx), _p(a1d), _p(dx), st))
    gref = torch.autograd.grad(ref, xr, dy)[0] + a0 + a1
    assert _rel(dx, gref) < 1e-5


@pytest.mark.parametrize("F,T,H,dh", [(2, 197, 12, 64), (3, 17, 2, 32), (1, 17, 3, 36)])
def test_attention_forward_and_backward(eng, F, T, H, dh):
    capi, st = eng.capi, eng.stream()
    Cw, ld = H * dh, capi.i2v_vit_probs_ld(T)
    qkv = _rand(F, T, 3 * Cw, seed=13, scale=1.5)
    qd = qkv.float().cuda()
    probs, out = torch.zeros(F, H, T, ld, device="cuda"), torch.empty(F, T, Cw, device="cuda")
    scale = dh ** -0.5
    _lib.check(capi, capi.i2v_vit_attention_f32(_p(qd), F, T, H, dh, scale, _p(probs), _p(out), st))
    qr = qkv.clone().requires_grad_(True)
    q, k, v = qr.reshape(F, T, 3, H, dh).permute(2, 0, 3, 1, 4)
    att = torch.softmax(q @ k.transpose(-2, -1) * scale, -1)
    ref = (att @ v).transpose(1, 2).reshape(F, T, Cw)
    assert _rel(probs[..., :T], att.detach()) < 1e-6 and _rel(out, ref.detach()) < 1e-6
    dout = _rand(F, T, Cw, seed=14)
    dP, dqkv = torch.empty_like(probs), torch.empty(F, T, 3 * Cw, device="cuda")
    dod = dout.float().cuda()
    _lib.check(capi, capi.i2v_vit_attention_bwd_f32(_p(qd), _p(probs), _p(dod), F, T, H, dh, scale, _p(dP), _p(dqkv), st))
    assert _rel(dqkv, torch.autograd.grad(ref, qr, dout)[0]) < 1e-5


@pytest.mark.parametrize("F,g,dim", [(2, 14, 768), (3, 1, 72)])
def test_token_assembly_and_its_backward(eng, F, g, dim):
    capi, st = eng.capi, eng.stream()
    P = 16
    img, W, b = _rand(F, 3, g * P, g * P, seed=15), _rand(dim, 3, P, P, seed=16, scale=0.05), _rand(dim, seed=17)
    cls, pos = _rand(dim, seed=18), _rand(1 + g * g, dim, seed=19)
    dev = [t.float().cuda().contiguous() for t in (img, W, b, cls, pos)]
    patches, emb = torch.empty(F * g * g, 3 * P * P, device="cuda"), torch.empty(F * g * g, dim, device="cuda")
    tok = torch.empty(F, 1 + g * g, dim, device="cuda")
    _lib.check(capi, capi.i2v_vit_embed_f32(*map(_p, dev[:1]), F, 3, g, P, *map(_p, dev[1:]), dim, _p(patches), _p(emb), _p(tok), st))
    ir = img.clone().requires_grad_(True)
    p = torch.nn.functional.conv2d(ir, W, b, stride=P).flatten(2).transpose(1, 2)
    ref = torch.cat([cls.view(1, 1, -1).expand(F, 1, dim), p], 1) + pos
    assert _rel(tok, ref.detach()) < 1e-6
    dt = _rand(F, 1 + g * g, dim, seed=20)
    gimg = torch.ones(F, 3, g * P, g * P, device="cuda")
    dtd = dt.float().cuda()
    _lib.check(capi, capi.i2v_vit_embed_bwd_f32(_p(dtd), F, 3, g, P, _p(dev[1]), dim, _p(patches), _p(gimg), 1, st))
    assert _rel(gimg - 1, torch.autograd.grad(ref, ir, dt)[0]) < 1e-5


def _hooks_and_grad(eng, spec, sd, blocks, x):
    return hooks_and_grad(eng, spec, sd, blocks, x)


def test_tiny_vit_hooks_and_input_gradient(eng):
    spec = graphs.build_tiny(VIT, (64, 64))
    sd = weights.synthetic_state_dict(spec, 0)
    x = _rand(3, 3, 64, 64, seed=21)
    (feats, gx), hg = _hooks_and_grad(eng, spec, sd, [2, 5], x)
    ref = VitReference(spec, sd, [2, 5])
    rf = ref.forward(x)
    for a, b in zip(feats, rf):
        assert _rel(a, b) < 2e-5
    assert _rel(gx, ref.backward(hg)) < 2e-4


def test_full_vit_b16_hooks_and_input_gradient(eng):
    """ViT-B/16 at 224^2, 2 frames, synthetic weights, hooks at d = 1..4, against float64: 2e-4 relative L2 for the hooks, 1e-3 for the
    input gradient.  An fp32 CPU run of the restatement is far inside both (measured on an MI355X host: 8.8e-7 hooks, 2.1e-6 gradient;
    this path: 1.5e-6 and 3.3e-6), so the bounds stand as set, not doubled."""
    spec = graphs.build(VIT)
    sd = weights.synthetic_state_dict(spec, 0)
    x = _rand(2, 3, 224, 224, seed=22)
    blocks = [spec.hook_for(d) for d in (1, 2, 3, 4)]
    (feats, gx), hg = _hooks_and_grad(eng, spec, sd, blocks, x)
    ref = VitReference(spec, sd, blocks)
    rf = ref.forward(x)
    rg = ref.backward(hg)
    f32 = VitReference(spec, sd, blocks, dtype=torch.float32)
    f32f = f32.forward(x)
    f32g = f32.backward(hg)
    print("fp32 CPU vs float64: hooks", [_rel(a, b) for a, b in zip(f32f, rf)], "grad", _rel(f32g, rg))
    errs = [_rel(a, b) for a, b in zip(feats, rf)]
    print("HIP vs float64: hooks", errs, "grad", _rel(gx, rg))
    assert max(errs) < 2e-4
    assert _rel(gx, rg) < 1e-3


def test_i2v_trajectory_on_the_tiny_vit_matches_the_restatement():
    vid = _video(2, 4, 64, 23)
    atk = attacks.ImageGuidedFMDirection_Adam([VIT], depth=2, step_size=0.005, steps=10, graph_builder=graphs.build_tiny, weight_seed=0)
    adv = atk(vid, torch.zeros(2, dtype=torch.long), ["a", "b"]).cpu()
    spec = graphs.build_tiny(VIT, (64, 64))
    check_trajectory(atk, None, VitReference(spec, weights.synthetic_state_dict(spec, 0), [spec.hook_for(2)], dtype=torch.float64), vid, rtol=TRAJECTORY_RTOL)
    mean = torch.tensor(restate.MEAN).view(1, 3, 1, 1, 1)
    std = torch.tensor(restate.STD).view(1, 3, 1, 1, 1)
    a, o = adv * std + mean, vid * std + mean
    assert float((a - o).abs().max()) <= 16 / 255 + 1e-6
    assert float(a.min()) >= -1e-6 and float(a.max()) <= 1 + 1e-6
    # two identical calls: bit-identical output
    atk2 = attacks.ImageGuidedFMDirection_Adam([VIT], depth=2, step_size=0.005, steps=10, graph_builder=graphs.build_tiny, weight_seed=0)
    assert torch.equal(atk2(vid, torch.zeros(2, dtype=torch.long), ["a", "b"]).cpu(), adv)


def test_aens_tiny_vit_with_tiny_resnet_matches_the_oracle():
    vid = _video(1, 4, 64, 24)
    depths = {VIT: [1, 2], "resnet": [2, 3]}
    atk = attacks.AENS_I2V_MF([VIT, "resnet"], depths=depths, step_size=0.005, steps=4, momentum=0.5, graph_builder=graphs.build_tiny,
                              weight_seed=0)
    adv, _, costs = atk(vid, torch.zeros(1, dtype=torch.long), ["a"])
    vs, rs = graphs.build_tiny(VIT, (64, 64)), graphs.build_tiny("resnet", (64, 64))
    nets = [VitReference(vs, weights.synthetic_state_dict(vs, 0), [vs.hook_for(d) for d in depths[VIT]], dtype=torch.float64),
            restate.OracleNet(rs, weights.synthetic_state_dict(rs, 0), [rs.hook_for(d, True) for d in depths["resnet"]], dtype=torch.float64)]
    ref = restate.run_attack(nets, vid, steps=4, step_size=0.005, mode="aens", coeffs=torch.ones(4, dtype=torch.float64), momentum=0.5)
    np.testing.assert_allclose(costs, ref["costs"], rtol=2e-4)
    w = np.stack(atk.weights)
    np.testing.assert_allclose(w, np.stack(ref["weights"]), rtol=1e-4, atol=1e-6)
    assert np.abs(w[-1] - 0.25).max() > 1e-4                         # the coefficients moved off uniform


def test_image_main_with_the_vit(tmp_path, monkeypatch):
    import image_main
    cdir = tmp_path / "clips"
    os.makedirs(cdir)
    rs = np.random.RandomState(25)
    for label in (3, 7):
        np.save(cdir / f"{label}-raw.npy", rs.randint(0, 256, size=(2, 224, 224, 3), dtype=np.uint8))
    monkeypatch.setattr(image_main, "OPT_PATH", str(tmp_path))
    image_main.main(["--attack_method", "ImageGuidedFMDirection_Adam", "--step", "2", "--depth", "2", "--direction_image_model", VIT,
                     "--frames", "2", "--hw", "224", "--batch_size", "2", "--synthetic_weights", "--file_prefix", "vit",
                     "--clip_dir", str(cdir)])
    out = tmp_path / "Image-ImageGuidedFMDirection_Adam-2-vit"
    for label in (3, 7):
        a = np.load(out / f"{label}-adv.npy")
        assert a.shape == (3, 2, 224, 224) and np.isfinite(a).all()
    infos = sorted(out.glob("loss_info_*.json"))
    assert len(infos) == 1 and len(json.load(open(infos[0]))) == 2
