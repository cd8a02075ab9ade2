"""GPU (-m gpu): timm's plain ViT / DeiT family on the MI355X (include/i2v_vit.h) -- the token assembly with one and
two prefix tokens against float64, the attention / linear / LayerNorm kernels on the family's shapes (50 and 198 tokens, 3 and 16 heads,
widths 192 and 1024), the test-size distilled and patch-32 twins and four full-size models against the float64 restatement
(tests/vit_family_reference.py), I2V / AENS trajectories against `oracle.restate.run_attack`, `vit_base_patch16_224` bit for bit through
the old and the new entry, repeatability, and `image_main.py` end to end."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from i2v_amd import attacks, graphs, weights
from i2v_amd import lib as _lib
from oracle import restate
from tests.family_harness import _hip, _set_hook_grads, check_trajectory, hooks_and_grad, rand as _rand, rel as _rel, video as _video
from tests.vit_family_reference import VitFamilyReference, gelu, layer_norm

pytestmark = pytest.mark.gpu
TRAJECTORY_RTOL = 2e-4      # of the trajectory's costs against the float64 run
DISTILLED, PATCH32 = "deit_base_distilled_patch16_224", "vit_base_patch32_224"
HOOK_BOUND, GRAD_BOUND = 2e-4, 1e-3            # relative L2 against float64: the bounds of the full ViT-B/16 test (tests/test_gpu_vit.py)
# vit_large_patch16_224 (24 blocks), 2 frames, synthetic weights: relative L2 error of an fp32 CPU run of the restatement against its
# float64 run, measured on the build host (worst hook of d = 1..4, and the input gradient at depth 4).  The bound for the 24-block model
# is the larger of the 12-block bound and 4 x this figure.
LARGE_FP32_CPU_HOOK, LARGE_FP32_CPU_GRAD = 1.94e-6, 5.67e-6


@pytest.fixture(scope="module")
def eng():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return attacks.get_engine("cuda:0")


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("n_prefix", [1, 2])
def test_prefix_token_assembly_and_its_backward(eng, n_prefix, accumulate):
    capi, st = eng.capi, eng.stream()
    F, g, P, dim = 3, 3, 8, 72                      # 9 patch rows of 8 x 8 pixels, a width that is no multiple of 64
    T = n_prefix + g * g
    img, W, b = _rand(F, 3, g * P, g * P, seed=15), _rand(dim, 3, P, P, seed=16, scale=0.05), _rand(dim, seed=17)
    prefix, pos = _rand(n_prefix, dim, seed=18), _rand(T, dim, seed=19)
    dev = [t.float().cuda().contiguous() for t in (img, W, b, prefix, pos)]
    patches, emb = torch.empty(F * g * g, 3 * P * P, device="cuda"), torch.empty(F * g * g, dim, device="cuda")
    tok = torch.empty(F, T, dim, device="cuda")
    _lib.check(capi, capi.i2v_vit_embed_ex_f32(_p(dev[0]), F, 3, g, P, _p(dev[1]), _p(dev[2]), _p(dev[3]), n_prefix, _p(dev[4]), dim,
                                               _p(patches), _p(emb), _p(tok), st))
    ir = img.clone().requires_grad_(True)
    p = torch.nn.functional.conv2d(ir, W, b, stride=P).flatten(2).transpose(1, 2)
    ref = torch.cat([prefix.view(1, n_prefix, dim).expand(F, n_prefix, dim), p], 1) + pos
    assert _rel(tok, ref.detach()) < 1e-6
    if n_prefix == 1:                               # the old entry is the new one with one prefix row: the same bits
        tok1 = torch.empty_like(tok)
        _lib.check(capi, capi.i2v_vit_embed_f32(_p(dev[0]), F, 3, g, P, _p(dev[1]), _p(dev[2]), _p(dev[3]), _p(dev[4]), dim, _p(patches),
                                                _p(emb), _p(tok1), st))
        assert torch.equal(tok1, tok)
    dt = _rand(F, T, dim, seed=20)
    base = _rand(F, 3, g * P, g * P, seed=21)
    gimg = base.float().cuda()
    dtd = dt.float().cuda()
    _lib.check(capi, capi.i2v_vit_embed_bwd_ex_f32(_p(dtd), F, 3, g, P, _p(dev[1]), dim, n_prefix, _p(patches), _p(gimg), accumulate, st))
    want = torch.autograd.grad(ref, ir, dt)[0]
    got = gimg.double().cpu() - (base.float().double() if accumulate else 0)
    assert _rel(got, want) < 1e-5
    if n_prefix == 1:
        g1 = base.float().cuda()
        _lib.check(capi, capi.i2v_vit_embed_bwd_f32(_p(dtd), F, 3, g, P, _p(dev[1]), dim, _p(patches), _p(g1), accumulate, st))
        assert torch.equal(g1, gimg)


@pytest.mark.parametrize("F,T,H,dh", [(2, 50, 3, 64), (2, 50, 16, 64), (1, 198, 3, 64), (1, 198, 16, 64)])
def test_attention_on_the_family_shapes(eng, F, T, H, dh):
    capi, st = eng.capi, eng.stream()
    Cw, ld = H * dh, capi.i2v_vit_probs_ld(T)
    assert ld % 4 == 0 and T <= ld < T + 4
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


# qkv of the 192-wide models (1.5 and 4.5 tiles of 128), fc1 / fc2 of the 1024-wide ones, and the patch-32 embedding (K = 3 * 32 * 32)
@pytest.mark.parametrize("M,K,N", [(2 * 50, 192, 576), (2 * 198, 192, 768), (198, 1024, 4096), (50, 4096, 1024), (2 * 49, 3072, 384)])
def test_linear_on_the_family_shapes(eng, M, K, N):
    """Bound, relative L2 against float64: fp32 sums of n random-sign terms drift as a random walk, so the error of a dot product of
    length n is of the order 2^-24 sqrt(n) (2^-24: fp32's unit roundoff) -- 3.8e-6 at the 4096-long sums of the 1024-wide models' MLP,
    which the 1e-6 the ViT-B shapes are held to (n <= 3072 forward, 768 backward) does not cover.  The bound is the larger of the two:
    1e-6 up to n = 279, 2^-24 sqrt(n) beyond.  A wrong tile or stride is off by orders of magnitude more."""
    capi, st = eng.capi, eng.stream()
    fwd_tol, bwd_tol = max(1e-6, 2.0 ** -24 * K ** 0.5), max(1e-6, 2.0 ** -24 * N ** 0.5)
    x, W, b, r = _rand(M, K, seed=1), _rand(N, K, seed=2, scale=K ** -0.5), _rand(N, seed=3), _rand(M, N, seed=4)
    d = [t.float().cuda() for t in (x, W, b, r)]
    y, g = torch.empty(M, N, device="cuda"), torch.empty(M, N, device="cuda")
    _lib.check(capi, capi.i2v_vit_linear_f32(_p(d[0]), M, K, _p(d[1]), _p(d[2]), N, _p(d[3]), _p(y), _p(g), st))
    ref = x @ W.T + b + r
    print(f"linear {M}x{K}x{N}: forward {_rel(y, ref):.3e} gelu {_rel(g, gelu(ref)):.3e} (bound {fwd_tol:.3e})")
    assert _rel(y, ref) < fwd_tol and _rel(g, gelu(ref)) < fwd_tol
    dy, pre = _rand(M, N, seed=5), _rand(M, K, seed=6)
    dd, pd = dy.float().cuda(), pre.float().cuda()
    dx = torch.empty(M, K, device="cuda")
    _lib.check(capi, capi.i2v_vit_linear_bwd_f32(_p(dd), M, N, _p(d[1]), K, _p(pd), _p(dx), st))
    pr = pre.clone().requires_grad_(True)
    gprime = torch.autograd.grad(gelu(pr).sum(), pr)[0]
    print(f"linear {M}x{K}x{N}: backward {_rel(dx, (dy @ W) * gprime):.3e} (bound {bwd_tol:.3e})")
    assert _rel(dx, (dy @ W) * gprime) < bwd_tol


@pytest.mark.parametrize("rows,Cw", [(2 * 50, 192), (198, 1024), (2 * 198, 384)])
def test_layernorm_on_the_family_shapes(eng, rows, Cw):
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


def _hooks_and_grad(eng, spec, sd, blocks, x):
    return hooks_and_grad(eng, spec, sd, blocks, x)


@pytest.mark.parametrize("name", [DISTILLED, PATCH32])
def test_tiny_twins_hooks_and_input_gradient(eng, name):
    spec = graphs.build_tiny(name, (64, 64))
    assert spec.tokens == (18 if name == DISTILLED else 5)
    sd = weights.synthetic_state_dict(spec, 0)
    x = _rand(3, 3, 64, 64, seed=21)
    (feats, gx), hg = _hooks_and_grad(eng, spec, sd, [2, 5], x)
    ref = VitFamilyReference(spec, sd, [2, 5])
    rf = ref.forward(x)
    for a, b in zip(feats, rf):
        assert _rel(a, b) < 2e-5
    assert _rel(gx, ref.backward(hg)) < 2e-4
    # repeatability: a second net, the same bits
    (feats2, gx2), _ = _hooks_and_grad(eng, spec, sd, [2, 5], x)
    assert all(torch.equal(a, b) for a, b in zip(feats, feats2)) and torch.equal(gx, gx2)


def _against_float64(eng, name):
    """Hooks at every depth and the input gradient at depth 4 (all four hook gradients flowing), 2 frames, synthetic weights: relative L2
    errors against the float64 restatement."""
    spec = graphs.build(name)
    sd = weights.synthetic_state_dict(spec, 0)
    x = _rand(2, 3, 224, 224, seed=22)
    blocks = [spec.hook_for(d) for d in (1, 2, 3, 4)]
    (feats, gx), hg = _hooks_and_grad(eng, spec, sd, blocks, x)
    ref = VitFamilyReference(spec, sd, blocks)
    rf = ref.forward(x)
    rg = ref.backward(hg)
    errs, gerr = [_rel(a, b) for a, b in zip(feats, rf)], _rel(gx, rg)
    print(f"{name}: HIP vs float64: hooks {errs} grad {gerr}; hook std {[float(f.std()) for f in rf]}")
    return errs, gerr


@pytest.mark.parametrize("name", ["deit_base_distilled_patch16_224", "vit_base_patch32_224", "vit_tiny_patch16_224"])
def test_full_size_12_block_models_against_float64(eng, name):
    """Measured on an MI355X (hooks d = 1..4 worst, input gradient): see DESIGN.md section 13."""
    errs, gerr = _against_float64(eng, name)
    assert max(errs) < HOOK_BOUND
    assert gerr < GRAD_BOUND


@pytest.fixture(scope="module")
def large(eng):
    return _against_float64(eng, "vit_large_patch16_224")           # built and run once for the module


def test_full_size_vit_large_hooks_against_float64(large):
    assert max(large[0]) < max(HOOK_BOUND, 4 * LARGE_FP32_CPU_HOOK)


def test_full_size_vit_large_input_gradient_against_float64(large):
    assert large[1] < max(GRAD_BOUND, 4 * LARGE_FP32_CPU_GRAD)


def test_vit_b16_through_the_new_entry_is_bit_identical_to_the_old_one(eng):
    capi, st = eng.capi, eng.stream()
    spec = graphs.build(graphs.VIT_NAME)
    sd = weights.synthetic_state_dict(spec, 0)
    x = _rand(2, 3, 224, 224, seed=23).float().cuda()
    blocks = [spec.hook_for(d) for d in (2, 4)]
    net = eng.build_vit_net(spec, sd, blocks, 2)                      # i2v_vit_create_ex, n_prefix = 1
    net.forward(x)
    new_feats = [net.save_hook(i, 2) for i in range(2)]
    hg = [_rand(2, spec.tokens * spec.dim, seed=40 + i) for i in range(2)]
    torch.cuda.synchronize()
    _set_hook_grads(net, hg)
    new_gx = torch.empty_like(x)
    net.backward(new_gx)
    torch.cuda.synchronize()
    net.close()
    # the old entry, called as a caller of the one-prefix layout calls it: cls_token as a (dim) array
    keys = ["patch_embed.proj.weight", "patch_embed.proj.bias", "cls_token", "pos_embed"]
    keys += [k for i in range(max(blocks) + 1) for k in spec.block_keys(i)]
    w = [sd[k].detach().float().cpu().contiguous() for k in keys]
    ptrs = (C.c_void_p * len(w))(*[t.data_ptr() for t in w])
    cfg = _lib.VitConfig(spec.img, spec.patch, spec.in_chans, spec.dim, spec.heads, spec.mlp, spec.blocks, spec.ln_eps)
    hb = (C.c_int32 * 2)(*blocks)
    h = C.c_void_p()
    _lib.check(capi, capi.i2v_vit_create(eng.device.index or 0, C.byref(cfg), ptrs, len(w), hb, 2, 2, C.byref(h)))
    try:
        assert capi.i2v_vit_workspace_bytes(h) == spec.workspace_bytes(blocks, 2)
        _lib.check(capi, capi.i2v_vit_forward(h, _p(x), 2, st))
        old_feats = [torch.empty(2, spec.tokens, spec.dim, device="cuda") for _ in range(2)]
        grads = []
        for i in range(2):
            _lib.check(capi, capi.i2v_vit_read_hook(h, i, 0, _p(old_feats[i]), 2, st))
            act, grad = C.c_void_p(), C.c_void_p()
            a_s, g_s, D = C.c_int64(), C.c_int64(), C.c_int64()
            _lib.check(capi, capi.i2v_vit_hook_info(h, i, C.byref(act), C.byref(a_s), C.byref(grad), C.byref(g_s), C.byref(D)))
            assert D.value == spec.tokens * spec.dim
            grads.append(grad.value)
        torch.cuda.synchronize()
        hip = _hip()
        hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        for gp, g in zip(grads, hg):
            gd = g.float().cuda().contiguous()
            torch.cuda.synchronize()
            assert hip.hipMemcpy(gp, gd.data_ptr(), gd.numel() * 4, 3) == 0
        old_gx = torch.empty_like(x)
        _lib.check(capi, capi.i2v_vit_backward(h, _p(old_gx), 0, st))
        torch.cuda.synchronize()
    finally:
        capi.i2v_vit_destroy(h)
    assert all(torch.equal(a, b) for a, b in zip(new_feats, old_feats))
    assert torch.equal(new_gx, old_gx)


def test_create_refuses_a_bad_prefix_count_and_reports_its_error(eng):
    capi = eng.capi
    spec = graphs.build_tiny(DISTILLED, (64, 64))
    sd = weights.synthetic_state_dict(spec, 0)
    w = [torch.zeros(s).float() for s in ((64, 3, 16, 16), (64,), (3, 64), (19, 64))] + [sd[k].float().contiguous() for k in spec.block_keys(0)]
    ptrs = (C.c_void_p * len(w))(*[t.data_ptr() for t in w])
    cfg = _lib.VitConfig(64, 16, 3, 64, 2, 256, 6, 1e-6)
    h = C.c_void_p()
    assert capi.i2v_vit_create_ex(0, C.byref(cfg), 3, ptrs, len(w), (C.c_int32 * 1)(0), 1, 2, C.byref(h)) != 0
    assert b"prefix" in capi.i2v_last_error() and not h.value


def test_create_refuses_more_rows_than_the_kernels_count_before_any_allocation(eng):
    """The kernels count the rows of a stream (frames x tokens) in an int: a plan past 2^31 / 4 rows is refused on the host, as Swin's is."""
    capi = eng.capi
    spec = graphs.build_tiny(DISTILLED, (64, 64))
    sd = weights.synthetic_state_dict(spec, 0)
    w = [torch.zeros(s).float() for s in ((64, 3, 16, 16), (64,), (2, 64), (18, 64))] + [sd[k].float().contiguous() for k in spec.block_keys(0)]
    ptrs = (C.c_void_p * len(w))(*[t.data_ptr() for t in w])
    cfg = _lib.VitConfig(64, 16, 3, 64, 2, 256, 6, 1e-6)
    frames = (0x7fffffff // 4) // spec.tokens + 1
    for n_frames, refused in ((frames, True), (2, False)):
        h = C.c_void_p()
        rc = capi.i2v_vit_create_ex(0, C.byref(cfg), 2, ptrs, len(w), (C.c_int32 * 1)(0), 1, n_frames, C.byref(h))
        if refused:
            assert rc != 0 and b"i2v_vit_create" in capi.i2v_last_error() and b"too many frames" in capi.i2v_last_error() and not h.value
        else:
            assert rc == 0 and h.value
            capi.i2v_vit_destroy(h)


@pytest.mark.parametrize("name", [DISTILLED, PATCH32])
def test_i2v_trajectory_on_the_tiny_twins_matches_the_restatement(name):
    vid = _video(2, 4, 64, 23)
    atk = attacks.ImageGuidedFMDirection_Adam([name], depth=2, step_size=0.005, steps=10, graph_builder=graphs.build_tiny, weight_seed=0)
    adv = atk(vid, torch.zeros(2, dtype=torch.long), ["a", "b"]).cpu()
    spec = graphs.build_tiny(name, (64, 64))
    check_trajectory(atk, None, VitFamilyReference(spec, weights.synthetic_state_dict(spec, 0), [spec.hook_for(2)], dtype=torch.float64), vid, rtol=TRAJECTORY_RTOL)
    mean = torch.tensor(restate.MEAN).view(1, 3, 1, 1, 1)
    std = torch.tensor(restate.STD).view(1, 3, 1, 1, 1)
    a, o = adv * std + mean, vid * std + mean
    assert float((a - o).abs().max()) <= 16 / 255 + 1e-6
    assert float(a.min()) >= -1e-6 and float(a.max()) <= 1 + 1e-6
    atk2 = attacks.ImageGuidedFMDirection_Adam([name], depth=2, step_size=0.005, steps=10, graph_builder=graphs.build_tiny, weight_seed=0)
    assert torch.equal(atk2(vid, torch.zeros(2, dtype=torch.long), ["a", "b"]).cpu(), adv)       # two calls: the same bits


def test_aens_tiny_distilled_vit_with_tiny_resnet_matches_the_oracle():
    vid = _video(1, 4, 64, 24)
    depths = {DISTILLED: [1, 2], "resnet": [2, 3]}
    atk = attacks.AENS_I2V_MF([DISTILLED, "resnet"], depths=depths, step_size=0.005, steps=4, momentum=0.5, graph_builder=graphs.build_tiny,
                              weight_seed=0)
    adv, _, costs = atk(vid, torch.zeros(1, dtype=torch.long), ["a"])
    vs, rs = graphs.build_tiny(DISTILLED, (64, 64)), graphs.build_tiny("resnet", (64, 64))
    nets = [VitFamilyReference(vs, weights.synthetic_state_dict(vs, 0), [vs.hook_for(d) for d in depths[DISTILLED]], dtype=torch.float64),
            restate.OracleNet(rs, weights.synthetic_state_dict(rs, 0), [rs.hook_for(d, True) for d in depths["resnet"]], dtype=torch.float64)]
    ref = restate.run_attack(nets, vid, steps=4, step_size=0.005, mode="aens", coeffs=torch.ones(4, dtype=torch.float64), momentum=0.5)
    np.testing.assert_allclose(costs, ref["costs"], rtol=2e-4)
    w = np.stack(atk.weights)
    np.testing.assert_allclose(w, np.stack(ref["weights"]), rtol=1e-4, atol=1e-6)
    assert np.abs(w[-1] - 0.25).max() > 1e-4                         # the coefficients moved off uniform


def test_image_main_with_a_distilled_deit(tmp_path, monkeypatch):
    import image_main
    name = "deit_small_distilled_patch16_224"
    cdir = tmp_path / "clips"
    os.makedirs(cdir)
    rs = np.random.RandomState(25)
    for label in (3, 7):
        np.save(cdir / f"{label}-raw.npy", rs.randint(0, 256, size=(2, 224, 224, 3), dtype=np.uint8))
    monkeypatch.setattr(image_main, "OPT_PATH", str(tmp_path))
    image_main.main(["--attack_method", "ImageGuidedFMDirection_Adam", "--step", "2", "--depth", "3", "--direction_image_model", name,
                     "--frames", "2", "--hw", "224", "--batch_size", "2", "--synthetic_weights", "--file_prefix", "deit",
                     "--clip_dir", str(cdir)])
    out = tmp_path / "Image-ImageGuidedFMDirection_Adam-2-deit"
    for label in (3, 7):
        a = np.load(out / f"{label}-adv.npy")
        assert a.shape == (3, 2, 224, 224) and np.isfinite(a).all()
    infos = sorted(out.glob("loss_info_*.json"))
    assert len(infos) == 1 and len(json.load(open(infos[0]))) == 2
