"""GPU (-m gpu): timm's Swin Transformer family on the MI355X (include/i2v_swin.h) -- the window attention kernels on
their own against float64 on every stage's shape, patch merging and the embedding with their backwards, the test-size twin and two
full-size models against the float64 restatement (tests/swin_reference.py), the workspace formula, I2V / AENS / ENS trajectories against
`oracle.restate.run_attack`, stale-scratch repeatability, and `image_main.py` end to end."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from i2v_amd import attacks, graphs, weights
from i2v_amd import lib as _lib
from oracle import restate
from tests import swin_reference as sr
from tests.family_harness import check_trajectory, hooks_and_grad, rand as _rand, rel as _rel, run_net as _run, video as _video
from tests.swin_reference import SwinReference
from tests.vit_family_reference import VitFamilyReference

pytestmark = pytest.mark.gpu
TRAJECTORY_RTOL = 2e-4      # of the trajectory's costs against the float64 run
TINY, BASE = "swin_tiny_patch4_window7_224", "swin_base_patch4_window7_224"
HOOK_BOUND, GRAD_BOUND = 2e-4, 1e-3            # relative L2 against float64: the bounds of the full ViT tests (tests/test_gpu_vit_family.py)
# fp32 CPU run of the restatement against its float64 run on this file's full-size inputs (tests/golden/make_swin_fp32_cpu_errors.py)
FP32_CPU = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "swin_fp32_cpu_errors.json")))


@pytest.fixture(scope="module")
def eng():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return attacks.get_engine("cuda:0")


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


# grids 56 / 28 / 14 / 7 with window 7, shift 0 and 3, heads 3 / 4 / 24, head width 32; the test-size twin's 16 / 8 grids with window 4,
# shift 0 and 2, head width 16.  (A 7 x 7 grid is one window: no shift.)
@pytest.mark.parametrize("F,g,ws,shift,H,dh", [(2, 56, 7, 0, 3, 32), (2, 56, 7, 3, 4, 32), (2, 28, 7, 3, 3, 32), (2, 28, 7, 0, 4, 32),
                                               (3, 14, 7, 3, 24, 32), (3, 14, 7, 0, 3, 32), (3, 7, 7, 0, 24, 32), (2, 7, 7, 0, 4, 32),
                                               (3, 16, 4, 0, 1, 16), (3, 16, 4, 2, 1, 16), (3, 8, 4, 2, 2, 16), (3, 8, 4, 0, 2, 16)])
def test_window_attention_forward_and_backward(eng, F, g, ws, shift, H, dh):
    """Bounds: those of `test_attention_on_the_family_shapes` (1e-6 forward, 1e-5 backward, relative L2 against float64).  The
    probabilities are not stored (the backward recomputes them), so the output stands for them."""
    capi, st = eng.capi, eng.stream()
    Cw, T = H * dh, g * g
    qkv = _rand(F, T, 3 * Cw, seed=13, scale=1.5)
    table = _rand((2 * ws - 1) ** 2, H, seed=12, scale=0.7)                     # std >= 0.5: the bias matters
    qd, td = qkv.float().cuda(), table.float().cuda()
    out = torch.full((F, T, Cw), float("nan"), device="cuda")
    _lib.check(capi, capi.i2v_swin_window_attention_f32(_p(qd), F, g, g, ws, shift, H, dh, _p(td), _p(out), st))
    qr = qkv.clone().requires_grad_(True)
    ref = sr.window_attention(qr, g, g, ws, shift, H, table)
    nobias = sr.window_attention(qkv, g, g, ws, shift, H, torch.zeros_like(table))
    assert _rel(nobias, ref.detach()) > 0.05                                     # ... and is seen to matter
    e_f = _rel(out, ref.detach())
    dout = _rand(F, T, Cw, seed=14)
    dqkv = torch.full((F, T, 3 * Cw), float("nan"), device="cuda")
    dod = dout.float().cuda()
    _lib.check(capi, capi.i2v_swin_window_attention_bwd_f32(_p(qd), _p(dod), F, g, g, ws, shift, H, dh, _p(td), _p(dqkv), st))
    e_b = _rel(dqkv, torch.autograd.grad(ref, qr, dout)[0])
    print(f"window attention grid {g} window {ws} shift {shift} heads {H}: forward {e_f:.3e} backward {e_b:.3e}")
    assert e_f < 1e-6
    assert e_b < 1e-5


def test_window_attention_refuses_what_it_does_not_serve(eng):
    capi, st = eng.capi, eng.stream()
    t = torch.zeros(4096, device="cuda")
    for g, ws, shift, dh in ((10, 7, 0, 32), (14, 7, 7, 32), (14, 7, 3, 64), (7, 7, 3, 32), (12, 6, 0, 32)):
        assert capi.i2v_swin_window_attention_f32(_p(t), 1, g, g, ws, shift, 1, dh, _p(t), _p(t), st) != 0
        assert b"unsupported shape" in capi.i2v_last_error()


@pytest.mark.parametrize("accumulate", [0, 1])
def test_patch_merging_gather_and_scatter_are_exact(eng, accumulate):
    capi, st = eng.capi, eng.stream()
    F, H, W, Cw = 3, 14, 14, 96
    x = _rand(F, H * W, Cw, seed=5).float()
    xd = x.cuda()
    out = torch.empty(F, H * W // 4, 4 * Cw, device="cuda")
    _lib.check(capi, capi.i2v_swin_merge_f32(_p(xd), F, H, W, Cw, _p(out), st))
    assert torch.equal(out.cpu(), sr.patch_merge_gather(x, H, W))
    dout, base = _rand(F, H * W // 4, 4 * Cw, seed=6).float(), _rand(F, H * W, Cw, seed=7).float()
    dx = base.cuda()
    dd = dout.cuda()
    _lib.check(capi, capi.i2v_swin_merge_bwd_f32(_p(dd), F, H, W, Cw, _p(dx), accumulate, st))
    xr = x.clone().requires_grad_(True)
    want = torch.autograd.grad(sr.patch_merge_gather(xr, H, W), xr, dout)[0]
    assert torch.equal(dx.cpu(), base + want if accumulate else want)           # a permutation: one addend per element, exact


@pytest.mark.parametrize("accumulate", [0, 1])
def test_embedding_without_prefix_rows_and_its_backward(eng, accumulate):
    capi, st = eng.capi, eng.stream()
    F, g, P, dim, eps = 3, 6, 4, 96, 1e-5
    img, W, b = _rand(F, 3, g * P, g * P, seed=15), _rand(dim, 3, P, P, seed=16, scale=0.2), _rand(dim, seed=17)
    nw, nb = 1 + 0.1 * _rand(dim, seed=18), _rand(dim, seed=19)
    dev = [t.float().cuda().contiguous() for t in (img, W, b, nw, nb)]
    R = F * g * g
    patches, emb, tok = torch.empty(R, 3 * P * P, device="cuda"), torch.empty(R, dim, device="cuda"), torch.empty(F, g * g, dim, device="cuda")
    mean, rstd = torch.empty(R, device="cuda"), torch.empty(R, device="cuda")
    _lib.check(capi, capi.i2v_swin_embed_f32(_p(dev[0]), F, 3, g, P, _p(dev[1]), _p(dev[2]), _p(dev[3]), _p(dev[4]), eps, dim, _p(patches),
                                             _p(emb), _p(mean), _p(rstd), _p(tok), st))
    ir = img.clone().requires_grad_(True)
    rows = torch.nn.functional.conv2d(ir, W, b, stride=P).flatten(2).transpose(1, 2)
    ref = sr.layer_norm(rows, nw, nb, eps)
    assert torch.equal(patches.cpu().reshape(F, g, g, 3, P, P),
                       img.float().reshape(F, 3, g, P, g, P).permute(0, 2, 4, 1, 3, 5))       # the permutation part: exact
    assert _rel(tok, ref.detach()) < 1e-6
    dt, base = _rand(F, g * g, dim, seed=20), _rand(F, 3, g * P, g * P, seed=21)
    gimg, dtd, demb = base.float().cuda(), dt.float().cuda(), torch.empty(R, dim, device="cuda")
    _lib.check(capi, capi.i2v_swin_embed_bwd_f32(_p(dtd), F, 3, g, P, _p(dev[1]), _p(dev[3]), dim, _p(emb), _p(mean), _p(rstd), _p(demb),
                                                 _p(patches), _p(gimg), accumulate, st))
    want = torch.autograd.grad(ref, ir, dt)[0]
    got = gimg.double().cpu() - (base.float().double() if accumulate else 0)
    assert _rel(got, want) < 1e-5


def _hooks_and_grad(eng, spec, sd, stages, x):
    return hooks_and_grad(eng, spec, sd, stages, x)


def test_tiny_twin_hooks_and_input_gradient(eng):
    spec = graphs.build_tiny(TINY, (64, 64))
    assert (spec.arch, spec.grid(0), spec.grid(1), spec.shift(0, 1), spec.shift(1, 1)) == ("swin_test", 16, 8, 2, 2)
    sd = weights.synthetic_state_dict(spec, 0)
    x = _rand(3, 3, 64, 64, seed=21)
    (feats, gx), hg = _hooks_and_grad(eng, spec, sd, [0, 1], x)
    ref = SwinReference(spec, sd, [0, 1])
    rf = ref.forward(x)
    errs, gerr = [_rel(a, b) for a, b in zip(feats, rf)], _rel(gx, ref.backward(hg))
    print(f"swin_test: HIP vs float64: hooks {errs} grad {gerr}; hook std {[float(f.std()) for f in rf]}")
    assert max(errs) < 2e-5                                                      # the bounds of the ViT twins
    assert gerr < 2e-4
    (feats2, gx2), _ = _hooks_and_grad(eng, spec, sd, [0, 1], x)                 # repeatability: a second net, the same bits
    assert all(torch.equal(a, b) for a, b in zip(feats, feats2)) and torch.equal(gx, gx2)


@pytest.fixture(scope="module", params=[TINY, BASE])
def full(eng, request):
    """Hooks at every depth and the input gradient with all four hook gradients flowing, 2 frames, synthetic weights."""
    name = request.param
    spec = graphs.build(name)
    sd = weights.synthetic_state_dict(spec, 0)
    x = _rand(2, 3, 224, 224, seed=22)
    stages = [spec.hook_for(d) for d in (1, 2, 3, 4)]
    (feats, gx), hg = _hooks_and_grad(eng, spec, sd, stages, x)
    ref = SwinReference(spec, sd, stages)
    rf = ref.forward(x)
    errs, gerr = [_rel(a, b) for a, b in zip(feats, rf)], _rel(gx, ref.backward(hg))
    print(f"{name}: HIP vs float64: hooks {errs} grad {gerr}; fp32 CPU vs float64: {FP32_CPU[name]}")
    return name, errs, gerr


def test_full_size_hooks_against_float64(full):
    name, errs, _ = full
    for e, cpu in zip(errs, FP32_CPU[name]["hooks"]):
        assert e < max(HOOK_BOUND, 4 * cpu)


def test_full_size_input_gradient_against_float64(full):
    name, _, gerr = full
    assert gerr < max(GRAD_BOUND, 4 * FP32_CPU[name]["grad"])


@pytest.mark.parametrize("name,stages", [(TINY, [2]), (TINY, [0, 3]), (BASE, [1]), (BASE, [3, 0, 2])])
def test_workspace_formula_equals_the_native_one(eng, name, stages):
    spec = graphs.build(name)
    sd = weights.synthetic_state_dict(spec, 0)
    net = eng.build_swin_net(spec, sd, stages, 3)
    try:
        assert net.workspace_bytes() == spec.workspace_bytes(stages, 3)
    finally:
        net.close()


def test_fewer_frames_on_a_used_handle_give_the_bits_of_a_fresh_one(eng):
    spec = graphs.build_tiny(TINY, (64, 64))
    sd = weights.synthetic_state_dict(spec, 0)
    big, small = _rand(5, 3, 64, 64, seed=41), _rand(2, 3, 64, 64, seed=42)
    hg = [_rand(2, spec.hook_dim(s), seed=43 + s) for s in (0, 1)]
    used = eng.build_swin_net(spec, sd, [0, 1], 5)
    _run(used, spec, [0, 1], big)
    f1, g1, _ = _run(used, spec, [0, 1], small, hg)
    used.close()
    fresh = eng.build_swin_net(spec, sd, [0, 1], 2)
    f2, g2, _ = _run(fresh, spec, [0, 1], small, hg)
    fresh.close()
    assert all(torch.equal(a, b) for a, b in zip(f1, f2)) and torch.equal(g1, g2)


def test_i2v_trajectory_on_the_tiny_twin_matches_the_restatement():
    vid = _video(2, 4, 64, 23)
    atk = attacks.ImageGuidedFMDirection_Adam([TINY], depth=2, step_size=0.005, steps=10, graph_builder=graphs.build_tiny, weight_seed=0)
    adv = atk(vid, torch.zeros(2, dtype=torch.long), ["a", "b"]).cpu()
    spec = graphs.build_tiny(TINY, (64, 64))
    check_trajectory(atk, None, SwinReference(spec, weights.synthetic_state_dict(spec, 0), [spec.hook_for(2)], dtype=torch.float64), vid, rtol=TRAJECTORY_RTOL)
    mean = torch.tensor(restate.MEAN).view(1, 3, 1, 1, 1)
    std = torch.tensor(restate.STD).view(1, 3, 1, 1, 1)
    a, o = adv * std + mean, vid * std + mean
    assert float((a - o).abs().max()) <= 16 / 255 + 1e-6
    assert float(a.min()) >= -1e-6 and float(a.max()) <= 1 + 1e-6


def test_aens_tiny_swin_with_tiny_resnet_matches_the_oracle():
    vid = _video(1, 4, 64, 24)
    depths = {TINY: [1, 2], "resnet": [2, 3]}
    atk = attacks.AENS_I2V_MF([TINY, "resnet"], depths=depths, step_size=0.005, steps=4, momentum=0.5, graph_builder=graphs.build_tiny,
                              weight_seed=0)
    adv, _, costs = atk(vid, torch.zeros(1, dtype=torch.long), ["a"])
    ss, rs = graphs.build_tiny(TINY, (64, 64)), graphs.build_tiny("resnet", (64, 64))
    nets = [SwinReference(ss, weights.synthetic_state_dict(ss, 0), [ss.hook_for(d) for d in depths[TINY]], dtype=torch.float64),
            restate.OracleNet(rs, weights.synthetic_state_dict(rs, 0), [rs.hook_for(d, True) for d in depths["resnet"]], dtype=torch.float64)]
    ref = restate.run_attack(nets, vid, steps=4, step_size=0.005, mode="aens", coeffs=torch.ones(4, dtype=torch.float64), momentum=0.5)
    np.testing.assert_allclose(costs, ref["costs"], rtol=2e-4)
    w = np.stack(atk.weights)
    np.testing.assert_allclose(w, np.stack(ref["weights"]), rtol=1e-4, atol=1e-6)
    assert np.abs(w[-1] - 0.25).max() > 1e-4                         # the coefficients moved off uniform


def test_ens_with_a_cnn_a_vit_and_a_swin_together():
    vid = _video(1, 4, 64, 26)
    names = ["resnet", "vit_base_patch16_224", TINY]
    atk = attacks.ImageGuidedFML2_Adam_MultiModels(names, depths={n: 2 for n in names}, steps=4, graph_builder=graphs.build_tiny, weight_seed=0)
    atk(vid, torch.zeros(1, dtype=torch.long), ["a"])
    gs = [graphs.build_tiny(n, (64, 64)) for n in names]
    sds = [weights.synthetic_state_dict(g, 0) for g in gs]
    nets = [restate.OracleNet(gs[0], sds[0], [gs[0].hook_for(2)], dtype=torch.float64),
            VitFamilyReference(gs[1], sds[1], [gs[1].hook_for(2)], dtype=torch.float64),
            SwinReference(gs[2], sds[2], [gs[2].hook_for(2)], dtype=torch.float64)]
    ref = restate.run_attack(nets, vid, steps=4, step_size=0.005)
    np.testing.assert_allclose(atk.last_costs, ref["costs"], rtol=2e-4)


def test_image_main_with_a_swin_name(tmp_path, monkeypatch):
    import image_main
    cdir = tmp_path / "clips"
    os.makedirs(cdir)
    rs = np.random.RandomState(25)
    for label in (3, 7):
        np.save(cdir / f"{label}-raw.npy", rs.randint(0, 256, size=(2, 224, 224, 3), dtype=np.uint8))
    monkeypatch.setattr(image_main, "OPT_PATH", str(tmp_path))
    image_main.main(["--attack_method", "ImageGuidedFMDirection_Adam", "--step", "2", "--depth", "3", "--direction_image_model", TINY,
                     "--frames", "2", "--hw", "224", "--batch_size", "2", "--synthetic_weights", "--file_prefix", "swin",
                     "--clip_dir", str(cdir)])
    out = tmp_path / "Image-ImageGuidedFMDirection_Adam-2-swin"
    for label in (3, 7):
        a = np.load(out / f"{label}-adv.npy")
        assert a.shape == (3, 2, 224, 224) and np.isfinite(a).all()
    infos = sorted(out.glob("loss_info_*.json"))
    assert len(infos) == 1 and len(json.load(open(infos[0]))) == 2
