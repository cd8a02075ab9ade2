"""CPU: timm's ConvNeXt family as image surrogates on the transformer stack -- for every served name the spec, the
key / shape contract against tests/golden/timm_convnext_keys.json, planes, widths and hook sizes; the refusals; checkpoint loading; the
native packing (filters transposed to (49, C), downsamples as Linears behind the 2 x 2 gather, gamma folded into fc2) checked by running
the packed arrays through the planner's launch sequence written in float64 torch; the test-size twin; the token-major depthwise
launch on the host simulation, which runs it as scalar code with the kernel's arithmetic order (csrc/i2v_convnext_host.h); and the
planner itself (csrc/i2v_convnext.cpp) on the host simulation, with the shared transformer launches as scalar code (csrc/i2v_xf_host.h):
the twin against float64, a 4-step I2V attack and AENS / ENS ensembles against the oracle.

The bound is relative L2 against float64: the larger of 1e-5 and 4 x the error of the float32 CPU run of the same reference on the same
inputs, read from tests/golden/convnext_fp32_cpu_errors.json (tests/make_convnext_fixtures.py) -- DESIGN.md sections 14 to 18."""
import ctypes as C
import json
import os

import pytest
import torch
import torch.nn.functional as F

from i2v_amd import attacks, graphs, weights
from i2v_amd import lib as _lib
from tests import convnext_reference as cr
from tests import make_convnext_fixtures as mk
from tests import swin_reference as sr
from tests.convnext_reference import ConvNextReference
from tests.family_harness import bound, check_trajectory, rand as _rand, rel as _rel, run_twin as _run_twin
from tests.hostsim_util import hostsim_engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = json.load(open(os.path.join(ROOT, "tests", "golden", "timm_convnext_keys.json")))
FP32 = json.load(open(os.path.join(ROOT, "tests", "golden", "convnext_fp32_cpu_errors.json")))
TABLE = {"convnext_tiny": (96, (3, 3, 9, 3)), "convnext_small": (96, (3, 3, 27, 3)), "convnext_base": (128, (3, 3, 27, 3)),
         "convnext_large": (192, (3, 3, 27, 3))}
NAMES = sorted(TABLE)
TINY = "convnext_tiny"
FLOOR = 1e-5


@pytest.mark.parametrize("name", NAMES)
def test_param_shapes_equal_the_key_fixture(name):
    want = {k: tuple(v) for k, v in KEYS["names"][name].items()}
    shapes = graphs.build(name).param_shapes()
    assert shapes == want and list(shapes) == list(want)


@pytest.mark.parametrize("name", NAMES)
def test_spec_planes_widths_and_hooks_of_every_name(name):
    dim, depths = TABLE[name]
    spec = graphs.build(name)
    assert isinstance(spec, graphs.ConvNextSpec) and spec.arch == name and spec.video is False and spec.in_hw == (224, 224)
    assert (spec.img, spec.patch, spec.in_chans, spec.dim, spec.depths, spec.ln_eps) == (224, 4, 3, dim, depths, 1e-6)
    assert [spec.grid(i) for i in range(4)] == [56, 28, 14, 7]
    assert [spec.width(i) for i in range(4)] == [dim, 2 * dim, 4 * dim, 8 * dim]
    assert {d: spec.hook_for(d) for d in (1, 2, 3, 4)} == {1: 0, 2: 1, 3: 2, 4: 3}
    assert [spec.hook_dim(spec.hook_for(d)) for d in (1, 2, 3, 4)] == [dim * 56 ** 2, 2 * dim * 28 ** 2, 4 * dim * 14 ** 2, 8 * dim * 7 ** 2]
    with pytest.raises(KeyError):
        spec.hook_for(5)
    assert graphs.convnext_named(name) == spec and graphs.is_convnext_name(name)
    assert not graphs.is_swin_name(name) and not graphs.is_vit_name(name)
    shapes = spec.param_shapes()
    assert shapes["stem.0.weight"] == (dim, 3, 4, 4) and shapes["stages.1.downsample.1.weight"] == (2 * dim, dim, 2, 2)
    assert shapes["stages.3.blocks.2.conv_dw.weight"] == (8 * dim, 1, 7, 7) and shapes["stages.2.blocks.0.mlp.fc1.weight"] == (16 * dim, 4 * dim)
    assert "stages.0.downsample.1.weight" not in shapes and not any(k.startswith(("head.", "norm_pre.")) for k in shapes)
    if name == TINY:
        assert spec.macs_per_frame() == pytest.approx(4.46e9, rel=0.01)            # the 4.5 GMACs convnext_tiny is known by


def test_refusals_name_the_reason_and_list_the_served_names():
    for name, why in (("convnext_tiny_in22k", "in22k"), ("convnext_base_384_in22ft1k", "384"), ("convnext_large_in22ft1k", "in22ft1k"),
                      ("convnext_tiny_384_in22ft1k", "384"), ("convnext_xlarge_in22k", "in22k"), ("convnext_xlarge", "not a model"),
                      ("convnext_nano", "not a model"), ("convnext_atto", "not a model"), ("convnextv2_tiny", "global response"),
                      ("convnextv2_base", "GRN")):
        with pytest.raises(ValueError, match=why) as ei:
            graphs.build(name)
        assert all(n in str(ei.value) for n in TABLE)
        with pytest.raises(ValueError):
            graphs.build_tiny(name)
    for name in NAMES:
        for hw in ((384, 384), (112, 112), (224, 192)):
            with pytest.raises(ValueError, match="224 x 224"):
                graphs.build(name, hw)


def test_existing_names_behave_as_before():
    assert not graphs.is_convnext_name("convolution") and not graphs.is_convnext_name("resnext50_32x4d")
    assert isinstance(graphs.build("swin_tiny_patch4_window7_224"), graphs.SwinSpec) and graphs.build("resnet").arch == "resnet101"
    assert not set(graphs.CONVNEXT_MODELS) & (set(graphs.SWIN_MODELS) | set(graphs.VIT_MODELS))
    assert graphs.CONVNEXT_MODELS == TABLE


def _checkpoint(spec):
    sd = {k: torch.zeros(1).expand(shp) for k, shp in spec.param_shapes().items()}
    top = spec.width(spec.stages - 1)
    sd.update({"head.norm.weight": torch.ones(top), "head.norm.bias": torch.zeros(top), "head.fc.weight": torch.zeros(1).expand(1000, top),
               "head.fc.bias": torch.zeros(1000)})
    return sd


@pytest.mark.parametrize("name", NAMES)
def test_checkpoint_with_extra_keys_loads_from_its_own_file(name, tmp_path, monkeypatch):
    spec = graphs.build(name)
    monkeypatch.delenv("I2V_SYNTHETIC_WEIGHTS", raising=False)
    monkeypatch.setenv("I2V_WEIGHTS_DIR", str(tmp_path))
    with pytest.raises(weights.MissingWeights, match=name):
        weights.load_state_dict(spec)
    sd = _checkpoint(spec)
    sd["stages.0.blocks.0.gamma"] = torch.full((spec.dim,), 0.25)
    torch.save(sd, tmp_path / f"{name}.pth")
    got = weights.load_state_dict(spec)
    assert list(got) == list(spec.param_shapes()) and not any(k.startswith("head.") for k in got)
    assert all(tuple(got[k].shape) == shp and got[k].is_contiguous() for k, shp in spec.param_shapes().items())
    assert float(got["stages.0.blocks.0.gamma"].mean()) == 0.25


def test_misshaped_and_missing_keys_are_refused_by_key(tmp_path, monkeypatch):
    spec = graphs.build(TINY)
    monkeypatch.setenv("I2V_WEIGHTS_DIR", str(tmp_path))
    sd = _checkpoint(spec)
    path = tmp_path / f"{TINY}.pth"
    torch.save(dict(sd, **{"stages.1.blocks.2.conv_dw.weight": torch.zeros(192, 1, 3, 3)}), path)
    with pytest.raises(ValueError, match=r"stages\.1\.blocks\.2\.conv_dw\.weight"):
        weights.load_state_dict(spec)
    short = dict(sd)
    del short["stages.2.blocks.8.gamma"]
    torch.save(short, path)
    with pytest.raises(KeyError, match=r"stages\.2\.blocks\.8\.gamma"):
        weights.load_state_dict(spec)


def test_synthetic_weights_under_the_opt_in_only(monkeypatch, tmp_path):
    monkeypatch.setenv("I2V_WEIGHTS_DIR", str(tmp_path))
    monkeypatch.delenv("I2V_SYNTHETIC_WEIGHTS", raising=False)
    spec = graphs.build(TINY)
    with pytest.raises(weights.MissingWeights):
        weights.load_state_dict(spec)
    sd = weights.load_state_dict(spec, seed=3)
    assert {k: tuple(v.shape) for k, v in sd.items()} == spec.param_shapes()
    g = sd["stages.2.blocks.4.gamma"].abs()
    assert 0.1 <= float(g.min()) and float(g.max()) <= 0.5 and float(sd["stages.2.blocks.4.gamma"].min()) < 0      # far from ones


def test_test_size_twin():
    t = graphs.build_tiny(TINY, (64, 64))
    assert t == graphs.build_tiny("convnext_large", (64, 64))
    assert t.arch == "convnext_test" and t.arch not in graphs.CONVNEXT_MODELS
    assert (t.patch, t.dim, t.depths) == (4, 8, (2, 1, 2, 1))
    assert [t.grid(i) for i in range(4)] == [16, 8, 4, 2] and [t.width(i) for i in range(4)] == [8, 16, 32, 64]
    assert t.hooks == {1: 0, 2: 1, 3: 2, 4: 3}
    with pytest.raises(ValueError):
        graphs.build_tiny(TINY, (48, 48))
    ref = ConvNextReference(t, weights.synthetic_state_dict(t, 0), [0, 1, 2, 3])
    f = ref.forward(torch.randn(2, 3, 64, 64))
    assert [tuple(a.shape) for a in f] == [(2, 256 * 8), (2, 64 * 16), (2, 16 * 32), (2, 4 * 64)]
    assert ref.backward([torch.ones_like(a) for a in f]).shape == (2, 3, 64, 64)


# ---- the native packing, run through the planner's launch sequence in float64 torch ----------------------------------------------
def _ln(x, w, b, eps):
    return F.layer_norm(x, (x.shape[-1],), w, b, eps)


def packed_forward(spec, arrays, x, n_stages):
    """What csrc/i2v_convnext.cpp launches, on the arrays of `ConvNextSpec.native_arrays`, token-major: the features of stages 0 .. n - 1."""
    a = [t.double() for t in arrays]
    N, P = x.shape[0], spec.patch
    g = spec.grid(0)
    rows = x.reshape(N, spec.in_chans, g, P, g, P).permute(0, 2, 4, 1, 3, 5).reshape(N, g * g, -1)            # patch rows
    t = _ln(rows @ a[0].reshape(spec.dim, -1).T + a[1], a[2], a[3], spec.ln_eps)
    wi, outs = 4, []
    for i in range(n_stages):
        g, D = spec.grid(i), spec.width(i)
        if i > 0:
            t = _ln(t, a[wi], a[wi + 1], spec.ln_eps)
            t = sr.patch_merge_gather(t, 2 * g, 2 * g) @ a[wi + 2].T + a[wi + 3]
            wi += 4
        for _ in range(spec.depths[i]):
            u = cr.dwconv_token_major(t.reshape(N, g, g, D), a[wi], a[wi + 1]).reshape(N, g * g, D)
            h = F.gelu(_ln(u, a[wi + 2], a[wi + 3], spec.ln_eps) @ a[wi + 4].T + a[wi + 5])
            t = t + (h @ a[wi + 6].T + a[wi + 7])
            wi += 8
        outs.append(t.reshape(N, -1))
    assert wi == len(a)
    return outs


def test_native_packing_transposes_permutes_and_folds_gamma():
    spec = graphs.build_tiny(TINY, (64, 64))
    sd = weights.synthetic_state_dict(spec, 0)
    x = _rand(2, 3, 64, 64, seed=21)
    arrays = spec.native_arrays(sd, 4)
    assert len(arrays) == 4 + 3 * 4 + 6 * 8 and all(t.dtype == torch.float32 and t.is_contiguous() for t in arrays)
    assert tuple(arrays[4].shape) == (49, 8) and tuple(arrays[4 + 2 * 8 + 2].shape) == (16, 32)
    got = packed_forward(spec, arrays, x, 4)
    want = ConvNextReference(spec, sd, [0, 1, 2, 3]).forward(x)
    ones = ConvNextReference(spec, sd, [0, 1, 2, 3], unit_gamma=True).forward(x)
    for gf, wf, of, fp in zip(got, want, ones, FP32["convnext_test"]["hooks"]):
        assert _rel(gf, wf) < bound(fp, FLOOR)                    # (the arrays are float32 roundings of the float64 weights: ~1e-7)
        assert _rel(of, wf) > 1000 * bound(fp, FLOOR)             # gamma = 1 misses the true features by far more than the bound
    assert len(spec.native_arrays(sd, 2)) == 4 + 4 + 3 * 8


def test_downsample_as_gather_and_linear_equals_the_strided_convolution():
    N, H, W, Cc = 2, 6, 4, 5
    x, w, b = _rand(N, H, W, Cc, seed=1), _rand(2 * Cc, Cc, 2, 2, seed=2), _rand(2 * Cc, seed=3)
    want = F.conv2d(x.permute(0, 3, 1, 2), w, b, stride=2).permute(0, 2, 3, 1).reshape(N, -1, 2 * Cc)
    L = graphs.ConvNextSpec.downsample_linear(w)
    assert tuple(L.shape) == (2 * Cc, 4 * Cc)
    for q in range(4):                                     # the stated permutation: L[o][q C + c] = w[o][c][q & 1][q >> 1]
        assert torch.equal(L[:, q * Cc:(q + 1) * Cc], w[:, :, q & 1, q >> 1])
    got = sr.patch_merge_gather(x.reshape(N, H * W, Cc), H, W) @ L.T + b
    assert float((got - want).abs().max()) < 1e-12
    wrong = w.reshape(2 * Cc, -1)                          # the weight flattened as it lies is NOT the Linear
    assert float((sr.patch_merge_gather(x.reshape(N, H * W, Cc), H, W) @ wrong.T + b - want).abs().max()) > 0.1


# ---- the depthwise launch on the host simulation ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def eng():
    e = hostsim_engine()
    _lib.bind(e.capi, _lib._CONVNEXT_PROTOS)
    return e


def _node(eng, Cc, H, W, N):
    x, w, b, dy = _rand(N, H, W, Cc, seed=1), _rand(49, Cc, seed=2) / 7, _rand(Cc, seed=3), _rand(N, H, W, Cc, seed=4)
    xf, wf, bf, dyf = (t.float().contiguous() for t in (x, w, b, dy))
    y = eng.convnext_dw(xf, wf, bf)
    res = _rand(N, H, W, Cc, seed=5).float()
    gx = eng.convnext_dw(dyf, wf.flip(0).contiguous(), None, res)          # the input gradient: mirrored filter, + the residual path
    return (x, w, b, dy, res), y, gx


@pytest.mark.parametrize("Cc,H,W", mk.NODE_CASES)
@pytest.mark.parametrize("N", [1, 3])
def test_depthwise_launch_on_the_host_simulation_against_float64(eng, Cc, H, W, N):
    (x, w, b, dy, res), y, gx = _node(eng, Cc, H, W, N)
    xr = x.clone().requires_grad_(True)
    ref = cr.dwconv_token_major(xr, w, b)
    want_gx = torch.autograd.grad(ref, xr, dy)[0] + res.double()
    fp = FP32["nodes"][f"{Cc}x{H}x{W}x{N}"]
    e_f, e_b = _rel(y, ref.detach()), _rel(gx, want_gx)
    print(f"dw {Cc} x {H} x {W}, {N} frames: forward {e_f:.3e} (fp32 CPU {fp['fwd']:.3e}) input gradient {e_b:.3e} (fp32 CPU {fp['bwd']:.3e})")
    assert e_f < bound(fp["fwd"], FLOOR) and e_b < bound(fp["bwd"], FLOOR)
    _, y2, gx2 = _node(eng, Cc, H, W, N)
    assert torch.equal(y, y2) and torch.equal(gx, gx2)                    # reruns: the same bits


def test_frame_0_of_a_3_frame_launch_has_the_bits_of_a_1_frame_launch(eng):
    for Cc, H, W in mk.NODE_CASES:
        x, w, b = _rand(3, H, W, Cc, seed=6).float(), (_rand(49, Cc, seed=7) / 7).float(), _rand(Cc, seed=8).float()
        y3, y1 = eng.convnext_dw(x, w, b), eng.convnext_dw(x[:1].contiguous(), w, b)
        assert torch.equal(y3[:1], y1)


def test_the_fma_chain_is_the_stated_one(eng):
    """One output computed by hand in the stated order -- acc = fma(w, x, acc) from 0 over the taps row-major, zero operands outside the
    plane, then + bias -- with float64 standing in for the fused multiply-add: the product of two float32 is exact in float64, and the
    double rounding of the sum is harmless for these magnitudes in all but rare ties, so the hand chain is allowed one ulp."""
    Cc, H, W = 4, 5, 9
    x, w, b = _rand(1, H, W, Cc, seed=9).float(), (_rand(49, Cc, seed=10) / 7).float(), _rand(Cc, seed=11).float()
    y = eng.convnext_dw(x, w, b)
    for (h, q, c) in ((0, 0, 0), (2, 4, 1), (4, 8, 3)):
        acc = torch.zeros((), dtype=torch.float32)
        for a in range(7):
            for t in range(7):
                hs, ws = h + a - 3, q + t - 3
                xv = x[0, hs, ws, c] if 0 <= hs < H and 0 <= ws < W else torch.zeros(())
                acc = (w[a * 7 + t, c].double() * xv.double() + acc.double()).float()
        want = acc + b[c]
        assert abs(float(y[0, h, q, c]) - float(want)) <= float(torch.finfo(torch.float32).eps * abs(want))


def test_the_launch_refuses_bad_arguments(eng):
    z = torch.zeros(8)
    p = lambda t: C.c_void_p(t.data_ptr())      # noqa: E731
    assert eng.capi.i2v_convnext_dw_f32(p(z), p(z), None, None, p(z), 0, 1, 1, 1, None) != 0
    assert b"i2v_convnext_dw_f32" in eng.capi.i2v_last_error()
    assert eng.capi.i2v_convnext_dw_f32(None, p(z), None, None, p(z), 1, 1, 1, 1, None) != 0


# ---- the attack classes, the CLI, the symbols ------------------------------------------------------------------------------------
def test_attack_classes_and_the_cli_take_the_names(tmp_path, monkeypatch):
    for name in NAMES:
        atk = attacks.ImageGuidedFMDirection_Adam([name], depth=4, step_size=0.005, steps=2, weight_seed=0)
        assert atk.model_names == [name]
    attacks.ImageGuidedStd_Adam(["convnext_base"], depth=1, step_size=0.005, weight_seed=0)
    swin = "swin_tiny_patch4_window7_224"
    attacks.ImageGuidedFML2_Adam_MultiModels(["resnet", swin, TINY], depths={"resnet": 2, swin: 3, TINY: 1}, weight_seed=0)
    attacks.AENS_I2V_MF([TINY, "vgg", "vit_small_patch32_224"], depths={TINY: [2, 4], "vgg": [2, 3], "vit_small_patch32_224": [1]},
                        step_size=0.005, weight_seed=0)
    # the test-size ensemble of the twin with resnet_tiny and the tiny Swin plans its names and depths
    attacks.AENS_I2V_MF([TINY, "resnet", swin], depths={TINY: [1, 4], "resnet": [2, 3], swin: [2]}, step_size=0.005,
                        graph_builder=graphs.build_tiny, weight_seed=0)
    with pytest.raises(KeyError):
        attacks.ImageGuidedFMDirection_Adam([TINY], depth=5, step_size=0.005, weight_seed=0)
    with pytest.raises(ValueError, match="in22k"):
        attacks.ImageGuidedFMDirection_Adam(["convnext_tiny_in22k"], depth=2, step_size=0.005, weight_seed=0)
    import image_main
    monkeypatch.setattr(image_main, "OPT_PATH", str(tmp_path))
    base = ["--attack_method", "ImageGuidedFMDirection_Adam", "--step", "2"]
    a = image_main.arg_parse(base + ["--direction_image_model", "convnext_large", "--depth", "4"])
    assert image_main.build_attack(a).model_names == ["convnext_large"]
    for bad in (["--direction_image_model", "convnext_base_384_in22ft1k"], ["--direction_image_model", TINY, "--depth", "5"],
                ["--direction_image_model", TINY, "--hw", "112"], ["--direction_image_model", "convnextv2_tiny"]):
        with pytest.raises(SystemExit):
            image_main.arg_parse(base + bad)


def test_planned_bytes_are_counted_in_64_bits():
    big = graphs.build("convnext_large")
    assert 2 ** 34 < big.workspace_bytes([0, 1, 2, 3], 128) < 2 ** 37
    t = graphs.build(TINY)
    for i in range(4):                          # one more frame costs, per block of stage i, 5 T D + 2 T floats
        per = lambda hooks: t.workspace_bytes(hooks, 3) - t.workspace_bytes(hooks, 2)       # noqa: E731
        T, D = t.tokens(i), t.width(i)
        assert t.depths[i] * (20 * T * D + 8 * T) < per([i]) - (per([i - 1]) if i else 0)


def test_new_native_symbols_are_exported_by_the_library_and_the_host_simulation():
    import __graft_entry__ as ge
    cd = C.CDLL(ge.LIB)
    assert all(hasattr(cd, n) for n in _lib.CONVNEXT_EXPORTS)
    assert not set(_lib.CONVNEXT_EXPORTS) & (set(_lib.EXPORTS) | set(_lib.VIT_EXPORTS) | set(_lib.SWIN_EXPORTS) | set(_lib.LOADER_EXPORTS))
    assert "i2v_convnext.hip" in ge.UNITS and "i2v_convnext.cpp" in ge.UNITS and "-DI2V_HAVE_CONVNEXT" in ge.FLAGS
    hs = C.CDLL(os.path.join(ROOT, "tests", "hostsim", "libi2v_hostsim.so"))
    assert all(hasattr(hs, n) for n in _lib.CONVNEXT_EXPORTS) and not hasattr(hs, "i2v_swin_create") and not hasattr(hs, "i2v_vit_create")
    assert "I2V_HAVE_CONVNEXT" not in open(os.path.join(ROOT, "tests", "hostsim", "build.sh")).read()


# ---- the planner (csrc/i2v_convnext.cpp) on the host simulation: the shared launches as scalar code (csrc/i2v_xf_host.h) ----------
def test_tiny_twin_on_the_host_simulation_against_float64(eng):
    """Features at all four depths and the input gradient with all four hook gradients flowing, 3 frames; reruns bit-identical; frame 0
    of the 3-frame run with the bits of a 1-frame run; a net planned for more frames than it runs gives the same bits."""
    spec = graphs.build_tiny(TINY, (64, 64))
    sd = weights.synthetic_state_dict(spec, 0)
    x = _rand(3, 3, 64, 64, seed=21)                                   # the inputs of tests/make_convnext_fixtures.py
    stages = [0, 1, 2, 3]
    ref = ConvNextReference(spec, sd, stages)
    rf = ref.forward(x)
    hg = [_rand(*f.shape, seed=30 + i) for i, f in enumerate(rf)]
    want_gx = ref.backward(hg)
    feats, gx = _run_twin(eng, spec, sd, stages, x, hg)
    fp = FP32["convnext_test"]
    errs, gerr = [_rel(a, b) for a, b in zip(feats, rf)], _rel(gx, want_gx)
    print(f"convnext_test on the host simulation vs float64: hooks {errs} grad {gerr}; fp32 CPU: {fp['hooks']} {fp['grad']}")
    for e, cpu in zip(errs, fp["hooks"]):
        assert e < bound(cpu, FLOOR)
    assert gerr < bound(fp["grad"], FLOOR)
    feats2, gx2 = _run_twin(eng, spec, sd, stages, x, hg, max_frames=5)
    assert all(torch.equal(a, b) for a, b in zip(feats, feats2)) and torch.equal(gx, gx2)
    f1, g1 = _run_twin(eng, spec, sd, stages, x[:1], [h[:1] for h in hg])
    assert all(torch.equal(a[:1], b) for a, b in zip(feats, f1)) and torch.equal(gx[:1], g1)
    # hooks in another order, and a net truncated below the last stage: the hook of stage 1 alone carries its own gradient only
    fa, ga = _run_twin(eng, spec, sd, [1], x, [hg[1]])
    assert torch.equal(fa[0], feats[1])
    ref1 = ConvNextReference(spec, sd, [1])
    ref1.forward(x)
    assert _rel(ga, ref1.backward([hg[1]])) < bound(fp["grad"], FLOOR)


def test_planner_refusals_on_the_host_simulation(eng):
    spec = graphs.build_tiny(TINY, (64, 64))
    sd = weights.synthetic_state_dict(spec, 0)
    with pytest.raises(_lib.I2VError, match="hooked twice"):
        eng.build_convnext_net(spec, sd, [1, 1], 2)
    with pytest.raises(_lib.I2VError, match="outside"):
        eng.build_convnext_net(spec, sd, [4], 2)
    net = eng.build_convnext_net(spec, sd, [0], 2)
    with pytest.raises(_lib.I2VError, match="planned for"):
        net.forward(torch.zeros(3, 3, 64, 64))
    net.close()


def test_i2v_trajectory_on_the_tiny_twin_matches_the_reference(eng):
    """4 steps of the I2V attack at depth 3 against `restate.run_attack` on the float32 reference net (costs at rtol 2e-4, as
    tests/test_seresnet_cpu.py)."""
    import numpy as np
    from oracle import restate
    torch.manual_seed(5)
    vid = torch.randn(1, 3, 2, 64, 64)
    atk = attacks.ImageGuidedFMDirection_Adam([TINY], depth=3, step_size=0.005, steps=4, engine=eng, graph_builder=graphs.build_tiny,
                                              weight_seed=0)
    adv = atk(vid, torch.zeros(1, dtype=torch.long), ["t"])
    g = graphs.build_tiny(TINY, (64, 64))
    check_trajectory(atk, adv, ConvNextReference(g, weights.synthetic_state_dict(g, 0), [g.hook_for(3)], dtype=torch.float32), vid, rtol=2e-4, steps=4)


def test_aens_and_ens_of_the_twin_with_tiny_resnet_plan_and_run(eng):
    """The ensembles on the host simulation: the twin with `resnet_tiny`, against the oracle.  (The tiny Swin joins them on the device,
    tests/test_gpu_convnext.py: window attention has no host form.)"""
    import numpy as np
    from oracle import restate
    torch.manual_seed(6)
    vid = torch.randn(1, 3, 2, 64, 64)
    depths = {TINY: [1, 4], "resnet": [2, 3]}
    atk = attacks.AENS_I2V_MF([TINY, "resnet"], depths=depths, step_size=0.005, steps=3, momentum=0.5, engine=eng,
                              graph_builder=graphs.build_tiny, weight_seed=0)
    _, _, costs = atk(vid, torch.zeros(1, dtype=torch.long), ["a"])
    cs, rs = graphs.build_tiny(TINY, (64, 64)), graphs.build_tiny("resnet", (64, 64))
    nets = [ConvNextReference(cs, weights.synthetic_state_dict(cs, 0), [cs.hook_for(d) for d in depths[TINY]], dtype=torch.float32),
            restate.OracleNet(rs, weights.synthetic_state_dict(rs, 0), [rs.hook_for(d, True) for d in depths["resnet"]], dtype=torch.float32)]
    ref = restate.run_attack(nets, vid, steps=3, step_size=0.005, mode="aens", coeffs=torch.ones(4), momentum=0.5)
    np.testing.assert_allclose(costs, ref["costs"], rtol=2e-4)
    ens = attacks.ImageGuidedFML2_Adam_MultiModels(["resnet", TINY], depths={"resnet": 2, TINY: 2}, steps=3, engine=eng,
                                                   graph_builder=graphs.build_tiny, weight_seed=0)
    ens(vid, torch.zeros(1, dtype=torch.long), ["a"])
    nets = [restate.OracleNet(rs, weights.synthetic_state_dict(rs, 0), [rs.hook_for(2)], dtype=torch.float32),
            ConvNextReference(cs, weights.synthetic_state_dict(cs, 0), [cs.hook_for(2)], dtype=torch.float32)]
    ref = restate.run_attack(nets, vid, steps=3, step_size=0.005)
    np.testing.assert_allclose(ens.last_costs, ref["costs"], rtol=2e-4)
