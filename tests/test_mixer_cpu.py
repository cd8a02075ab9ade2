"""CPU: timm's all-MLP family, MLP-Mixer and ResMLP, as image surrogates on the transformer stack -- for every
served name the spec and the key / shape contract against tests/golden/timm_mixer_keys.json; the refusals; checkpoint loading; the
native packing (ResMLP's norm2 folded into fc1, ls2 into fc2) checked by running the packed arrays through the planner's launch
sequence written in float64 torch; the token-mixing launch on the host simulation, which runs it as scalar code with the kernel's
arithmetic order (csrc/i2v_mixer_host.h); and the planner itself (csrc/i2v_mixer.cpp) on the host simulation: both twins against
float64, a 4-step I2V attack and AENS / ENS ensembles against the oracle.

The bound is relative L2 against float64: the larger of 1e-5 and 4 x the error of the float32 CPU run of the same reference on the same
inputs, read from tests/golden/mixer_fp32_cpu_errors.json (tests/make_mixer_fixtures.py)."""
import ctypes as C
import json
import os

import pytest
import torch
import torch.nn.functional as F

from i2v_amd import attacks, graphs, weights
from i2v_amd import lib as _lib
from tests import make_mixer_fixtures as mk
from tests import mixer_reference as mr
from tests.family_harness import bound, check_trajectory, rand as _rand, rel as _rel, run_twin as _run_twin
from tests.hostsim_util import hostsim_engine
from tests.mixer_reference import MixerReference

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = json.load(open(os.path.join(ROOT, "tests", "golden", "timm_mixer_keys.json")))
FP32 = json.load(open(os.path.join(ROOT, "tests", "golden", "mixer_fp32_cpu_errors.json")))
TABLE = {"mixer_s32_224": ("mixer", 32, 512, 8), "mixer_s16_224": ("mixer", 16, 512, 8), "mixer_b32_224": ("mixer", 32, 768, 12),
         "mixer_b16_224": ("mixer", 16, 768, 12), "mixer_l32_224": ("mixer", 32, 1024, 24), "mixer_l16_224": ("mixer", 16, 1024, 24),
         "resmlp_12_224": ("resmlp", 16, 384, 12), "resmlp_24_224": ("resmlp", 16, 384, 24), "resmlp_36_224": ("resmlp", 16, 384, 36),
         "resmlp_12_distilled_224": ("resmlp", 16, 384, 12), "resmlp_24_distilled_224": ("resmlp", 16, 384, 24),
         "resmlp_36_distilled_224": ("resmlp", 16, 384, 36)}
NAMES = sorted(TABLE)
MIXER, RESMLP = "mixer_b16_224", "resmlp_12_224"
TWINS = {"mixer_test": MIXER, "mixer_test_patch32": "mixer_b32_224", "resmlp_test": RESMLP}
FLOOR = 1e-5
ALL_CASES = mk.HIDDEN_CASES + [(S, 0, Cn) for S, Cn in mk.LINEAR_CASES]


# ---- the specs ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_param_shapes_equal_the_key_fixture(name):
    want = {k: tuple(v) for k, v in KEYS["names"][name].items()}
    shapes = graphs.build(name).param_shapes()
    assert shapes == want and list(shapes) == list(want)


@pytest.mark.parametrize("name", NAMES)
def test_spec_tokens_widths_and_hooks_of_every_name(name):
    kind, patch, dim, blocks = TABLE[name]
    spec = graphs.build(name)
    assert isinstance(spec, graphs.MixerSpec) and spec.arch == name and spec.video is False and spec.in_hw == (224, 224)
    assert (spec.img, spec.patch, spec.in_chans, spec.dim, spec.blocks, spec.kind, spec.ln_eps) == (224, patch, 3, dim, blocks, kind, 1e-6)
    S = (224 // patch) ** 2
    assert spec.tokens == S == {16: 196, 32: 49}[patch] and spec.mlp == 4 * dim
    assert spec.tokens_hidden == (dim // 2 if kind == "mixer" else 0)
    assert {d: spec.hook_for(d) for d in (1, 2, 3, 4)} == {d: d * blocks // 4 - 1 for d in (1, 2, 3, 4)}
    assert all(spec.hook_dim(spec.hook_for(d)) == S * dim for d in (1, 2, 3, 4))
    with pytest.raises(KeyError):
        spec.hook_for(5)
    assert graphs.mixer_named(name) == spec and graphs.is_mixer_name(name)
    assert not graphs.is_swin_name(name) and not graphs.is_vit_name(name) and not graphs.is_convnext_name(name)
    shapes = spec.param_shapes()
    assert shapes["stem.proj.weight"] == (dim, 3, patch, patch) and not any(k.startswith(("head.", "norm.")) for k in shapes)
    if kind == "mixer":
        assert shapes[f"blocks.{blocks - 1}.mlp_tokens.fc1.weight"] == (dim // 2, S) and shapes["blocks.0.mlp_tokens.fc2.weight"] == (S, dim // 2)
    else:
        assert shapes[f"blocks.{blocks - 1}.linear_tokens.weight"] == (S, S) and shapes["blocks.0.norm1.alpha"] == (1, 1, dim)
    if name == MIXER:
        assert spec.macs_per_frame() == pytest.approx(12.6e9, rel=0.01)            # the 12.6 GMACs Mixer-B/16 is published with


def test_refusals_name_the_reason_and_list_the_served_names():
    for name, why in (("mixer_b16_224_in21k", "label sets"), ("mixer_l16_224_in21k", "in21k"), ("mixer_b16_224_miil", "miil"),
                      ("mixer_b16_224_miil_in21k", "label sets"), ("resmlp_12_224_dino", "dino"), ("resmlp_big_24_224_in22ft1k", "in22ft1k"),
                      ("resmlp_big_24_224", "patches"), ("resmlp_big_24_distilled_224", "784 tokens"), ("gmixer_12_224", "gated"),
                      ("gmixer_24_224", "SiLU"), ("gmlp_s16_224", "spatial gating"), ("gmlp_ti16_224", "gated"),
                      ("mixer_s8_224", "not a model"), ("mixer_24_224", "not a model"), ("resmlp_48_224", "not a model")):
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
    with pytest.raises(UnboundLocalError):
        graphs.build("transformer")
    with pytest.raises(ValueError, match="not served"):
        graphs.build("mobilenet_v2")
    with pytest.raises(AttributeError):
        graphs.build("densenet")
    assert not graphs.is_mixer_name("mixer") and not graphs.is_mixer_name("resmlp") and not graphs.is_mixer_name("mnasnet1_0")
    assert isinstance(graphs.build("convnext_tiny"), graphs.ConvNextSpec) and graphs.build("resnet").arch == "resnet101"
    assert not set(graphs.MIXER_MODELS) & (set(graphs.SWIN_MODELS) | set(graphs.VIT_MODELS) | set(graphs.CONVNEXT_MODELS))
    assert graphs.MIXER_MODELS == TABLE


# ---- checkpoints -------------------------------------------------------------------------------------------------------------------
def _checkpoint(spec):
    sd = {k: torch.zeros(1).expand(shp) for k, shp in spec.param_shapes().items()}
    sd.update({"norm.weight": torch.ones(spec.dim), "norm.bias": torch.zeros(spec.dim), "head.weight": torch.zeros(1).expand(1000, spec.dim),
               "head.bias": torch.zeros(1000)})
    if spec.kind == "resmlp":
        sd.update({"norm.alpha": torch.ones(1, 1, spec.dim), "norm.beta": torch.zeros(1, 1, spec.dim)})
    return sd


@pytest.mark.parametrize("name", NAMES)
def test_checkpoint_with_extra_keys_loads_from_its_own_file(name, tmp_path, monkeypatch):
    spec = graphs.build(name)
    monkeypatch.delenv("I2V_SYNTHETIC_WEIGHTS", raising=False)
    monkeypatch.setenv("I2V_WEIGHTS_DIR", str(tmp_path))
    with pytest.raises(weights.MissingWeights, match=name):
        weights.load_state_dict(spec)
    sd = _checkpoint(spec)
    sd["stem.proj.bias"] = torch.full((spec.dim,), 0.25)
    torch.save(sd, tmp_path / f"{name}.pth")
    got = weights.load_state_dict(spec)
    assert list(got) == list(spec.param_shapes()) and not any(k.startswith(("head.", "norm.")) for k in got)
    assert all(tuple(got[k].shape) == shp and got[k].is_contiguous() for k, shp in spec.param_shapes().items())
    assert float(got["stem.proj.bias"].mean()) == 0.25


def test_misshaped_and_missing_keys_are_refused_by_key(tmp_path, monkeypatch):
    monkeypatch.setenv("I2V_WEIGHTS_DIR", str(tmp_path))
    for name, bad, shape, gone in ((MIXER, "blocks.3.mlp_tokens.fc1.weight", (196, 384), "blocks.11.mlp_tokens.fc2.bias"),
                                   (RESMLP, "blocks.2.norm1.alpha", (384,), "blocks.7.ls2")):
        spec = graphs.build(name)
        sd = _checkpoint(spec)
        path = tmp_path / f"{name}.pth"
        torch.save(dict(sd, **{bad: torch.zeros(*shape)}), path)
        with pytest.raises(ValueError, match=bad.replace(".", r"\.")):
            weights.load_state_dict(spec)
        short = dict(sd)
        del short[gone]
        torch.save(short, path)
        with pytest.raises(KeyError, match=gone.replace(".", r"\.")):
            weights.load_state_dict(spec)


def test_synthetic_weights_under_the_opt_in_only(monkeypatch, tmp_path):
    monkeypatch.setenv("I2V_WEIGHTS_DIR", str(tmp_path))
    monkeypatch.delenv("I2V_SYNTHETIC_WEIGHTS", raising=False)
    spec = graphs.build(RESMLP)
    with pytest.raises(weights.MissingWeights):
        weights.load_state_dict(spec)
    sd = weights.load_state_dict(spec, seed=3)
    assert {k: tuple(v.shape) for k, v in sd.items()} == spec.param_shapes()
    for k in ("blocks.4.ls1", "blocks.9.ls2"):                 # far from timm's 1e-4 and from the ones of a forgotten fold
        assert 0.1 <= float(sd[k].abs().min()) and float(sd[k].abs().max()) <= 0.4 and float(sd[k].min()) < 0
    a, b = sd["blocks.4.norm2.alpha"], sd["blocks.4.norm2.beta"]
    assert float((a - 1).abs().mean()) > 0.2 and float(b.abs().mean()) > 0.2


def test_test_size_twins():
    tm, tm32, tr = (graphs.build_tiny(TWINS[a], (64, 64)) for a in ("mixer_test", "mixer_test_patch32", "resmlp_test"))
    assert tm == graphs.build_tiny("mixer_l16_224", (64, 64)) and tr == graphs.build_tiny("resmlp_36_distilled_224", (64, 64))
    assert (tm.arch, tm32.arch, tr.arch) == ("mixer_test", "mixer_test_patch32", "resmlp_test")
    assert not {tm.arch, tm32.arch, tr.arch} & set(graphs.MIXER_MODELS)
    assert (tm.kind, tm.patch, tm.dim, tm.blocks, tm.tokens, tm.tokens_hidden) == ("mixer", 16, 32, 8, 16, 16)
    assert (tm32.kind, tm32.patch, tm32.tokens, tm32.tokens_hidden) == ("mixer", 32, 4, 16)
    assert (tr.kind, tr.patch, tr.dim, tr.blocks, tr.tokens, tr.tokens_hidden) == ("resmlp", 32, 32, 8, 4, 0)
    assert tm.hooks == tr.hooks == {1: 1, 2: 3, 3: 5, 4: 7}
    with pytest.raises(ValueError):
        graphs.build_tiny(MIXER, (48, 48))
    for t in (tm, tr):
        ref = MixerReference(t, weights.synthetic_state_dict(t, 0), [1, 7])
        f = ref.forward(torch.randn(2, 3, 64, 64))
        assert [tuple(a.shape) for a in f] == [(2, t.tokens * 32)] * 2
        assert ref.backward([torch.ones_like(a) for a in f]).shape == (2, 3, 64, 64)


# ---- the native packing, run through the planner's launch sequence in float64 torch ------------------------------------------------
def _ln(x, w, b, eps):
    return F.layer_norm(x, (x.shape[-1],), w, b, eps)


def packed_forward(spec, arrays, x, n_blocks, drop=None):
    """What csrc/i2v_mixer.cpp launches, on the arrays of `MixerSpec.native_arrays`, token-major: the stream after every block.  The
    token launch is written as the kernel states it -- W . tile down the token axis with the bias per ROW -- by einsum."""
    a = [t.double() for t in arrays]
    N, P, g = x.shape[0], spec.patch, spec.img // spec.patch
    rows = x.reshape(N, spec.in_chans, g, P, g, P).permute(0, 2, 4, 1, 3, 5).reshape(N, g * g, -1)            # patch rows
    t = rows @ a[0].reshape(spec.dim, -1).T + a[1]
    wi, outs = 2, []
    tok = lambda W, v, b: torch.einsum("mk,nkc->nmc", W, v) + b[None, :, None]      # noqa: E731
    for _ in range(n_blocks):
        if spec.kind == "mixer":
            n1w, n1b, w1, b1, w2, b2, n2w, n2b, f1w, f1b, f2w, f2b = a[wi:wi + 12]
            wi += 12
            y = t + tok(w2, F.gelu(tok(w1, _ln(t, n1w, n1b, spec.ln_eps), b1)), b2)
            t = y + (F.gelu(_ln(y, n2w, n2b, spec.ln_eps) @ f1w.T + f1b) @ f2w.T + f2b)
        else:
            a1, be1, ls1, W, b, f1w, f1b, f2w, f2b = a[wi:wi + 9]
            wi += 9
            y = t + ls1 * tok(W, a1 * t + be1, b)
            t = y + (F.gelu(y @ f1w.T + f1b) @ f2w.T + f2b)
        outs.append(t.reshape(N, -1))
    assert wi == len(a)
    return outs


@pytest.mark.parametrize("twin", ["mixer_test", "resmlp_test"])
def test_native_packing_runs_the_planner_sequence_to_the_reference(twin):
    spec = graphs.build_tiny(TWINS[twin], (64, 64))
    sd = weights.synthetic_state_dict(spec, 0)
    x = _rand(3, 3, 64, 64, seed=21)
    arrays = spec.native_arrays(sd, 8)
    assert len(arrays) == 2 + 8 * (12 if spec.kind == "mixer" else 9)
    assert all(t.dtype == torch.float32 and t.is_contiguous() for t in arrays)
    got = packed_forward(spec, arrays, x, 8)
    hooks = [1, 3, 5, 7]
    want = MixerReference(spec, sd, hooks).forward(x)
    for b, wf, fp in zip(hooks, want, FP32[twin]["hooks"]):
        assert _rel(got[b], wf) < bound(fp, FLOOR)                    # (the arrays are float32 roundings of the float64 weights: ~1e-7)
    assert len(spec.native_arrays(sd, 2)) == 2 + 2 * (12 if spec.kind == "mixer" else 9)
    if spec.kind == "resmlp":                                  # a dropped fold is far outside the bound
        assert tuple(arrays[2].shape) == (32,) and tuple(arrays[5].shape) == (4, 4) and tuple(arrays[7].shape) == (128, 32)
        ones = MixerReference(spec, sd, hooks, unit_ls=True).forward(x)
        nofold = MixerReference(spec, sd, hooks, no_norm2=True).forward(x)
        for b, wf, of, nf, fp in zip(hooks, want, ones, nofold, FP32[twin]["hooks"]):
            assert _rel(of, wf) > 1000 * bound(fp, FLOOR) and _rel(nf, wf) > 1000 * bound(fp, FLOOR)
            assert _rel(got[b], of) > 1000 * bound(fp, FLOOR) and _rel(got[b], nf) > 1000 * bound(fp, FLOOR)


# ---- the token launch on the host simulation ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def eng():
    e = hostsim_engine()
    _lib.bind(e.capi, _lib._MIXER_PROTOS)
    return e


def _f(t):
    return None if t is None else t.float().contiguous()


def run_case(eng, d, tile=0):
    """(out, dz + add) of a token case through the two C entries."""
    c = {k: _f(v) for k, v in d.items()}
    out = eng.mixer_tokens(c["z"], c["residual"], c["w1"], c["b1"], c["w2"], c["b2"], c["in_scale"], c["in_shift"], c["out_scale"], tile)
    dz = eng.mixer_tokens_bwd(c["z"], c["g"], c["w1"], c["b1"], c["w2"], c["in_scale"], c["in_shift"], c["out_scale"], c["add"], tile)
    return out, dz


@pytest.mark.parametrize("S,Sh,Cn", ALL_CASES)
@pytest.mark.parametrize("N", [1, 3])
def test_token_launch_on_the_host_simulation_against_float64(eng, S, Sh, Cn, N):
    d = mk.token_case(S, Sh, Cn, N)
    out, dz = run_case(eng, d)
    want, want_dz = mk.token_reference(d)
    fp = FP32["tokens"][mk.case_key(S, Sh, Cn, N)]
    e_f, e_b = _rel(out, want), _rel(dz, want_dz)
    print(f"tokens S {S} Sh {Sh} C {Cn}, {N} frames: forward {e_f:.3e} (fp32 CPU {fp['fwd']:.3e}) input gradient {e_b:.3e} (fp32 CPU {fp['bwd']:.3e})")
    assert e_f < bound(fp["fwd"], FLOOR) and e_b < bound(fp["bwd"], FLOOR)
    out2, dz2 = run_case(eng, d)
    assert torch.equal(out, out2) and torch.equal(dz, dz2)                # reruns: the same bits
    if N == 3:                                                            # frame 0 of the 3-frame launch: the bits of a 1-frame launch
        o1, g1 = run_case(eng, {k: (v[:1] if v is not None and v.dim() == 3 else v) for k, v in d.items()})
        assert torch.equal(out[:1], o1) and torch.equal(dz[:1], g1)


def test_the_fma_chain_is_the_stated_one(eng):
    """A few outputs of the hidden-less launch computed by hand in the stated order -- t = fma(in_scale, z, in_shift); acc = fma(w, t, acc)
    from 0 over the tokens in increasing order, an odd count closed by fma(0, 0, acc); + bias of the row; * out_scale; residual + --
    with float64 standing in for the fused multiply-add: the product of two float32 is exact in float64, and the double rounding of the
    sum is harmless for these magnitudes in all but rare ties, so the hand chain is allowed one ulp."""
    S, Cn = 9, 8
    d = {k: _f(v) for k, v in mk.token_case(S, 0, Cn, 2).items()}
    out = eng.mixer_tokens(d["z"], d["residual"], d["w1"], d["b1"], None, None, d["in_scale"], d["in_shift"], d["out_scale"])
    f32 = lambda v: v.float()      # noqa: E731
    for (n, m, c) in ((0, 0, 0), (1, 4, 3), (1, 8, 7)):
        acc = torch.zeros((), dtype=torch.float32)
        for k in range(S):
            t = f32(d["in_scale"][c].double() * d["z"][n, k, c].double() + d["in_shift"][c].double())
            acc = f32(d["w1"][m, k].double() * t.double() + acc.double())
        v = acc + d["b1"][m]
        v = d["out_scale"][c] * v
        want = d["residual"][n, m, c] + v
        assert abs(float(out[n, m, c]) - float(want)) <= float(torch.finfo(torch.float32).eps * abs(want))


def test_the_launch_refuses_bad_arguments(eng):
    z = torch.zeros(64)
    p = lambda t: C.c_void_p(t.data_ptr())      # noqa: E731
    capi = eng.capi
    fwd = lambda *, zz=p(z), frames=1, Cn=4, w=p(z): capi.i2v_mixer_tokens_f32(zz, p(z), p(z), frames, 4, 0, Cn, w, p(z), None, None,      # noqa: E731
                                                                             None, None, None, 0, None)
    assert fwd() == 0
    for kw in (dict(zz=None), dict(w=None), dict(frames=0), dict(frames=-2), dict(Cn=6), dict(Cn=0)):
        assert fwd(**kw) != 0
        assert b"i2v_mixer_tokens_f32" in capi.i2v_last_error()
    bwd = lambda *, g=p(z), frames=1, Cn=4, wt=p(z): capi.i2v_mixer_tokens_bwd_f32(None, g, None, p(z), frames, 4, 0, Cn, None, None, wt,      # noqa: E731
                                                                                None, None, None, None, 0, None)
    assert bwd() == 0
    for kw in (dict(g=None), dict(wt=None), dict(frames=0), dict(Cn=10)):
        assert bwd(**kw) != 0
        assert b"i2v_mixer_tokens_bwd_f32" in capi.i2v_last_error()
    # a hidden layer without its second Linear; a channel tile that is neither 32 nor 64; scale without shift
    assert capi.i2v_mixer_tokens_f32(p(z), p(z), p(z), 1, 4, 2, 4, p(z), p(z), None, None, None, None, None, 0, None) != 0
    assert capi.i2v_mixer_tokens_f32(p(z), p(z), p(z), 1, 4, 0, 4, p(z), p(z), None, None, None, None, None, 48, None) != 0
    assert b"i2v_mixer_tokens_f32" in capi.i2v_last_error()
    assert capi.i2v_mixer_tokens_f32(p(z), p(z), p(z), 1, 4, 0, 4, p(z), p(z), None, None, p(z), None, None, 0, None) != 0
    # (196 + 512) rows of a 64-channel tile do not fit the LDS: refused when insisted on, planned at 32 otherwise
    big = torch.zeros(196 * 512)
    assert capi.i2v_mixer_tokens_f32(p(big), p(big), p(big), 1, 196, 512, 64, p(big), p(big), p(big), p(big), None, None, None, 64, None) != 0
    assert b"LDS" in capi.i2v_last_error()


# ---- the attack classes, the CLI, the symbols --------------------------------------------------------------------------------------
def test_attack_classes_and_the_cli_take_the_names(tmp_path, monkeypatch):
    for name in NAMES:
        atk = attacks.ImageGuidedFMDirection_Adam([name], depth=4, step_size=0.005, steps=2, weight_seed=0)
        assert atk.model_names == [name]
    attacks.ImageGuidedStd_Adam(["mixer_l16_224"], depth=1, step_size=0.005, weight_seed=0)
    attacks.ImageGuidedFML2_Adam_MultiModels(["resnet", MIXER, RESMLP], depths={"resnet": 2, MIXER: 3, RESMLP: 1}, weight_seed=0)
    attacks.AENS_I2V_MF([MIXER, "vgg", RESMLP], depths={MIXER: [2, 4], "vgg": [2, 3], RESMLP: [1]}, step_size=0.005, weight_seed=0)
    attacks.AENS_I2V_MF([MIXER, "resnet", RESMLP], depths={MIXER: [1, 4], "resnet": [2, 3], RESMLP: [2]}, step_size=0.005,
                        graph_builder=graphs.build_tiny, weight_seed=0)
    with pytest.raises(KeyError):
        attacks.ImageGuidedFMDirection_Adam([MIXER], depth=5, step_size=0.005, weight_seed=0)
    with pytest.raises(ValueError, match="in21k"):
        attacks.ImageGuidedFMDirection_Adam(["mixer_b16_224_in21k"], depth=2, step_size=0.005, weight_seed=0)
    with pytest.raises(ValueError, match="gated"):
        attacks.ImageGuidedFMDirection_Adam(["gmlp_s16_224"], depth=2, step_size=0.005, weight_seed=0)
    import image_main
    monkeypatch.setattr(image_main, "OPT_PATH", str(tmp_path))
    base = ["--attack_method", "ImageGuidedFMDirection_Adam", "--step", "2"]
    for name in (MIXER, "resmlp_36_distilled_224"):
        a = image_main.arg_parse(base + ["--direction_image_model", name, "--depth", "4"])
        assert image_main.build_attack(a).model_names == [name]
    for bad in (["--direction_image_model", "mixer_b16_224_miil"], ["--direction_image_model", MIXER, "--depth", "5"],
                ["--direction_image_model", RESMLP, "--hw", "112"], ["--direction_image_model", "resmlp_big_24_224"],
                ["--direction_image_model", "gmixer_24_224"], ["--direction_image_model", "mixer_xl16_224"]):
        with pytest.raises(SystemExit):
            image_main.arg_parse(base + bad)


def test_planned_bytes_are_counted_in_64_bits_and_grow_as_the_saves_do():
    big = graphs.build("mixer_l16_224")
    assert 2 ** 33 < big.workspace_bytes([23], 128) < 2 ** 36            # past 32 bits
    for name in (MIXER, RESMLP):
        t = graphs.build(name)
        S, D = t.tokens, t.dim
        per = lambda blocks: t.workspace_bytes(blocks, 3) - t.workspace_bytes(blocks, 2)       # noqa: E731
        # one more frame costs per further block: Mixer x', y, h and four statistics per token; ResMLP h alone
        want = 4 * (S * (2 * D + 4 * D + 4) if t.kind == "mixer" else S * 4 * D)
        assert per([7]) - per([6]) == want


def test_new_native_symbols_are_exported_by_the_library_and_the_host_simulation():
    import __graft_entry__ as ge
    cd = C.CDLL(ge.LIB)
    assert all(hasattr(cd, n) for n in _lib.MIXER_EXPORTS)
    assert not set(_lib.MIXER_EXPORTS) & (set(_lib.EXPORTS) | set(_lib.VIT_EXPORTS) | set(_lib.SWIN_EXPORTS) | set(_lib.LOADER_EXPORTS)
                                          | set(_lib.CONVNEXT_EXPORTS))
    assert {"i2v_mixer.hip", "i2v_mixer.cpp"} <= set(ge.UNITS) and "-DI2V_HAVE_MIXER" in ge.FLAGS
    assert {"i2v_mixer_host.h", "i2v_gelu.h"} <= set(ge.HEADERS)
    hs = C.CDLL(os.path.join(ROOT, "tests", "hostsim", "libi2v_hostsim.so"))
    assert all(hasattr(hs, n) for n in _lib.MIXER_EXPORTS) and not hasattr(hs, "i2v_swin_create") and not hasattr(hs, "i2v_vit_create")
    assert "I2V_HAVE_MIXER" not in open(os.path.join(ROOT, "tests", "hostsim", "build.sh")).read()
    header = open(os.path.join(ROOT, "include", "i2v_mixer.h")).read()
    assert all(n + "(" in header for n in _lib.MIXER_EXPORTS)


# ---- the planner (csrc/i2v_mixer.cpp) on the host simulation -----------------------------------------------------------------------
@pytest.mark.parametrize("twin", sorted(TWINS))
def test_twins_on_the_host_simulation_against_float64(eng, twin):
    """Features at all four depths and the input gradient with all four hook gradients flowing, 3 frames; a net planned for 5 frames
    gives the same bits, frame 0 the bits of a 1-frame run; a single mid-stack hook gives the same features and its own gradient."""
    spec = graphs.build_tiny(TWINS[twin], (64, 64))
    sd = weights.synthetic_state_dict(spec, 0)
    x = _rand(3, 3, 64, 64, seed=21)                                   # the inputs of tests/make_mixer_fixtures.py
    blocks = [spec.hook_for(d) for d in (1, 2, 3, 4)]
    ref = MixerReference(spec, sd, blocks)
    rf = ref.forward(x)
    hg = [_rand(*f.shape, seed=30 + i) for i, f in enumerate(rf)]
    want_gx = ref.backward(hg)
    feats, gx = _run_twin(eng, spec, sd, blocks, x, hg)
    fp = FP32[twin]
    errs, gerr = [_rel(a, b) for a, b in zip(feats, rf)], _rel(gx, want_gx)
    print(f"{twin} on the host simulation vs float64: hooks {errs} grad {gerr}; fp32 CPU: {fp['hooks']} {fp['grad']}")
    for e, cpu in zip(errs, fp["hooks"]):
        assert e < bound(cpu, FLOOR)
    assert gerr < bound(fp["grad"], FLOOR)
    feats2, gx2 = _run_twin(eng, spec, sd, blocks, x, hg, max_frames=5)
    assert all(torch.equal(a, b) for a, b in zip(feats, feats2)) and torch.equal(gx, gx2)
    f1, g1 = _run_twin(eng, spec, sd, blocks, x[:1], [h[:1] for h in hg])
    assert all(torch.equal(a[:1], b) for a, b in zip(feats, f1)) and torch.equal(gx[:1], g1)
    # hooks in another order
    fo, go = _run_twin(eng, spec, sd, blocks[::-1], x, hg[::-1])
    assert all(torch.equal(a, b) for a, b in zip(feats, fo[::-1])) and torch.equal(gx, go)
    # one mid-stack hook: the net is truncated there and carries that hook's gradient only
    fa, ga = _run_twin(eng, spec, sd, [blocks[1]], x, [hg[1]])
    assert torch.equal(fa[0], feats[1])
    ref1 = MixerReference(spec, sd, [blocks[1]])
    ref1.forward(x)
    assert _rel(ga, ref1.backward([hg[1]])) < bound(fp["grad"], FLOOR)


def test_planner_refusals_on_the_host_simulation(eng):
    for name in (MIXER, RESMLP):
        spec = graphs.build_tiny(name, (64, 64))
        sd = weights.synthetic_state_dict(spec, 0)
        with pytest.raises(_lib.I2VError, match="hooked twice"):
            eng.build_mixer_net(spec, sd, [1, 1], 2)
        with pytest.raises(_lib.I2VError, match="outside"):
            eng.build_mixer_net(spec, sd, [8], 2)
        net = eng.build_mixer_net(spec, sd, [0], 2)
        with pytest.raises(_lib.I2VError, match="planned for"):
            net.forward(torch.zeros(3, 3, 64, 64))
        with pytest.raises(_lib.I2VError):
            net.forward(torch.zeros(2, 3, 32, 32))
        net.close()


def test_i2v_trajectory_on_the_mixer_twin_matches_the_reference(eng):
    """4 steps of the I2V attack at depth 3 against `restate.run_attack` on the float32 reference net (costs at rtol 2e-4, as
    tests/test_convnext_cpu.py)."""
    import numpy as np
    from oracle import restate
    torch.manual_seed(5)
    vid = torch.randn(1, 3, 2, 64, 64)
    atk = attacks.ImageGuidedFMDirection_Adam([MIXER], depth=3, step_size=0.005, steps=4, engine=eng, graph_builder=graphs.build_tiny,
                                              weight_seed=0)
    adv = atk(vid, torch.zeros(1, dtype=torch.long), ["t"])
    g = graphs.build_tiny(MIXER, (64, 64))
    check_trajectory(atk, adv, MixerReference(g, weights.synthetic_state_dict(g, 0), [g.hook_for(3)], dtype=torch.float32), vid, rtol=2e-4, steps=4)


def test_aens_and_ens_of_the_twins_with_tiny_resnet_match_the_oracle(eng):
    """3 steps of AENS over [mixer twin, resnet] and of ENS over [resnet, resmlp twin] on the host simulation, against the oracle."""
    import numpy as np
    from oracle import restate
    torch.manual_seed(6)
    vid = torch.randn(1, 3, 2, 64, 64)
    depths = {MIXER: [1, 4], "resnet": [2, 3]}
    atk = attacks.AENS_I2V_MF([MIXER, "resnet"], depths=depths, step_size=0.005, steps=3, momentum=0.5, engine=eng,
                              graph_builder=graphs.build_tiny, weight_seed=0)
    _, _, costs = atk(vid, torch.zeros(1, dtype=torch.long), ["a"])
    ms, rs, ps = (graphs.build_tiny(n, (64, 64)) for n in (MIXER, "resnet", RESMLP))
    nets = [MixerReference(ms, weights.synthetic_state_dict(ms, 0), [ms.hook_for(d) for d in depths[MIXER]], dtype=torch.float32),
            restate.OracleNet(rs, weights.synthetic_state_dict(rs, 0), [rs.hook_for(d, True) for d in depths["resnet"]], dtype=torch.float32)]
    ref = restate.run_attack(nets, vid, steps=3, step_size=0.005, mode="aens", coeffs=torch.ones(4), momentum=0.5)
    np.testing.assert_allclose(costs, ref["costs"], rtol=2e-4)
    ens = attacks.ImageGuidedFML2_Adam_MultiModels(["resnet", RESMLP], depths={"resnet": 2, RESMLP: 2}, steps=3, engine=eng,
                                                   graph_builder=graphs.build_tiny, weight_seed=0)
    adv = ens(vid, torch.zeros(1, dtype=torch.long), ["a"])
    nets = [restate.OracleNet(rs, weights.synthetic_state_dict(rs, 0), [rs.hook_for(2)], dtype=torch.float32),
            MixerReference(ps, weights.synthetic_state_dict(ps, 0), [ps.hook_for(2)], dtype=torch.float32)]
    ref = restate.run_attack(nets, vid, steps=3, step_size=0.005)
    np.testing.assert_allclose(ens.last_costs, ref["costs"], rtol=2e-4)
    assert float((adv - ref["adv"]).abs().mean()) < 5e-3
