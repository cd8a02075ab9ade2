"""CPU: timm's CaiT family as image surrogates on the transformer stack -- for every served name the spec and the
key / shape contract against tests/golden/timm_cait_keys.json; the refusals; checkpoint loading; the native packing (gamma_1 folded into
attn.proj, gamma_2 into mlp.fc2); the talking-heads attention launch on the host simulation, which runs it as scalar code
(csrc/i2v_cait_host.h); and the planner itself (csrc/i2v_cait.cpp) on the host simulation: the twin against float64, a 4-step I2V attack
and an AENS ensemble against the oracle, and a sensitivity check that the cases can see the operator.

The bound is relative L2 against float64: the larger of the floor for that kind of case (attention entries 1e-6 forward, 1e-5 backward;
nets 1e-5) and 4 x the error of the float32 CPU run of the same reference on the same inputs, read from
tests/golden/cait_fp32_cpu_errors.json (tests/make_cait_fixtures.py).  A case without a recorded error fails (KeyError)."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from i2v_amd import attacks, graphs, weights
from i2v_amd import lib as _lib
from oracle import restate
from tests import make_cait_fixtures as mk
from tests.cait_reference import CaitReference
from tests.family_harness import bound, check_trajectory, rand as _rand, rel as _rel, run_twin as _run_twin
from tests.hostsim_util import hostsim_engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = json.load(open(os.path.join(ROOT, "tests", "golden", "timm_cait_keys.json")))
FP32 = json.load(open(os.path.join(ROOT, "tests", "golden", "cait_fp32_cpu_errors.json")))
TABLE = {"cait_xxs24_224": (192, 24, 4), "cait_xxs36_224": (192, 36, 4), "cait_s24_224": (384, 24, 8)}
NAMES = sorted(TABLE)
S24, XXS = "cait_s24_224", "cait_xxs24_224"
NET_FLOOR, FWD_FLOOR, BWD_FLOOR = 1e-5, 1e-6, 1e-5


# ---- the specs ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_param_shapes_equal_the_key_fixture(name):
    want = {k: tuple(v) for k, v in KEYS["names"][name].items()}
    shapes = graphs.build(name).param_shapes()
    assert shapes == want and list(shapes) == list(want)


@pytest.mark.parametrize("name", NAMES)
def test_spec_tokens_widths_and_hooks_of_every_name(name):
    dim, blocks, heads = TABLE[name]
    spec = graphs.build(name)
    assert isinstance(spec, graphs.CaitSpec) and spec.arch == name and spec.video is False and spec.in_hw == (224, 224)
    assert (spec.img, spec.patch, spec.in_chans, spec.dim, spec.heads, spec.blocks, spec.ln_eps) == (224, 16, 3, dim, heads, blocks, 1e-6)
    assert spec.tokens == 196 and spec.mlp == 4 * dim and dim // heads == 48
    hooks = {d: spec.hook_for(d) for d in (1, 2, 3, 4)}
    assert hooks == {d: d * blocks // 4 - 1 for d in (1, 2, 3, 4)}
    assert list(hooks.values()) == ([5, 11, 17, 23] if blocks == 24 else [8, 17, 26, 35])
    assert all(spec.hook_dim(b) == 196 * dim for b in hooks.values())
    with pytest.raises(KeyError):
        spec.hook_for(5)
    assert graphs.cait_named(name) == spec and graphs.is_cait_name(name)
    assert not graphs.is_swin_name(name) and not graphs.is_vit_name(name) and not graphs.is_convnext_name(name) and not graphs.is_mixer_name(name)
    shapes = spec.param_shapes()
    assert shapes["pos_embed"] == (1, 196, dim) and shapes["blocks.0.attn.proj_l.weight"] == (heads, heads)
    assert not any(k == "cls_token" or k.startswith(("head.", "norm.", "blocks_token_only.")) for k in shapes)
    for hw in ((384, 384), (112, 112), (224, 192)):
        with pytest.raises(ValueError, match="224 x 224"):
            graphs.build(name, hw)


def test_refusals_name_the_reason_and_list_the_served_names():
    for name in ("cait_xxs24_384", "cait_xxs36_384", "cait_xs24_384", "cait_s24_384", "cait_s36_384", "cait_m36_384", "cait_m48_448"):
        with pytest.raises(ValueError, match="384 x 384 and 448 x 448") as ei:
            graphs.build(name)
        assert all(n in str(ei.value) for n in TABLE)
        with pytest.raises(ValueError):
            graphs.build_tiny(name)
    for name in ("cait_s36_224", "cait_xs24_224", "cait_m36_224", "cait", "cait_tiny"):
        with pytest.raises(ValueError, match="not a model of this table") as ei:
            graphs.build(name)
        assert all(n in str(ei.value) for n in TABLE)


def test_existing_names_behave_as_before():
    with pytest.raises(UnboundLocalError):
        graphs.build("transformer")
    with pytest.raises(UnboundLocalError):
        graphs.build("pit_s_224")
    with pytest.raises(ValueError, match="not served"):
        graphs.build("mobilenet_v2")
    with pytest.raises(ValueError, match="not served"):
        graphs.build("efficientnet_b0")
    with pytest.raises(AttributeError):
        graphs.build("densenet")
    assert not graphs.is_cait_name("vit_base_patch16_224") and not graphs.is_cait_name("mixer_b16_224") and not graphs.is_cait_name("resnet")
    assert isinstance(graphs.build("mixer_b16_224"), graphs.MixerSpec) and isinstance(graphs.build("vit_base_patch16_224"), graphs.VitSpec)
    assert isinstance(graphs.build("convnext_tiny"), graphs.ConvNextSpec) and graphs.build("resnet").arch == "resnet101"
    assert not set(graphs.CAIT_MODELS) & (set(graphs.SWIN_MODELS) | set(graphs.VIT_MODELS) | set(graphs.CONVNEXT_MODELS) | set(graphs.MIXER_MODELS))
    assert graphs.CAIT_MODELS == TABLE


# ---- checkpoints -------------------------------------------------------------------------------------------------------------------
def _checkpoint(spec):
    """A timm-shaped checkpoint with the keys behind every hook as well: cls_token, the two class-attention blocks, norm and head."""
    D = spec.dim
    sd = {k: torch.zeros(1).expand(shp) for k, shp in spec.param_shapes().items()}
    sd.update({"cls_token": torch.zeros(1, 1, D), "norm.weight": torch.ones(D), "norm.bias": torch.zeros(D),
               "head.weight": torch.zeros(1).expand(1000, D), "head.bias": torch.zeros(1000)})
    for i in (0, 1):
        p = f"blocks_token_only.{i}."
        sd.update({p + "gamma_1": torch.zeros(D), p + "gamma_2": torch.zeros(D), p + "attn.q.weight": torch.zeros(1).expand(D, D),
                   p + "attn.k.weight": torch.zeros(1).expand(D, D), p + "attn.v.weight": torch.zeros(1).expand(D, D),
                   p + "mlp.fc1.weight": torch.zeros(1).expand(4 * D, D)})
    return sd


@pytest.mark.parametrize("name", NAMES)
def test_checkpoint_with_the_keys_behind_the_hooks_loads_from_its_own_file(name, tmp_path, monkeypatch):
    spec = graphs.build(name)
    monkeypatch.delenv("I2V_SYNTHETIC_WEIGHTS", raising=False)
    monkeypatch.setenv("I2V_WEIGHTS_DIR", str(tmp_path))
    with pytest.raises(weights.MissingWeights, match=name):
        weights.load_state_dict(spec)
    sd = _checkpoint(spec)
    sd["patch_embed.proj.bias"] = torch.full((spec.dim,), 0.25)
    torch.save(sd, tmp_path / f"{name}.pth")
    got = weights.load_state_dict(spec)
    assert list(got) == list(spec.param_shapes())
    assert not any(k == "cls_token" or k.startswith(("head.", "norm.", "blocks_token_only.")) for k in got)
    assert all(tuple(got[k].shape) == shp and got[k].is_contiguous() for k, shp in spec.param_shapes().items())
    assert float(got["patch_embed.proj.bias"].mean()) == 0.25


def test_misshaped_and_missing_keys_are_refused_by_key(tmp_path, monkeypatch):
    monkeypatch.setenv("I2V_WEIGHTS_DIR", str(tmp_path))
    for name, bad, shape, gone in ((S24, "blocks.3.attn.proj_l.weight", (4, 4), "blocks.23.attn.proj_w.bias"),
                                   (XXS, "blocks.2.gamma_1", (1, 1, 192), "blocks.7.gamma_2")):
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


def test_synthetic_weights_let_the_new_arithmetic_show(monkeypatch, tmp_path):
    monkeypatch.setenv("I2V_WEIGHTS_DIR", str(tmp_path))
    monkeypatch.delenv("I2V_SYNTHETIC_WEIGHTS", raising=False)
    spec = graphs.build(XXS)
    with pytest.raises(weights.MissingWeights):
        weights.load_state_dict(spec)
    sd = weights.load_state_dict(spec, seed=3)
    assert {k: tuple(v.shape) for k, v in sd.items()} == spec.param_shapes()
    for k in ("blocks.4.gamma_1", "blocks.19.gamma_2"):        # of order 1, far from timm's 1e-5
        assert 0.5 <= float(sd[k].abs().min()) and float(sd[k].abs().max()) <= 1.0 and float(sd[k].min()) < 0 < float(sd[k].max())
    for k in ("blocks.4.attn.proj_l.weight", "blocks.19.attn.proj_w.weight"):
        assert float((sd[k] - torch.eye(4)).abs().mean()) > 0.1 and float(sd[k].diagonal().mean()) > 0.5
    assert float(sd["blocks.4.attn.proj_l.bias"].abs().mean()) > 0.05 and float(sd["blocks.4.attn.proj_w.bias"].abs().max()) > 0
    assert float(sd["pos_embed"].std()) > 0.3


def test_test_size_twin():
    t = graphs.build_tiny(S24, (64, 64))
    assert t == graphs.build_tiny(XXS, (64, 64)) == graphs.build_tiny("cait_xxs36_224", (64, 64)) == graphs.cait_tiny_twin()
    assert t.arch == "cait_test" and t.arch not in graphs.CAIT_MODELS
    assert (t.patch, t.dim, t.heads, t.blocks, t.tokens, t.mlp) == (16, 32, 4, 8, 16, 128) and t.hooks == {1: 1, 2: 3, 3: 5, 4: 7}
    assert graphs.build_tiny(S24, (80, 80)).tokens == 25
    with pytest.raises(ValueError):
        graphs.build_tiny(S24, (72, 72))
    ref = CaitReference(t, weights.synthetic_state_dict(t, 0), [1, 7])
    f = ref.forward(torch.randn(2, 3, 64, 64))
    assert [tuple(a.shape) for a in f] == [(2, 16 * 32)] * 2
    assert ref.backward([torch.ones_like(a) for a in f]).shape == (2, 3, 64, 64)


def test_native_packing_folds_the_layer_scales():
    spec = graphs.build_tiny(S24, (64, 64))
    sd = weights.synthetic_state_dict(spec, 0)
    a = spec.native_arrays(sd, 3)
    assert len(a) == 3 + 16 * 3 and all(t.dtype == torch.float32 and t.is_contiguous() for t in a)
    assert tuple(a[2].shape) == (16, 32) and tuple(a[3 + 4].shape) == (4, 4) and tuple(a[3 + 6].shape) == (4, 4)
    b = 3 + 16 * 2
    g1, g2 = sd["blocks.2.gamma_1"].double(), sd["blocks.2.gamma_2"].double()
    assert torch.equal(a[b + 8], (sd["blocks.2.attn.proj.weight"].double() * g1[:, None]).float())
    assert torch.equal(a[b + 9], (sd["blocks.2.attn.proj.bias"].double() * g1).float())
    assert torch.equal(a[b + 14], (sd["blocks.2.mlp.fc2.weight"].double() * g2[:, None]).float())
    assert torch.equal(a[b + 15], (sd["blocks.2.mlp.fc2.bias"].double() * g2).float())
    assert torch.equal(a[b + 4], sd["blocks.2.attn.proj_l.weight"]) and torch.equal(a[b + 7], sd["blocks.2.attn.proj_w.bias"])


# ---- the attention launch on the host simulation -----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def eng():
    e = hostsim_engine()
    _lib.bind(e.capi, _lib._CAIT_PROTOS)
    return e


def run_attn(eng, d, device="cpu"):
    """(out, probs (F, H, T, T), dqkv) of an attention case through the two C entries."""
    c = {k: (v.float().to(device).contiguous() if torch.is_tensor(v) else v) for k, v in d.items()}
    out, probs = eng.cait_attention(c["qkv"], c["heads"], c["scale"], c["wl"], c["bl"], c["ww"], c["bw"])
    dqkv = eng.cait_attention_bwd(c["qkv"], probs, c["dout"], c["heads"], c["scale"], c["wl"], c["ww"], c["bw"])
    return out, probs[..., :c["qkv"].shape[1]], dqkv


@pytest.mark.parametrize("F,T,H,dh", mk.ATTN_CASES)
def test_attention_host_twin_against_float64(eng, F, T, H, dh):
    d = mk.attn_case(F, T, H, dh)
    out, probs, dqkv = run_attn(eng, d)
    want, want_p, want_g = mk.attn_reference(d)
    fp = FP32["attention"][mk.case_key(F, T, H, dh)]
    e_f, e_p, e_b = _rel(out, want), _rel(probs, want_p), _rel(dqkv, want_g)
    print(f"attention F {F} T {T} H {H} dh {dh}: out {e_f:.3e} (fp32 CPU {fp['fwd']:.3e}) probs {e_p:.3e} ({fp['probs']:.3e}) "
          f"dqkv {e_b:.3e} ({fp['bwd']:.3e})")
    assert e_f < bound(fp["fwd"], FWD_FLOOR) and e_p < bound(fp["probs"], FWD_FLOOR) and e_b < bound(fp["bwd"], BWD_FLOOR)
    out2, probs2, dqkv2 = run_attn(eng, d)
    assert torch.equal(out, out2) and torch.equal(probs, probs2) and torch.equal(dqkv, dqkv2)      # reruns: the same bits
    if F > 1:                                                             # frame 0 of the F-frame call: the bits of a 1-frame call
        o1, p1, g1 = run_attn(eng, {k: (v[:1] if torch.is_tensor(v) and v.dim() == 3 else v) for k, v in d.items()})
        assert torch.equal(out[:1], o1) and torch.equal(probs[:1], p1) and torch.equal(dqkv[:1], g1)


def test_the_attention_entries_refuse_with_the_reason(eng):
    z = torch.zeros(4096)
    p = lambda t: C.c_void_p(t.data_ptr())      # noqa: E731
    capi = eng.capi
    fwd = lambda *, q=p(z), frames=1, T=4, H=2, dh=8: capi.i2v_cait_attention_f32(q, frames, T, H, dh, 0.5, p(z), p(z), p(z), p(z), p(z), p(z), None)      # noqa: E731
    assert fwd() == 0
    for kw, why in ((dict(q=None), b"null"), (dict(frames=0), b"positive"), (dict(dh=6), b"multiple of 4"), (dict(H=17, dh=4), b"LDS budget"),
                    (dict(T=400, H=8, dh=4), b"LDS budget"), (dict(frames=70000), b"65535"), (dict(frames=40000, T=196, H=8, dh=48), b"2^31")):
        assert fwd(**kw) != 0
        err = capi.i2v_last_error()
        assert b"cait_attention" in err and b"hipErrorInvalidValue" in err and why in err, err
    assert capi.i2v_cait_attention_bwd_f32(p(z), p(z), p(z), 1, 4, 2, 6, 0.5, p(z), p(z), p(z), p(z), p(z), p(z), None) != 0
    assert b"cait_attention_bwd" in capi.i2v_last_error() and b"multiple of 4" in capi.i2v_last_error()
    assert capi.i2v_cait_attention_bwd_f32(p(z), p(z), p(z), 1, 4, 2, 8, 0.5, p(z), p(z), p(z), p(z), None, p(z), None) != 0
    assert b"null" in capi.i2v_last_error()


# ---- the attack classes, the CLI, the symbols --------------------------------------------------------------------------------------
def test_attack_classes_and_the_cli_take_the_names(tmp_path, monkeypatch):
    for name in NAMES:
        atk = attacks.ImageGuidedFMDirection_Adam([name], depth=4, step_size=0.005, steps=2, weight_seed=0)
        assert atk.model_names == [name]
    attacks.ImageGuidedStd_Adam([XXS], depth=1, step_size=0.005, weight_seed=0)
    attacks.ImageGuidedFML2_Adam_MultiModels(["resnet", S24, "vit_base_patch16_224"], depths={"resnet": 2, S24: 3, "vit_base_patch16_224": 1},
                                             weight_seed=0)
    attacks.AENS_I2V_MF([S24, "vgg", "mixer_b16_224"], depths={S24: [2, 4], "vgg": [2, 3], "mixer_b16_224": [1]}, step_size=0.005, weight_seed=0)
    with pytest.raises(KeyError):
        attacks.ImageGuidedFMDirection_Adam([S24], depth=5, step_size=0.005, weight_seed=0)
    with pytest.raises(ValueError, match="384 x 384"):
        attacks.ImageGuidedFMDirection_Adam(["cait_s24_384"], depth=2, step_size=0.005, weight_seed=0)
    import image_main
    monkeypatch.setattr(image_main, "OPT_PATH", str(tmp_path))
    base = ["--attack_method", "ImageGuidedFMDirection_Adam", "--step", "2"]
    for name in (S24, "cait_xxs36_224"):
        a = image_main.arg_parse(base + ["--direction_image_model", name, "--depth", "4"])
        assert image_main.build_attack(a).model_names == [name]
    for bad in (["--direction_image_model", "cait_m48_448"], ["--direction_image_model", S24, "--depth", "5"],
                ["--direction_image_model", XXS, "--hw", "112"], ["--direction_image_model", "cait_s36_224"]):
        with pytest.raises(SystemExit):
            image_main.arg_parse(base + bad)


def test_new_native_symbols_are_exported_by_the_library_and_the_host_simulation():
    import __graft_entry__ as ge
    cd = C.CDLL(ge.LIB)
    assert all(hasattr(cd, n) for n in _lib.CAIT_EXPORTS)
    assert {"i2v_cait_attention_f32", "i2v_cait_attention_bwd_f32", "i2v_cait_add_pos_f32", "i2v_cait_create", "i2v_cait_destroy", "i2v_cait_workspace_bytes",
            "i2v_cait_forward", "i2v_cait_backward", "i2v_cait_hook_info", "i2v_cait_read_hook"} == set(_lib.CAIT_EXPORTS)
    assert not set(_lib.CAIT_EXPORTS) & (set(_lib.EXPORTS) | set(_lib.VIT_EXPORTS) | set(_lib.SWIN_EXPORTS) | set(_lib.LOADER_EXPORTS)
                                         | set(_lib.CONVNEXT_EXPORTS) | set(_lib.MIXER_EXPORTS))
    assert {"i2v_cait.hip", "i2v_cait.cpp"} <= set(ge.UNITS) and "-DI2V_HAVE_CAIT" in ge.FLAGS
    assert {"i2v_cait_host.h", "i2v_cait_kernels.h"} <= set(ge.HEADERS)
    hs = C.CDLL(os.path.join(ROOT, "tests", "hostsim", "libi2v_hostsim.so"))
    assert all(hasattr(hs, n) for n in _lib.CAIT_EXPORTS) and not hasattr(hs, "i2v_swin_create") and not hasattr(hs, "i2v_vit_create")
    assert "I2V_HAVE_CAIT" not in open(os.path.join(ROOT, "tests", "hostsim", "build.sh")).read()
    header = open(os.path.join(ROOT, "include", "i2v_cait.h")).read()
    assert all(n + "(" in header for n in _lib.CAIT_EXPORTS)


def test_planned_bytes_are_counted_in_64_bits_and_grow_as_the_saves_do():
    t = graphs.build(S24)
    assert 2 ** 33 < t.workspace_bytes([23], 128) < 2 ** 36               # past 32 bits
    T, D, H = t.tokens, t.dim, t.heads
    per = lambda blocks: t.workspace_bytes(blocks, 3) - t.workspace_bytes(blocks, 2)       # noqa: E731
    # one more frame costs per further block: x, qkv, y (5 D per token), h (4 D), four statistics, and H x T x 196 probabilities
    assert per([7]) - per([6]) == 4 * (T * (5 * D + 4 * D + 4) + H * T * 196)
    assert H * T * 196 * 128 * 4 == 157_351_936                          # P of one block at 128 frames: about 157 MB


# ---- the planner (csrc/i2v_cait.cpp) on the host simulation ------------------------------------------------------------------------
@pytest.fixture(scope="module")
def twin_refs():
    """The float64 reference of each twin case, computed once: label -> (spec, sd, x, hooks, features, hook gradients, input gradient)."""
    out = {}
    for label, (side, _) in mk.TWINS.items():
        spec = graphs.build_tiny(S24, (side, side))
        sd = weights.synthetic_state_dict(spec, 0)
        x = mk.twin_input(label)
        ref = CaitReference(spec, sd, mk.TWIN_HOOKS)
        rf = ref.forward(x)
        hg = [_rand(*f.shape, seed=30 + i) for i, f in enumerate(rf)]
        out[label] = (spec, sd, x, rf, hg, ref.backward(hg))
    return out


@pytest.mark.parametrize("label", sorted(mk.TWINS))
def test_twin_on_the_host_simulation_against_float64(eng, twin_refs, label):
    """Features at all four depths and the input gradient with all four hook gradients flowing; a net planned for 5 frames gives the same
    bits, frame 0 the bits of a 1-frame run; a single mid-stack hook gives the same features and its own gradient."""
    spec, sd, x, rf, hg, want_gx = twin_refs[label]
    blocks = [spec.hook_for(d) for d in (1, 2, 3, 4)]
    assert blocks == mk.TWIN_HOOKS
    feats, gx = _run_twin(eng, spec, sd, blocks, x, hg)
    fp = FP32[label]
    errs, gerr = [_rel(a, b) for a, b in zip(feats, rf)], _rel(gx, want_gx)
    print(f"{label} on the host simulation vs float64: hooks {errs} grad {gerr}; fp32 CPU: {fp['hooks']} {fp['grad']}")
    for e, cpu in zip(errs, fp["hooks"]):
        assert e < bound(cpu, NET_FLOOR)
    assert gerr < bound(fp["grad"], NET_FLOOR)
    feats2, gx2 = _run_twin(eng, spec, sd, blocks, x, hg, max_frames=5)
    assert all(torch.equal(a, b) for a, b in zip(feats, feats2)) and torch.equal(gx, gx2)
    f1, g1 = _run_twin(eng, spec, sd, blocks, x[:1], [h[:1] for h in hg])
    assert all(torch.equal(a[:1], b) for a, b in zip(feats, f1)) and torch.equal(gx[:1], g1)
    fo, go = _run_twin(eng, spec, sd, blocks[::-1], x, hg[::-1])          # hooks in another order
    assert all(torch.equal(a, b) for a, b in zip(feats, fo[::-1])) and torch.equal(gx, go)
    fa, ga = _run_twin(eng, spec, sd, [blocks[1]], x, [hg[1]])            # one mid-stack hook: the net is truncated there
    assert torch.equal(fa[0], feats[1])
    ref1 = CaitReference(spec, sd, [blocks[1]])
    ref1.forward(x)
    assert _rel(ga, ref1.backward([hg[1]])) < bound(fp["grad"], NET_FLOOR)


def test_the_cases_can_see_the_operator(eng, twin_refs):
    """Sensitivity: with both head mixes replaced by the identity and zero biases, and separately with gamma = 1e-5 (timm's init), the
    twin's hooked features move by more than 100 x the bound -- from the reference's and from the library's."""
    spec, sd, x, rf, hg, _ = twin_refs["cait_test"]
    blocks = mk.TWIN_HOOKS
    feats, _ = _run_twin(eng, spec, sd, blocks, x, hg)
    plain = CaitReference(spec, sd, blocks, identity_mix=True).forward(x)
    flat = CaitReference(spec, sd, blocks, gamma=1e-5).forward(x)
    for got, want, pl, fl, cpu in zip(feats, rf, plain, flat, FP32["cait_test"]["hooks"]):
        b = bound(cpu, NET_FLOOR)
        assert _rel(pl, want) > 100 * b and _rel(fl, want) > 100 * b
        assert _rel(got, pl) > 100 * b and _rel(got, fl) > 100 * b


def test_planner_refusals_on_the_host_simulation(eng):
    spec = graphs.build_tiny(S24, (64, 64))
    sd = weights.synthetic_state_dict(spec, 0)
    with pytest.raises(_lib.I2VError, match="hooked twice"):
        eng.build_cait_net(spec, sd, [1, 1], 2)
    with pytest.raises(_lib.I2VError, match="outside"):
        eng.build_cait_net(spec, sd, [8], 2)
    net = eng.build_cait_net(spec, sd, [0], 2)
    with pytest.raises(_lib.I2VError, match="planned for"):
        net.forward(torch.zeros(3, 3, 64, 64))
    with pytest.raises(_lib.I2VError):
        net.forward(torch.zeros(2, 3, 32, 32))
    net.close()
    # the s24 plan at 128 frames, depth 3, without allocating: the figure of DESIGN.md section 21
    assert graphs.build(S24).workspace_bytes([17], 128) == 10_027_172_480


def test_i2v_trajectory_on_the_twin_matches_the_reference(eng):
    """4 steps of the I2V attack at depth 3 against `restate.run_attack` on the float32 reference net (costs at rtol 2e-4, as
    tests/test_mixer_cpu.py)."""
    torch.manual_seed(5)
    vid = torch.randn(1, 3, 2, 64, 64)
    atk = attacks.ImageGuidedFMDirection_Adam([S24], depth=3, step_size=0.005, steps=4, engine=eng, graph_builder=graphs.build_tiny,
                                              weight_seed=0)
    adv = atk(vid, torch.zeros(1, dtype=torch.long), ["t"])
    g = graphs.build_tiny(S24, (64, 64))
    check_trajectory(atk, adv, CaitReference(g, weights.synthetic_state_dict(g, 0), [g.hook_for(3)], dtype=torch.float32), vid, rtol=2e-4, steps=4)


def test_aens_of_the_twin_with_tiny_resnet_matches_the_oracle(eng):
    torch.manual_seed(6)
    vid = torch.randn(1, 3, 2, 64, 64)
    depths = {S24: [1, 4], "resnet": [2, 3]}
    atk = attacks.AENS_I2V_MF([S24, "resnet"], depths=depths, step_size=0.005, steps=3, momentum=0.5, engine=eng,
                              graph_builder=graphs.build_tiny, weight_seed=0)
    _, _, costs = atk(vid, torch.zeros(1, dtype=torch.long), ["a"])
    cs, rs = (graphs.build_tiny(n, (64, 64)) for n in (S24, "resnet"))
    nets = [CaitReference(cs, weights.synthetic_state_dict(cs, 0), [cs.hook_for(d) for d in depths[S24]], dtype=torch.float32),
            restate.OracleNet(rs, weights.synthetic_state_dict(rs, 0), [rs.hook_for(d, True) for d in depths["resnet"]], dtype=torch.float32)]
    ref = restate.run_attack(nets, vid, steps=3, step_size=0.005, mode="aens", coeffs=torch.ones(4), momentum=0.5)
    np.testing.assert_allclose(costs, ref["costs"], rtol=2e-4)
