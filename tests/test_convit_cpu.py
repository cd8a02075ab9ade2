"""CPU: timm's ConViT family as image surrogates on the transformer stack -- for every served name the spec and the
key / shape contract against tests/golden/timm_convit_keys.json; the refusals; checkpoint loading; the native packing (pos_proj.bias
dropped, the gate folded into one table and one vector, qk and v stacked) against timm's literal arithmetic; the gated positional
attention launch on the host simulation, which runs it as scalar code (csrc/i2v_convit_host.h); and the planner itself
(csrc/i2v_convit.cpp) on the host simulation: the twin against float64 across the join, a 4-step I2V attack and an AENS ensemble against
the oracle, and sensitivity checks that the cases can see the gate, the grid convention and the position of the join.

The bound is relative L2 against float64: the larger of the floor for that kind of case (attention entries 1e-6 forward and on probs,
1e-5 backward; nets 1e-5) and 4 x the error of the float32 CPU run of the same reference on the same inputs, read from
tests/golden/convit_fp32_cpu_errors.json (tests/make_convit_fixtures.py).  A case without a recorded error fails (KeyError)."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from i2v_amd import attacks, graphs, weights
from i2v_amd import lib as _lib
from oracle import restate
from tests import convit_reference as cr
from tests import make_convit_fixtures as mk
from tests.convit_reference import ConvitReference
from tests.family_harness import bound, check_trajectory, rand as _rand, rel as _rel, run_twin as _run_twin
from tests.hostsim_util import hostsim_engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = json.load(open(os.path.join(ROOT, "tests", "golden", "timm_convit_keys.json")))
FP32 = json.load(open(os.path.join(ROOT, "tests", "golden", "convit_fp32_cpu_errors.json")))
TABLE = {"convit_tiny": (192, 4), "convit_small": (432, 9), "convit_base": (768, 16)}
NAMES = sorted(TABLE)
TINY, SMALL = "convit_tiny", "convit_small"
NET_FLOOR, FWD_FLOOR, BWD_FLOOR = 1e-5, 1e-6, 1e-5


# ---- the specs ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_param_shapes_equal_the_key_fixture(name):
    want = {k: tuple(v) for k, v in KEYS["names"][name].items()}
    shapes = graphs.build(name).param_shapes()
    assert shapes == want and list(shapes) == list(want)
    assert KEYS["checked_against"].startswith(("timm ", "unchecked"))


@pytest.mark.parametrize("name", NAMES)
def test_spec_tokens_widths_and_hooks_of_every_name(name):
    dim, heads = TABLE[name]
    spec = graphs.build(name)
    assert isinstance(spec, graphs.ConvitSpec) and spec.arch == name and spec.video is False and spec.in_hw == (224, 224)
    assert (spec.img, spec.patch, spec.in_chans, spec.dim, spec.heads, spec.blocks, spec.local_blocks, spec.ln_eps) == (224, 16, 3, dim, heads, 12, 10, 1e-6)
    assert spec.tokens == 196 and spec.grid == 14 and spec.mlp == 4 * dim and dim // heads == 48
    hooks = [spec.hook_for(d) for d in (1, 2, 3, 4)]
    assert hooks == [2, 5, 8, 11]
    assert [spec.hook_dim(b) for b in hooks] == [196 * dim, 196 * dim, 196 * dim, 197 * dim]
    assert [spec.tokens_at(b) for b in (0, 9, 10, 11)] == [196, 196, 197, 197]
    with pytest.raises(KeyError):
        spec.hook_for(5)
    assert graphs.convit_named(name) == spec and graphs.is_convit_name(name)
    assert not any(f(name) for f in (graphs.is_swin_name, graphs.is_vit_name, graphs.is_convnext_name, graphs.is_mixer_name, graphs.is_cait_name))
    shapes = spec.param_shapes()
    assert shapes["cls_token"] == (1, 1, dim) and shapes["pos_embed"] == (1, 196, dim) and shapes["blocks.0.attn.pos_proj.weight"] == (heads, 3)
    assert shapes["blocks.9.attn.qk.weight"] == (2 * dim, dim) and shapes["blocks.10.attn.qkv.weight"] == (3 * dim, dim)
    assert "blocks.10.attn.qk.weight" not in shapes and "blocks.9.attn.qkv.weight" not in shapes
    assert not any(k.endswith(("qk.bias", "qkv.bias", "attn.v.bias")) or k.startswith(("head.", "norm.")) for k in shapes)
    for hw in ((384, 384), (112, 112), (224, 192)):
        with pytest.raises(ValueError, match="224 x 224") as ei:
            graphs.build(name, hw)
        assert all(n in str(ei.value) for n in TABLE)


def test_refusals_name_the_reason_and_list_the_served_names():
    for name in ("convit", "convit_large", "convit_tiny_384", "convit_small_patch8", "convit_base_in21k"):
        assert graphs.is_convit_name(name)
        with pytest.raises(ValueError, match="not a model of this table") as ei:
            graphs.build(name)
        assert all(n in str(ei.value) for n in TABLE)
        with pytest.raises(ValueError, match="not a model of this table"):
            graphs.build_tiny(name)


def test_existing_names_behave_as_before():
    with pytest.raises(UnboundLocalError):
        graphs.build("transformer")
    with pytest.raises(UnboundLocalError):
        graphs.build("pit_s_224")
    with pytest.raises(ValueError, match="not served"):
        graphs.build("mobilenet_v2")
    with pytest.raises(ValueError, match="not served"):
        graphs.build("efficientnet_b0")
    assert not any(graphs.is_convit_name(n) for n in ("convnext_tiny", "vit_base_patch16_224", "cait_s24_224", "resnet", "conv"))
    assert isinstance(graphs.build("convnext_tiny"), graphs.ConvNextSpec) and isinstance(graphs.build("cait_s24_224"), graphs.CaitSpec)
    assert isinstance(graphs.build("vit_base_patch16_224"), graphs.VitSpec) and graphs.build("resnet").arch == "resnet101"
    others = set(graphs.SWIN_MODELS) | set(graphs.VIT_MODELS) | set(graphs.CONVNEXT_MODELS) | set(graphs.MIXER_MODELS) | set(graphs.CAIT_MODELS)
    assert not set(graphs.CONVIT_MODELS) & others and graphs.CONVIT_MODELS == TABLE


# ---- checkpoints -------------------------------------------------------------------------------------------------------------------
def _checkpoint(spec):
    """A timm-shaped checkpoint with the keys behind every hook as well: norm and head."""
    D = spec.dim
    sd = {k: torch.zeros(1).expand(shp) for k, shp in spec.param_shapes().items()}
    sd.update({"norm.weight": torch.ones(D), "norm.bias": torch.zeros(D), "head.weight": torch.zeros(1).expand(1000, D), "head.bias": torch.zeros(1000)})
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
    assert list(got) == list(spec.param_shapes()) and not any(k.startswith(("head.", "norm.")) for k in got)
    assert all(tuple(got[k].shape) == shp and got[k].is_contiguous() for k, shp in spec.param_shapes().items())
    assert float(got["patch_embed.proj.bias"].mean()) == 0.25


def test_misshaped_and_missing_keys_are_refused_by_key(tmp_path, monkeypatch):
    monkeypatch.setenv("I2V_WEIGHTS_DIR", str(tmp_path))
    for name, bad, shape, gone in ((SMALL, "blocks.3.attn.pos_proj.weight", (3, 9), "blocks.9.attn.gating_param"),
                                   (TINY, "blocks.10.attn.qkv.weight", (384, 192), "cls_token")):
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


def test_synthetic_weights_let_the_new_arithmetic_show():
    spec = graphs.build(SMALL)
    sd = weights.load_state_dict(spec, seed=3)
    assert {k: tuple(v.shape) for k, v in sd.items()} == spec.param_shapes()
    for i in (0, 9):
        w, g = sd[f"blocks.{i}.attn.pos_proj.weight"], sd[f"blocks.{i}.attn.gating_param"]
        assert float((w[:, 0] - w[:, 1]).abs().min()) > 1e-3                  # x and y columns differ in every head
        assert float(w[:, 2].max()) < -0.5 and float(w[:, :2].abs().max()) > 1.5     # timm's local initialisation shows through the noise
        s = torch.sigmoid(g)
        assert float(s.min()) < 0.4 and float(s.max()) > 0.6
        v = sd[f"blocks.{i}.attn.v.weight"]
        assert float((v - torch.eye(spec.dim)).abs().mean()) > 0.01 and float(v.diagonal().abs().mean()) < 0.2
    assert float(sd["cls_token"].std()) > 0.3 and float(sd["blocks.4.attn.pos_proj.bias"].abs().mean()) > 0.05


def test_test_size_twin():
    t = graphs.build_tiny(SMALL, (64, 64))
    assert t == graphs.build_tiny(TINY, (64, 64)) == graphs.build_tiny("convit_base", (64, 64)) == graphs.convit_tiny_twin()
    assert t.arch == "convit_test" and t.arch not in graphs.CONVIT_MODELS
    assert (t.patch, t.dim, t.heads, t.blocks, t.local_blocks, t.tokens, t.mlp) == (16, 32, 4, 8, 6, 16, 128) and t.hooks == {1: 1, 2: 3, 3: 5, 4: 7}
    assert [t.hook_dim(b) for b in (1, 3, 5, 7)] == [16 * 32] * 3 + [17 * 32]
    t80 = graphs.build_tiny(SMALL, (80, 80))
    assert t80.tokens == 25 and t80.tokens_at(7) == 26
    with pytest.raises(ValueError):
        graphs.build_tiny(SMALL, (72, 72))
    ref = ConvitReference(t, weights.synthetic_state_dict(t, 0), [1, 7])
    f = ref.forward(torch.randn(2, 3, 64, 64))
    assert [tuple(a.shape) for a in f] == [(2, 16 * 32), (2, 17 * 32)]
    assert ref.backward([torch.ones_like(a) for a in f]).shape == (2, 3, 64, 64)


# ---- the packer against timm's literal arithmetic ----------------------------------------------------------------------------------
def test_native_packing_against_the_literal_reference():
    spec = graphs.build_tiny(SMALL, (80, 80))
    sd = weights.synthetic_state_dict(spec, 0)
    a = spec.native_arrays(sd, 8)
    T, ld, D, H = 25, 28, 32, 4
    assert len(a) == 4 + 14 * 6 + 12 * 2 and all(t.dtype == torch.float32 and t.is_contiguous() for t in a)
    assert tuple(a[2].shape) == (T, D) and tuple(a[3].shape) == (D,) and len(spec.native_arrays(sd, 3)) == 4 + 14 * 3
    b = 4 + 14 * 2                                                            # block 2
    qkv, bias, c, A = a[b + 2], a[b + 3], a[b + 4], a[b + 5]
    assert tuple(qkv.shape) == (3 * D, D) and tuple(c.shape) == (H,) and tuple(A.shape) == (H, T, ld) and not bias.any()
    assert torch.equal(qkv[:2 * D], sd["blocks.2.attn.qk.weight"]) and torch.equal(qkv[2 * D:], sd["blocks.2.attn.v.weight"])
    assert torch.equal(a[4 + 14 * 6 + 2], sd["blocks.6.attn.qkv.weight"]) and tuple(a[4 + 14 * 6 + 4].shape) == (D, D)      # a plain block: proj follows
    # the table in float64: rows sum to sigma(g); pos_proj.bias changes nothing
    sig = torch.sigmoid(sd["blocks.2.attn.gating_param"].double())
    c64 = 1.0 - sig
    rel = spec.rel_indices()
    assert torch.equal(rel, cr.rel_indices(5))                               # the grid convention is timm's
    pos = torch.einsum("ijk,hk->hij", rel, sd["blocks.2.attn.pos_proj.weight"].double()).softmax(-1)
    assert float(((sig[:, None, None] * pos).sum(-1) - sig[:, None]).abs().max()) < 1e-14
    assert float((A[:, :, :T].double().sum(-1) - sig[:, None]).abs().max()) < 1e-6 and not A[:, :, T:].any() and float(A.min()) >= 0
    assert torch.equal(c, c64.float()) and torch.equal(A[:, :, :T], (sig[:, None, None] * pos).float())
    sd2 = dict(sd, **{"blocks.2.attn.pos_proj.bias": sd["blocks.2.attn.pos_proj.bias"] + 3.0})
    assert all(torch.equal(x, y) for x, y in zip(a, spec.native_arrays(sd2, 8)))
    # the folded definition against timm's literal one (bias, division, separate qk / v), float64
    t = _rand(2, T, D, seed=7)
    qk = torch.nn.functional.linear(t, sd["blocks.2.attn.qk.weight"].double()).reshape(2, T, 2, H, 8).permute(2, 0, 3, 1, 4)
    v = torch.nn.functional.linear(t, sd["blocks.2.attn.v.weight"].double()).reshape(2, T, H, 8).permute(0, 2, 1, 3)
    lit = cr.gpsa_core(qk[0], qk[1], v, 8 ** -0.5, sd["blocks.2.attn.pos_proj.weight"].double(), sd["blocks.2.attn.pos_proj.bias"].double(),
                       sd["blocks.2.attn.gating_param"].double(), cr.rel_indices(5))
    lit2 = cr.gpsa_core(qk[0], qk[1], v, 8 ** -0.5, sd["blocks.2.attn.pos_proj.weight"].double(), sd2["blocks.2.attn.pos_proj.bias"].double(),
                        sd["blocks.2.attn.gating_param"].double(), cr.rel_indices(5))
    fold, _ = cr.blend_attention(torch.nn.functional.linear(t, qkv.double()), H, 8 ** -0.5, c64, sig[:, None, None] * pos)
    assert _rel(fold, lit) < 1e-13 and _rel(lit2, lit) < 1e-13


# ---- the attention launch on the host simulation -----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def eng():
    e = hostsim_engine()
    _lib.bind(e.capi, _lib._CONVIT_PROTOS)
    return e


def _pad(table, device="cpu"):
    """(H, T, T) -> (H, T, ld) float32, rows zero-padded"""
    if table is None:
        return None
    H, T, _ = table.shape
    out = torch.zeros(H, T, (T + 3) // 4 * 4, dtype=torch.float32)
    out[:, :, :T] = table.float()
    return out.to(device).contiguous()


def run_attn(eng, d, device="cpu"):
    """(out, probs (F, H, T, T), dqkv) of an attention case through the two C entries."""
    f = lambda v: v.float().to(device).contiguous()      # noqa: E731
    qkv, c, table = f(d["qkv"]), (None if d["c"] is None else f(d["c"])), _pad(d["table"], device)
    out, probs = eng.convit_attention(qkv, d["heads"], d["scale"], c, table)
    dqkv = eng.convit_attention_bwd(qkv, probs, f(d["dout"]), d["heads"], d["scale"], c, table)
    return out, probs[..., :qkv.shape[1]], dqkv


@pytest.mark.parametrize("F,T,H,dh,gated", mk.ATTN_CASES)
def test_attention_host_twin_against_float64(eng, F, T, H, dh, gated):
    """Gated cases against (c softmax + table) v and its autograd; `table = null` cases against float64 plain attention."""
    d = mk.attn_case(F, T, H, dh, gated)
    out, probs, dqkv = run_attn(eng, d)
    want, want_p, want_g = mk.attn_reference(d)
    fp = FP32["attention"][mk.case_key(F, T, H, dh, gated)]
    e_f, e_p, e_b = _rel(out, want), _rel(probs, want_p), _rel(dqkv, want_g)
    print(f"attention F {F} T {T} H {H} dh {dh} gated {gated}: out {e_f:.3e} (fp32 CPU {fp['fwd']:.3e}) probs {e_p:.3e} ({fp['probs']:.3e}) "
          f"dqkv {e_b:.3e} ({fp['bwd']:.3e})")
    assert e_f < bound(fp["fwd"], FWD_FLOOR) and e_p < bound(fp["probs"], FWD_FLOOR) and e_b < bound(fp["bwd"], BWD_FLOOR)
    out2, probs2, dqkv2 = run_attn(eng, d)
    assert torch.equal(out, out2) and torch.equal(probs, probs2) and torch.equal(dqkv, dqkv2)      # reruns: the same bits
    if F > 1:                                                             # frame 0 of the F-frame call: the bits of a 1-frame call
        o1, p1, g1 = run_attn(eng, dict(d, qkv=d["qkv"][:1], dout=d["dout"][:1]))
        assert torch.equal(out[:1], o1) and torch.equal(probs[:1], p1) and torch.equal(dqkv[:1], g1)


def test_the_attention_entries_refuse_with_the_reason(eng):
    z = torch.zeros(8192)
    p = lambda t: C.c_void_p(t.data_ptr())      # noqa: E731
    capi = eng.capi
    fwd = lambda *, q=p(z), frames=1, T=4, H=2, dh=8, c=p(z), tab=p(z): capi.i2v_convit_attention_f32(q, frames, T, H, dh, 0.5, c, tab, p(z), p(z), None)      # noqa: E731
    assert fwd() == 0 and fwd(c=None, tab=None) == 0
    off = C.c_void_p(z.data_ptr() + 4)
    for kw, why in ((dict(q=None), b"null"), (dict(frames=0), b"positive"), (dict(dh=6), b"multiple of 4"), (dict(c=None), b"go together"),
                    (dict(tab=None), b"go together"), (dict(T=4000, H=1, dh=4), b"LDS budget"), (dict(frames=70000), b"65535"),
                    (dict(frames=40000, T=196, H=8, dh=48), b"2^31"), (dict(q=off), b"alignment"), (dict(tab=off), b"alignment")):
        assert fwd(**kw) != 0
        err = capi.i2v_last_error()
        assert b"convit_attention" in err and b"hipErrorInvalidValue" in err and why in err, err
    bwd = lambda *, dh=8, c=p(z), tab=p(z), ds=p(z): capi.i2v_convit_attention_bwd_f32(p(z), p(z), p(z), 1, 4, 2, dh, 0.5, c, tab, ds, p(z), None)      # noqa: E731
    assert bwd() == 0
    for kw, why in ((dict(dh=6), b"multiple of 4"), (dict(ds=None), b"null"), (dict(c=None), b"go together")):
        assert bwd(**kw) != 0
        assert b"convit_attention_bwd" in capi.i2v_last_error() and why in capi.i2v_last_error()


# ---- the attack classes, the CLI, the symbols --------------------------------------------------------------------------------------
def test_attack_classes_and_the_cli_take_the_names(tmp_path, monkeypatch):
    for name in NAMES:
        atk = attacks.ImageGuidedFMDirection_Adam([name], depth=4, step_size=0.005, steps=2, weight_seed=0)
        assert atk.model_names == [name]
    attacks.ImageGuidedStd_Adam([TINY], depth=1, step_size=0.005, weight_seed=0)
    attacks.ImageGuidedFML2_Adam_MultiModels(["resnet", SMALL, "vit_base_patch16_224"], depths={"resnet": 2, SMALL: 4, "vit_base_patch16_224": 1},
                                             weight_seed=0)
    attacks.AENS_I2V_MF([SMALL, "vgg", "cait_s24_224"], depths={SMALL: [2, 4], "vgg": [2, 3], "cait_s24_224": [1]}, step_size=0.005, weight_seed=0)
    with pytest.raises(KeyError):
        attacks.ImageGuidedFMDirection_Adam([SMALL], depth=5, step_size=0.005, weight_seed=0)
    with pytest.raises(ValueError, match="not a model of this table"):
        attacks.ImageGuidedFMDirection_Adam(["convit_large"], depth=2, step_size=0.005, weight_seed=0)
    import image_main
    monkeypatch.setattr(image_main, "OPT_PATH", str(tmp_path))
    base = ["--attack_method", "ImageGuidedFMDirection_Adam", "--step", "2"]
    for name in (SMALL, "convit_base"):
        a = image_main.arg_parse(base + ["--direction_image_model", name, "--depth", "4"])
        assert image_main.build_attack(a).model_names == [name]
    for bad in (["--direction_image_model", "convit_large"], ["--direction_image_model", SMALL, "--depth", "5"],
                ["--direction_image_model", TINY, "--hw", "112"]):
        with pytest.raises(SystemExit):
            image_main.arg_parse(base + bad)


def test_new_native_symbols_are_exported_by_the_library_and_the_host_simulation():
    import __graft_entry__ as ge
    cd = C.CDLL(ge.LIB)
    assert all(hasattr(cd, n) for n in _lib.CONVIT_EXPORTS)
    assert {"i2v_convit_attention_f32", "i2v_convit_attention_bwd_f32", "i2v_convit_join_cls_f32", "i2v_convit_join_cls_bwd_f32", "i2v_convit_create", "i2v_convit_destroy", "i2v_convit_workspace_bytes",
            "i2v_convit_forward", "i2v_convit_backward", "i2v_convit_hook_info", "i2v_convit_read_hook"} == set(_lib.CONVIT_EXPORTS)
    assert not set(_lib.CONVIT_EXPORTS) & (set(_lib.EXPORTS) | set(_lib.VIT_EXPORTS) | set(_lib.SWIN_EXPORTS) | set(_lib.LOADER_EXPORTS)
                                           | set(_lib.CONVNEXT_EXPORTS) | set(_lib.MIXER_EXPORTS) | set(_lib.CAIT_EXPORTS))
    assert {"i2v_convit.hip", "i2v_convit.cpp"} <= set(ge.UNITS) and "-DI2V_HAVE_CONVIT" in ge.FLAGS
    assert {"i2v_convit_host.h", "i2v_convit_kernels.h"} <= set(ge.HEADERS)
    hs = C.CDLL(os.path.join(ROOT, "tests", "hostsim", "libi2v_hostsim.so"))
    assert all(hasattr(hs, n) for n in _lib.CONVIT_EXPORTS) and not hasattr(hs, "i2v_swin_create") and not hasattr(hs, "i2v_vit_create")
    assert "I2V_HAVE_CONVIT" not in open(os.path.join(ROOT, "tests", "hostsim", "build.sh")).read()
    header = open(os.path.join(ROOT, "include", "i2v_convit.h")).read()
    assert all(n + "(" in header for n in _lib.CONVIT_EXPORTS)


def test_planned_bytes_are_counted_in_64_bits_and_grow_as_the_saves_do():
    t = graphs.build("convit_base")
    assert 2 ** 33 < t.workspace_bytes([11], 128) < 2 ** 37               # past 32 bits
    T, D, H = t.tokens, t.dim, t.heads
    per = lambda blocks: t.workspace_bytes(blocks, 3) - t.workspace_bytes(blocks, 2)       # noqa: E731
    # one more frame costs per further GPSA block: x, qkv, y (5 D per token), h (4 D), four statistics, and H x T x 196 probabilities
    assert per([7]) - per([6]) == 4 * (T * (5 * D + 4 * D + 4) + H * T * 196)
    # ... and the step across the join: block 10 at 197 tokens with rows of 200, the shared scratch and the hook grown to 197 tokens, and
    # the two patch-token streams at the join
    assert per([10]) - per([9]) == 4 * (197 * (9 * D + 4) + H * 197 * 200 + (6 * D + 4 * D) + H * (197 * 200 - 196 * 196) + 2 * T * D + D)


# ---- the planner (csrc/i2v_convit.cpp) on the host simulation ----------------------------------------------------------------------
@pytest.fixture(scope="module")
def twin_refs():
    """The float64 reference of each twin case, computed once: label -> (spec, sd, x, features, hook gradients, input gradient)."""
    out = {}
    for label, (side, _) in mk.TWINS.items():
        spec = graphs.build_tiny(SMALL, (side, side))
        sd = weights.synthetic_state_dict(spec, 0)
        x = mk.twin_input(label)
        ref = ConvitReference(spec, sd, mk.TWIN_HOOKS)
        rf = ref.forward(x)
        hg = [_rand(*f.shape, seed=30 + i) for i, f in enumerate(rf)]
        out[label] = (spec, sd, x, rf, hg, ref.backward(hg))
    return out


@pytest.mark.parametrize("label", sorted(mk.TWINS))
def test_twin_on_the_host_simulation_against_float64(eng, twin_refs, label):
    """Features at all four depths (depth 4 behind the join, one token more) and the input gradient with all four hook gradients
    flowing; a net planned for 5 frames gives the same bits, frame 0 the bits of a 1-frame run; hooks in another order; a single hook
    below the join, at the last GPSA block and behind the join gives the same features and its own gradient."""
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
    for i in (1, 2, 3):                                                   # one hook: the net is truncated there (3, 5: no join; 7: behind it)
        fa, ga = _run_twin(eng, spec, sd, [blocks[i]], x, [hg[i]])
        assert torch.equal(fa[0], feats[i])
        ref1 = ConvitReference(spec, sd, [blocks[i]])
        ref1.forward(x)
        assert _rel(ga, ref1.backward([hg[i]])) < bound(fp["grad"], NET_FLOOR)


def test_the_cases_can_see_the_gate_the_grid_and_the_join(eng, twin_refs):
    """Sensitivity: (a) c = 1 with a zero table (plain attention in the GPSA blocks), (b) the x and y columns of pos_proj.weight
    swapped, each move every hooked feature of the twin by more than 100 x the bound -- from the reference's and from the library's.
    (c) The class token joining one block early (tests/make_convit_fixtures.early_join: block 5 runs behind the join on its own
    weights): the hook at block 5 changes its width, and the hook at block 7, whose width stays, moves by more than 100 x the bound;
    the library follows `local_blocks` there within the bound."""
    spec, sd, x, rf, hg, _ = twin_refs["convit_test"]
    blocks = mk.TWIN_HOOKS
    feats, _ = _run_twin(eng, spec, sd, blocks, x, hg)
    plain = ConvitReference(spec, sd, blocks, plain=True).forward(x)
    swapped = ConvitReference(spec, sd, blocks, swap_xy=True).forward(x)
    for got, want, pl, sw, cpu in zip(feats, rf, plain, swapped, FP32["convit_test"]["hooks"]):
        b = bound(cpu, NET_FLOOR)
        assert _rel(pl, want) > 100 * b and _rel(sw, want) > 100 * b
        assert _rel(got, pl) > 100 * b and _rel(got, sw) > 100 * b
    spec_e, sd_e = mk.early_join(spec, sd)
    early = ConvitReference(spec_e, sd_e, blocks).forward(x)
    assert early[2].shape[1] == 17 * 32 != rf[2].shape[1] and early[3].shape == rf[3].shape
    b = bound(FP32["convit_test"]["hooks"][3], NET_FLOOR)
    assert _rel(early[3], rf[3]) > 100 * b and _rel(feats[3], early[3]) > 100 * b
    got_e, _ = _run_twin(eng, spec_e, sd_e, blocks, x, [_rand(*f.shape, seed=40 + i) for i, f in enumerate(early)])
    for g, w, cpu in zip(got_e, early, FP32[mk.EARLY]["hooks"]):
        assert _rel(g, w) < bound(cpu, NET_FLOOR)


def test_planner_refusals_on_the_host_simulation(eng):
    spec = graphs.build_tiny(SMALL, (64, 64))
    sd = weights.synthetic_state_dict(spec, 0)
    with pytest.raises(_lib.I2VError, match="hooked twice"):
        eng.build_convit_net(spec, sd, [1, 1], 2)
    with pytest.raises(_lib.I2VError, match="outside"):
        eng.build_convit_net(spec, sd, [8], 2)
    net = eng.build_convit_net(spec, sd, [0], 2)
    with pytest.raises(_lib.I2VError, match="planned for"):
        net.forward(torch.zeros(3, 3, 64, 64))
    with pytest.raises(_lib.I2VError):
        net.forward(torch.zeros(2, 3, 32, 32))
    net.close()
    # the convit_base plan at 128 frames, depth 3, without allocating: the figure of DESIGN.md section 22
    assert graphs.build("convit_base").workspace_bytes([8], 128) == mk.WORKSPACE_BASE_D3


def test_i2v_trajectory_on_the_twin_matches_the_reference(eng):
    """4 steps of the I2V attack at depth 4 -- behind the join -- against `restate.run_attack` on the float32 reference net (costs at
    rtol 2e-4, as tests/test_cait_cpu.py)."""
    torch.manual_seed(5)
    vid = torch.randn(1, 3, 2, 64, 64)
    atk = attacks.ImageGuidedFMDirection_Adam([SMALL], depth=4, step_size=0.005, steps=4, engine=eng, graph_builder=graphs.build_tiny,
                                              weight_seed=0)
    adv = atk(vid, torch.zeros(1, dtype=torch.long), ["t"])
    g = graphs.build_tiny(SMALL, (64, 64))
    check_trajectory(atk, adv, ConvitReference(g, weights.synthetic_state_dict(g, 0), [g.hook_for(4)], dtype=torch.float32), vid, rtol=2e-4, steps=4)


def test_aens_of_the_twin_with_tiny_resnet_matches_the_oracle(eng):
    torch.manual_seed(6)
    vid = torch.randn(1, 3, 2, 64, 64)
    depths = {SMALL: [1, 4], "resnet": [2, 3]}
    atk = attacks.AENS_I2V_MF([SMALL, "resnet"], depths=depths, step_size=0.005, steps=3, momentum=0.5, engine=eng,
                              graph_builder=graphs.build_tiny, weight_seed=0)
    _, _, costs = atk(vid, torch.zeros(1, dtype=torch.long), ["a"])
    cs, rs = (graphs.build_tiny(n, (64, 64)) for n in (SMALL, "resnet"))
    nets = [ConvitReference(cs, weights.synthetic_state_dict(cs, 0), [cs.hook_for(d) for d in depths[SMALL]], dtype=torch.float32),
            restate.OracleNet(rs, weights.synthetic_state_dict(rs, 0), [rs.hook_for(d, True) for d in depths["resnet"]], dtype=torch.float32)]
    ref = restate.run_attack(nets, vid, steps=3, step_size=0.005, mode="aens", coeffs=torch.ones(4), momentum=0.5)
    np.testing.assert_allclose(costs, ref["costs"], rtol=2e-4)
