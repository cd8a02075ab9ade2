"""CPU: timm's BEiT family as image surrogates on the transformer stack -- for both served names the spec, the hooks
and the key / shape contract against tests/golden/timm_beit_keys.json; the refusals; checkpoint loading with the index buffer verified;
the packing (the built qkv bias, the folded LayerScale, the dense bias) against timm's literal arithmetic, and that leaving the new
arithmetic out is seen; the attention entries on the host simulation, which runs them as scalar code (csrc/i2v_beit_host.h); and the
planner itself (csrc/i2v_beit.cpp) on the host simulation: all three twins against float64, under both routes, a 4-step I2V attack and an
AENS ensemble against the oracle.

The bound is relative L2 against float64: the larger of the floor for that kind of case (entries 1e-6 forward, 1e-5 backward; nets 1e-5)
and 4 x the error of the float32 CPU run of the same reference on the same inputs, read from tests/golden/beit_fp32_cpu_errors.json
(tests/make_beit_fixtures.py).  A case without a recorded error fails (KeyError)."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from i2v_amd import attacks, graphs, weights
from i2v_amd import lib as _lib
from oracle import restate
from tests import beit_reference as br
from tests import make_beit_fixtures as mk
from tests.beit_reference import BeitReference
from tests.family_harness import bound, check_net, check_trajectory, rand as _rand, rel as _rel, run_twin as _run_twin
from tests.hostsim_util import hostsim_engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = json.load(open(os.path.join(ROOT, "tests", "golden", "timm_beit_keys.json")))
FP32 = json.load(open(os.path.join(ROOT, "tests", "golden", "beit_fp32_cpu_errors.json")))
TABLE = {"beit_base_patch16_224": (16, 768, 12, 3072, 12), "beit_large_patch16_224": (16, 1024, 16, 4096, 24)}
NAMES = sorted(TABLE)
BASE, LARGE = "beit_base_patch16_224", "beit_large_patch16_224"
NET_FLOOR, FWD_FLOOR, BWD_FLOOR = 1e-5, 1e-6, 1e-5


# ---- the specs ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_param_shapes_equal_the_key_fixture(name):
    """The golden list is timm's state dict, buffers included; `param_shapes` is that list without the index buffers, in its order."""
    want = {k: tuple(v) for k, v in KEYS["names"][name].items()}
    spec = graphs.build(name)
    index = {spec.index_key(i): (197, 197) for i in range(spec.blocks)}
    assert {k: v for k, v in want.items() if k.endswith("relative_position_index")} == index
    params = {k: v for k, v in want.items() if k not in index}
    shapes = spec.param_shapes()
    assert shapes == params and list(shapes) == list(params)
    assert list(want).index(spec.index_key(3)) == list(want).index("blocks.3.attn.relative_position_bias_table") + 1
    assert KEYS["checked_against"].startswith(("timm ", "unchecked"))


@pytest.mark.parametrize("name", NAMES)
def test_spec_sizes_and_hooks_of_every_name(name):
    patch, dim, heads, mlp, blocks = TABLE[name]
    spec = graphs.build(name)
    assert isinstance(spec, graphs.BeitSpec) and spec.arch == name and spec.video is False and spec.in_hw == (224, 224)
    assert (spec.img, spec.patch, spec.in_chans, spec.dim, spec.heads, spec.mlp, spec.blocks, spec.ln_eps) == (224, patch, 3, dim, heads, mlp, blocks, 1e-6)
    assert (spec.grid, spec.tokens, spec.table_rows, spec.dim // spec.heads) == (14, 197, 732, 64)
    hooks = [spec.hook_for(d) for d in (1, 2, 3, 4)]
    assert hooks == ([2, 5, 8, 11] if blocks == 12 else [5, 11, 17, 23]) and spec.hook_dim == 197 * dim
    with pytest.raises(KeyError):
        spec.hook_for(5)
    assert graphs.beit_named(name) == spec and graphs.is_beit_name(name)
    assert not any(f(name) for f in (graphs.is_swin_name, graphs.is_vit_name, graphs.is_convnext_name, graphs.is_mixer_name, graphs.is_cait_name,
                                     graphs.is_convit_name, graphs.is_xcit_name, graphs.is_twins_name))
    shapes = spec.param_shapes()
    assert shapes["blocks.0.attn.relative_position_bias_table"] == (732, heads) and shapes["blocks.1.attn.qkv.weight"] == (3 * dim, dim)
    assert "pos_embed" not in shapes and "rel_pos_bias.relative_position_bias_table" not in shapes and "blocks.0.attn.qkv.bias" not in shapes
    assert not any(k.startswith(("head.", "norm.", "fc_norm.")) for k in shapes)
    assert spec.macs_per_frame() > 196 * dim * 768 + blocks * 197 * dim * (4 * dim + 2 * mlp)
    for hw in ((384, 384), (112, 112), (224, 192)):
        with pytest.raises(ValueError, match="224 x 224") as ei:
            graphs.build(name, hw)
        assert all(n in str(ei.value) for n in TABLE)


def test_refusals_name_the_reason_and_list_the_served_names():
    for name, why in (("beit_base_patch16_384", "384 x 384 and 512 x 512"), ("beit_large_patch16_512", "384 x 384 and 512 x 512"),
                      ("beit_base_patch16_224_in22k", "in22k"), ("beit_large_patch16_224_in22k", "in22k"), ("beit_", "not a model of this table"),
                      ("beit_tiny_patch16_224", "not a model of this table"), ("beit_base_patch32_224", "not a model of this table")):
        assert graphs.is_beit_name(name)
        with pytest.raises(ValueError, match=why) as ei:
            graphs.build(name)
        assert all(n in str(ei.value) for n in TABLE)
        with pytest.raises(ValueError, match=why):
            graphs.build_tiny(name)


def test_existing_names_behave_as_before():
    with pytest.raises(UnboundLocalError):
        graphs.build("transformer")
    with pytest.raises(UnboundLocalError):
        graphs.build("pit_s_224")
    with pytest.raises(ValueError, match="not served"):
        graphs.build("mobilenet_v2")
    assert not any(graphs.is_beit_name(n) for n in ("convnext_tiny", "vit_base_patch16_224", "swin_tiny_patch4_window7_224", "xcit_nano_12_p16_224",
                                                    "twins_svt_small", "cait_s24_224", "convit_base", "mixer_b16_224", "resnet", "conv", "pit_s_224"))
    assert isinstance(graphs.build("vit_base_patch16_224"), graphs.VitSpec) and isinstance(graphs.build("twins_svt_small"), graphs.TwinsSpec)
    assert isinstance(graphs.build("swin_tiny_patch4_window7_224"), graphs.SwinSpec) and graphs.build("resnet").arch == "resnet101"
    others = (set(graphs.SWIN_MODELS) | set(graphs.VIT_MODELS) | set(graphs.CONVNEXT_MODELS) | set(graphs.MIXER_MODELS) | set(graphs.CAIT_MODELS)
              | set(graphs.CONVIT_MODELS) | set(graphs.XCIT_MODELS) | set(graphs.TWINS_MODELS))
    assert not set(graphs.BEIT_MODELS) & others and graphs.BEIT_MODELS == TABLE


def test_test_size_twins():
    t = graphs.build_tiny(BASE, (64, 64))
    assert t == graphs.build_tiny(LARGE, (64, 64)) == graphs.beit_tiny_twin()
    assert (t.arch, t.grid, t.tokens, t.table_rows, t.dim, t.heads, t.blocks) == ("beit_test", 4, 17, 52, 64, 2, 8)
    assert [t.hook_for(d) for d in (1, 2, 3, 4)] == [1, 3, 5, 7]
    t96 = graphs.build_tiny(BASE, (96, 96))
    assert (t96.arch, t96.grid, t96.tokens, t96.table_rows, t96.dim, t96.heads, t96.blocks) == ("beit_test_96", 6, 37, 124, 48, 4, 8)
    assert t96.tokens % 4 and t96.tokens % 16 and (t96.dim // t96.heads) % 16
    t224 = graphs.build_tiny(LARGE, (224, 224))
    assert (t224.arch, t224.tokens, t224.dim, t224.heads, t224.blocks) == ("beit_test_224", 197, 64, 1, 4)
    assert [t224.hook_for(d) for d in (1, 2, 3, 4)] == [0, 1, 2, 3]
    assert not any(tw.arch in graphs.BEIT_MODELS for tw in (t, t96, t224))
    for hw in ((72, 72), (128, 128), (64, 96)):
        with pytest.raises(ValueError):
            graphs.build_tiny(BASE, hw)
    ref = BeitReference(t, weights.synthetic_state_dict(t, 0), [1, 7])
    f = ref.forward(torch.randn(2, 3, 64, 64))
    assert [tuple(a.shape) for a in f] == [(2, 17 * 64)] * 2
    assert ref.backward([torch.ones_like(a) for a in f]).shape == (2, 3, 64, 64)


# ---- checkpoints and packing -------------------------------------------------------------------------------------------------------
def _checkpoint(spec, with_index=True):
    """A timm-shaped checkpoint with the keys behind every hook as well, and the index buffers."""
    D = spec.dim
    sd = {k: torch.zeros(1).expand(shp) for k, shp in spec.param_shapes().items()}
    sd.update({"fc_norm.weight": torch.ones(D), "fc_norm.bias": torch.zeros(D), "head.weight": torch.zeros(1).expand(1000, D), "head.bias": torch.zeros(1000)})
    if with_index:
        sd.update({spec.index_key(i): br.relative_position_index(spec.grid) for i in range(spec.blocks)})
    return sd


def test_checkpoint_loads_and_its_index_buffer_is_verified(tmp_path, monkeypatch):
    spec = graphs.build(BASE)
    monkeypatch.delenv("I2V_SYNTHETIC_WEIGHTS", raising=False)
    monkeypatch.setenv("I2V_WEIGHTS_DIR", str(tmp_path))
    with pytest.raises(weights.MissingWeights, match=BASE):
        weights.load_state_dict(spec)
    path = tmp_path / f"{BASE}.pth"
    for with_index in (True, False):                                      # a present index is verified, an absent one tolerated
        sd = _checkpoint(spec, with_index)
        sd["blocks.4.gamma_2"] = torch.full((spec.dim,), 0.25)
        torch.save(sd, path)
        got = weights.load_state_dict(spec)
        assert list(got) == list(spec.param_shapes()) and "head.weight" not in got and spec.index_key(0) not in got
        assert all(tuple(got[k].shape) == shp and got[k].is_contiguous() for k, shp in spec.param_shapes().items())
        assert float(got["blocks.4.gamma_2"].mean()) == 0.25
    sd = _checkpoint(spec)
    wrong = sd[spec.index_key(7)].clone()
    wrong[5, 9] += 1
    torch.save(dict(sd, **{spec.index_key(7): wrong}), path)
    with pytest.raises(ValueError, match=r"blocks\.7\.attn\.relative_position_index"):
        weights.load_state_dict(spec)
    torch.save(dict(sd, **{spec.index_key(2): torch.zeros(577, 577, dtype=torch.int64)}), path)      # another grid's buffer
    with pytest.raises(ValueError, match=r"blocks\.2\.attn\.relative_position_index"):
        weights.load_state_dict(spec)
    torch.save(dict(sd, **{"blocks.1.attn.relative_position_bias_table": torch.zeros(2212, 12)}), path)
    with pytest.raises(ValueError, match=r"blocks\.1\.attn\.relative_position_bias_table"):
        weights.load_state_dict(spec)
    short = dict(sd)
    del short["blocks.11.attn.v_bias"]
    torch.save(short, path)
    with pytest.raises(KeyError, match=r"blocks\.11\.attn\.v_bias"):
        weights.load_state_dict(spec)
    with pytest.raises(weights.MissingWeights):                             # every name reads its own file
        weights.load_state_dict(graphs.build(LARGE))


def test_synthetic_weights_let_the_new_arithmetic_show():
    spec = graphs.build_tiny(BASE, (64, 64))
    sd = weights.load_state_dict(spec, seed=3)
    assert {k: tuple(v.shape) for k, v in sd.items()} == spec.param_shapes() and not any("relative_position_index" in k for k in sd)
    for i in range(spec.blocks):
        p = f"blocks.{i}."
        assert 0.7 < float(sd[p + "attn.relative_position_bias_table"].std()) < 1.3
        for k in ("gamma_1", "gamma_2"):
            assert 0.5 <= float(sd[p + k].min()) and float(sd[p + k].max()) <= 1.5 and float(sd[p + k].std()) > 0.2
        assert float(sd[p + "attn.q_bias"].abs().mean()) > 0.03 and float(sd[p + "attn.v_bias"].abs().mean()) > 0.03


@pytest.mark.parametrize("g", [4, 6, 14])
def test_dense_bias_equals_the_reference_gather_exactly(g):
    spec = graphs.BeitSpec("beit_probe", 16 * g, 16, 3, 32, 2, 64, 4)
    assert torch.equal(spec.relative_position_index(), br.relative_position_index(g))
    idx = spec.relative_position_index()
    n = spec.table_rows
    assert n == (2 * g - 1) ** 2 + 3 and int(idx.max()) == n - 1 and int(idx[1:, 1:].max()) == n - 4 and int(idx[1:, 1:].min()) == 0
    assert int(idx[0, 0]) == n - 1 and set(idx[0, 1:].tolist()) == {n - 3} and set(idx[1:, 0].tolist()) == {n - 2}
    sd = weights.synthetic_state_dict(spec, 1)
    arrays = spec.native_arrays(sd, 2)
    assert len(arrays) == 3 + 13 * 2
    for i in range(2):
        dense = arrays[3 + 13 * i + 4]
        assert dense.shape == (2, g * g + 1, g * g + 1) and dense.is_contiguous()
        assert torch.equal(dense, br.gathered_bias(sd[f"blocks.{i}.attn.relative_position_bias_table"], g))


def test_packing_builds_the_qkv_bias_and_folds_layerscale():
    spec = graphs.build_tiny(BASE, (64, 64))
    sd = weights.synthetic_state_dict(spec, 0)
    arrays = spec.native_arrays(sd, 3)
    D = spec.dim
    assert arrays[0].shape == (D, 3 * 16 * 16) and arrays[2].shape == (D,) and torch.equal(arrays[2], sd["cls_token"].reshape(D))
    x, h = _rand(5, D, seed=1), _rand(5, spec.mlp, seed=2)
    for i in range(3):
        a, p = arrays[3 + 13 * i:16 + 13 * i], f"blocks.{i}."
        assert [tuple(t.shape) for t in a] == [(D,), (D,), (3 * D, D), (3 * D,), (2, 17, 17), (D, D), (D,), (D,), (D,), (spec.mlp, D), (spec.mlp,),
                                               (D, spec.mlp), (D,)]
        assert all(t.dtype == torch.float32 and t.is_contiguous() for t in a)
        qkvb = a[3]
        assert float(qkvb[D:2 * D].abs().max()) == 0.0                     # the k part is exactly zero
        assert torch.equal(qkvb[:D], sd[p + "attn.q_bias"]) and torch.equal(qkvb[2 * D:], sd[p + "attn.v_bias"])
        # folding equals the scale-after arithmetic to rounding
        want = sd[p + "gamma_1"].double() * (x @ sd[p + "attn.proj.weight"].double().t() + sd[p + "attn.proj.bias"].double())
        assert _rel(x @ a[5].double().t() + a[6].double(), want) < 2e-7
        want = sd[p + "gamma_2"].double() * (h @ sd[p + "mlp.fc2.weight"].double().t() + sd[p + "mlp.fc2.bias"].double())
        assert _rel(h @ a[11].double().t() + a[12].double(), want) < 2e-7


# ---- the entries on the host simulation --------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def eng():
    e = hostsim_engine()
    _lib.bind(e.capi, _lib._BEIT_PROTOS)
    return e


def _f(v):
    return None if v is None else v.float().contiguous()


def run_attn(eng, d):
    """(out, dq, dk, dv) of an attention case through the two C entries."""
    qkv, bias = _f(d["qkv"]), _f(d["bias"])
    out = eng.beit_attention(qkv, bias, d["heads"])
    dqkv = eng.beit_attention_bwd(qkv, bias, _f(d["dout"]), d["heads"])
    Cn = qkv.shape[2] // 3
    return out, dqkv[:, :, :Cn], dqkv[:, :, Cn:2 * Cn], dqkv[:, :, 2 * Cn:]


def check_attn(got, want, fp, T, label):
    """out, dq, dk and dv, each against float64 at its own bound; a single key makes dq and dk exactly 0."""
    errs = {"fwd": _rel(got[0], want[0]), "dv": _rel(got[3], want[3])}
    if T == 1:
        assert float(got[1].abs().max()) == 0.0 and float(got[2].abs().max()) == 0.0
        assert float(want[1].abs().max()) < 1e-12 and float(want[2].abs().max()) < 1e-12
    else:
        errs.update({"dq": _rel(got[1], want[1]), "dk": _rel(got[2], want[2])})
    print(f"{label}: " + ", ".join(f"{k} {v:.3e} (fp32 CPU {fp[k]:.3e})" for k, v in errs.items()))
    for k, v in errs.items():
        assert v < bound(fp[k], FWD_FLOOR if k == "fwd" else BWD_FLOOR), (k, v, fp[k])


@pytest.mark.parametrize("F_,T,H,dh,kind", mk.ATTN_CASES)
def test_attention_host_twin_against_float64_autograd(eng, F_, T, H, dh, kind):
    d = mk.attn_case(F_, T, H, dh, kind)
    got = run_attn(eng, d)
    check_attn(got, mk.attn_reference(d), FP32["attention"][mk.case_key(F_, T, H, dh, kind)], T, f"host F {F_} T {T} H {H} dh {dh} {kind}")
    if kind == "hot":                                                      # the case is what it says: the row maximum in the last key tile
        s = (d["qkv"][:, :, :H * dh].reshape(F_, T, H, dh).permute(0, 2, 1, 3) @ d["qkv"][:, :, H * dh:2 * H * dh].reshape(F_, T, H, dh).permute(0, 2, 3, 1))
        s = s * dh ** -0.5 + d["bias"]
        assert float((s.argmax(-1) >= (T - 1) // 16 * 16).float().mean()) > 0.9 and 25 < float(s.abs().max()) < 70
    again = run_attn(eng, d)
    assert all(torch.equal(a, b) for a, b in zip(got, again))              # reruns: the same bits
    if F_ > 1:                                                             # frame 0 of the F-frame call: the bits of a 1-frame call
        one = run_attn(eng, dict(d, qkv=d["qkv"][:1], dout=d["dout"][:1]))
        assert all(torch.equal(a[:1], b) for a, b in zip(got, one))


def test_a_null_bias_is_plain_attention_and_a_zero_bias_equals_it(eng):
    d = mk.attn_case(2, 37, 2, 16, "nobias")
    z = dict(d, bias=torch.zeros(2, 37, 37, dtype=torch.float64))
    assert all(torch.equal(a, b) for a, b in zip(run_attn(eng, d), run_attn(eng, z)))


def test_the_entries_refuse_with_the_reason(eng):
    z = torch.zeros(65536)                                                 # (room for the largest served call: a 208 x 208 bias)
    p = lambda t: C.c_void_p(t.data_ptr())      # noqa: E731
    capi = eng.capi
    fwd = lambda *, qkv=p(z), bias=p(z), frames=1, T=4, H=2, dh=8, out=p(z): capi.i2v_beit_attention_f32(qkv, bias, frames, T, H, dh, 0.5, out, None)      # noqa: E731
    assert fwd() == 0 and fwd(H=1, dh=64, T=208) == 0 and fwd(bias=None) == 0          # the limits and a null bias are served
    off = C.c_void_p(z.data_ptr() + 4)
    for kw, why in ((dict(qkv=None), b"null"), (dict(out=None), b"null"), (dict(frames=0), b"positive"), (dict(dh=6), b"multiple of 4"),
                    (dict(H=1, dh=68), b"wider than 64"), (dict(T=209, H=1), b"more than 208 tokens"), (dict(frames=70000), b"65535"),
                    (dict(H=70000, dh=4), b"65535"), (dict(frames=60000, T=197, H=3, dh=64), b"2^31"), (dict(qkv=off), b"alignment"),
                    (dict(bias=off), b"alignment"), (dict(out=off), b"alignment")):
        assert fwd(**kw) != 0
        err = capi.i2v_last_error()
        assert b"beit_attention" in err and b"hipErrorInvalidValue" in err and why in err, err
    bwd = lambda *, dh=8, T=4, g=p(z), dqkv=p(z), bias=p(z): capi.i2v_beit_attention_bwd_f32(p(z), bias, g, 1, T, 2, dh, 0.5, dqkv, None)      # noqa: E731
    y = C.c_void_p(z.data_ptr() + 4096)
    assert bwd(dqkv=y) == 0 and bwd(dqkv=y, bias=None) == 0
    for kw, why in ((dict(dh=6), b"multiple of 4"), (dict(T=209), b"more than 208 tokens"), (dict(g=None), b"null"), (dict(dqkv=None), b"null"),
                    (dict(dqkv=off), b"alignment")):
        assert bwd(**kw) != 0
        assert b"beit_attention_bwd" in capi.i2v_last_error() and why in capi.i2v_last_error(), capi.i2v_last_error()


def test_bias_add_host_twin_is_exact_and_refuses(eng):
    S, b = _rand(3, 2, 5, 8, seed=1).float(), _rand(2, 5, 8, seed=2).float()
    assert torch.equal(eng.beit_bias_add(S.clone(), b), S + b)
    p = lambda t: C.c_void_p(t.data_ptr())      # noqa: E731
    for args, why in (((None, p(b), 3, 80), b"null"), ((p(S), p(b), 3, 78), b"multiple of 4"), ((p(S), C.c_void_p(b.data_ptr() + 4), 3, 76), b"alignment")):
        assert eng.capi.i2v_beit_bias_add_f32(*args, None) != 0
        assert b"beit_bias_add" in eng.capi.i2v_last_error() and why in eng.capi.i2v_last_error()


# ---- the attack classes, the CLI, the symbols --------------------------------------------------------------------------------------
def test_attack_classes_and_the_cli_take_the_names(tmp_path, monkeypatch):
    for name in NAMES:
        atk = attacks.ImageGuidedFMDirection_Adam([name], depth=4, step_size=0.005, steps=2, weight_seed=0)
        assert atk.model_names == [name]
    attacks.ImageGuidedStd_Adam([BASE], depth=1, step_size=0.005, weight_seed=0)
    attacks.ImageGuidedFML2_Adam_MultiModels([BASE, "resnet"], depths={BASE: 2, "resnet": 3}, weight_seed=0)
    attacks.AENS_I2V_MF([LARGE, "vgg", "twins_svt_small"], depths={LARGE: [2, 4], "vgg": [2, 3], "twins_svt_small": [1]}, step_size=0.005, weight_seed=0)
    with pytest.raises(KeyError):
        attacks.ImageGuidedFMDirection_Adam([BASE], depth=5, step_size=0.005, weight_seed=0)
    with pytest.raises(ValueError, match="in22k"):
        attacks.ImageGuidedFMDirection_Adam(["beit_base_patch16_224_in22k"], depth=2, step_size=0.005, weight_seed=0)
    import image_main
    monkeypatch.setattr(image_main, "OPT_PATH", str(tmp_path))
    base = ["--attack_method", "ImageGuidedFMDirection_Adam", "--step", "2"]
    for name in NAMES:
        for depth in ("1", "2", "3", "4"):
            a = image_main.arg_parse(base + ["--direction_image_model", name, "--depth", depth])
            assert image_main.build_attack(a).model_names == [name]
    for bad in (["--direction_image_model", "beit_base_patch16_384"], ["--direction_image_model", BASE, "--depth", "5"],
                ["--direction_image_model", BASE, "--hw", "112"]):
        with pytest.raises(SystemExit):
            image_main.arg_parse(base + bad)


def test_new_native_symbols_are_exported_by_the_library_and_the_host_simulation():
    import __graft_entry__ as ge
    cd = C.CDLL(ge.LIB)
    assert all(hasattr(cd, n) for n in _lib.BEIT_EXPORTS)
    assert {"i2v_beit_create", "i2v_beit_destroy", "i2v_beit_workspace_bytes", "i2v_beit_forward", "i2v_beit_backward", "i2v_beit_hook_info",
            "i2v_beit_read_hook", "i2v_beit_attention_f32", "i2v_beit_attention_bwd_f32", "i2v_beit_bias_add_f32"} == set(_lib.BEIT_EXPORTS)
    assert not set(_lib.BEIT_EXPORTS) & (set(_lib.EXPORTS) | set(_lib.VIT_EXPORTS) | set(_lib.SWIN_EXPORTS) | set(_lib.LOADER_EXPORTS)
                                         | set(_lib.CONVNEXT_EXPORTS) | set(_lib.MIXER_EXPORTS) | set(_lib.CAIT_EXPORTS) | set(_lib.CONVIT_EXPORTS)
                                         | set(_lib.XCIT_EXPORTS) | set(_lib.TWINS_EXPORTS))
    assert {"i2v_beit.hip", "i2v_beit.cpp"} <= set(ge.UNITS) and "-DI2V_HAVE_BEIT" in ge.FLAGS
    assert {"i2v_beit_host.h", "i2v_beit_kernels.h"} <= set(ge.HEADERS)
    hs = C.CDLL(os.path.join(ROOT, "tests", "hostsim", "libi2v_hostsim.so"))
    assert all(hasattr(hs, n) for n in _lib.BEIT_EXPORTS) and not hasattr(hs, "i2v_vit_create")
    assert "I2V_HAVE_BEIT" not in open(os.path.join(ROOT, "tests", "hostsim", "build.sh")).read()
    header = open(os.path.join(ROOT, "include", "i2v_beit.h")).read()
    assert all(n + "(" in header for n in _lib.BEIT_EXPORTS)


def test_planned_bytes_are_counted_in_64_bits_and_grow_as_the_saves_do():
    big = graphs.build(LARGE)
    assert 2 ** 34 < big.workspace_bytes([23], 128, composed=False) < big.workspace_bytes([23], 128, composed=True) < 2 ** 38      # past 32 bits
    b = graphs.build(BASE)
    T, D, M, H = 197, 768, 3072, 12
    per = lambda hooks, c: b.workspace_bytes(hooks, 3, composed=c) - b.workspace_bytes(hooks, 2, composed=c)       # noqa: E731
    # one more frame costs per block x, qkv (3 D), y, h and four statistics; the scratch six streams, one MLP-wide, the patch rows and
    # their embedding; a hook view.  Three blocks more cost three blocks' saves.
    assert per([8], False) - per([5], False) == 4 * 3 * T * (5 * D + M + 4)
    assert per([5], False) == 4 * (6 * T * (5 * D + M + 4) + 6 * T * D + T * M + 196 * (768 + D) + T * D)
    # under the switch: per block and once more as scratch, the probabilities at row stride 200
    assert per([5], True) - per([5], False) == 4 * 7 * H * T * 200
    assert b.workspace_bytes([5], 2, composed=True) - b.workspace_bytes([5], 2, composed=False) == 4 * (7 * 2 * H * T * 200 + 6 * H * T * 200)


# ---- the planner (csrc/i2v_beit.cpp) on the host simulation ------------------------------------------------------------------------
@pytest.fixture(scope="module")
def twin_refs():
    """The float64 reference of each twin case, computed once: label -> (spec, sd, x, hooks, features, hook gradients, input gradient)."""
    out = {}
    for label, (name, side, _) in mk.TWINS.items():
        spec = graphs.build_tiny(name, (side, side))
        sd = weights.synthetic_state_dict(spec, 0)
        x = mk.twin_input(label)
        hooks = [spec.hook_for(d) for d in (1, 2, 3, 4)]
        ref = BeitReference(spec, sd, hooks)
        rf = ref.forward(x)
        hg = [_rand(*f.shape, seed=30 + i) for i, f in enumerate(rf)]
        out[label] = (spec, sd, x, hooks, rf, hg, ref.backward(hg))
    return out


@pytest.mark.parametrize("label", sorted(mk.TWINS))
def test_twin_on_the_host_simulation_against_float64(eng, twin_refs, label):
    """Features at all four depths and the input gradient with all four hook gradients flowing; reruns and a net planned for 5 frames
    give the same bits, frame 0 the bits of a 1-frame run; hooks in another order; a single hook gives the same features and its own
    gradient."""
    spec, sd, x, hooks, rf, hg, want_gx = twin_refs[label]
    assert spec.arch == label
    feats, gx = _run_twin(eng, spec, sd, hooks, x, hg)
    check_net(label, feats, gx, rf, want_gx, FP32[label], NET_FLOOR)
    f1, g1 = _run_twin(eng, spec, sd, hooks, x[:1], [h[:1] for h in hg])
    assert all(torch.equal(a[:1], b) for a, b in zip(feats, f1)) and torch.equal(gx[:1], g1)
    feats2, gx2 = _run_twin(eng, spec, sd, hooks, x, hg, max_frames=5)
    assert all(torch.equal(a, b) for a, b in zip(feats, feats2)) and torch.equal(gx, gx2)
    fo, go = _run_twin(eng, spec, sd, hooks[::-1], x, hg[::-1])           # hooks in another order
    assert all(torch.equal(a, b) for a, b in zip(feats, fo[::-1])) and torch.equal(gx, go)
    fa, ga = _run_twin(eng, spec, sd, [hooks[1]], x, [hg[1]])             # one hook: the net is truncated there
    assert torch.equal(fa[0], feats[1])
    ref1 = BeitReference(spec, sd, [hooks[1]])
    ref1.forward(x)
    assert _rel(ga, ref1.backward([hg[1]])) < bound(FP32[label]["grad"], NET_FLOOR)


@pytest.mark.parametrize("label", ["beit_test", "beit_test_96"])
def test_twin_on_the_shared_launch_route_against_float64(eng, twin_refs, label, monkeypatch):
    """I2V_BEIT_ATTN=0, read when the net is planned: the core as gemm + bias add + softmax + gemm with P kept, backward the softmax
    backward and four products.  The same bound; the plan holds what the formula says under the switch; a net planned without the
    switch afterwards is the attention launch's again."""
    spec, sd, x, hooks, rf, hg, want_gx = twin_refs[label]
    plain = spec.workspace_bytes(hooks, x.shape[0], composed=False)
    monkeypatch.setenv("I2V_BEIT_ATTN", "0")
    feats, gx = _run_twin(eng, spec, sd, hooks, x, hg)                    # (checks the planned bytes against the formula under the switch)
    T, ld = spec.tokens, (spec.tokens + 3) // 4 * 4
    probs = x.shape[0] * spec.heads * T * ld
    assert spec.workspace_bytes(hooks, x.shape[0]) - plain == 4 * ((spec.blocks + 1) * probs + spec.blocks * spec.heads * T * ld)
    check_net(label, feats, gx, rf, want_gx, FP32[label], NET_FLOOR)
    f1, g1 = _run_twin(eng, spec, sd, hooks, x[:1], [h[:1] for h in hg])
    assert all(torch.equal(a[:1], b) for a, b in zip(feats, f1)) and torch.equal(gx[:1], g1)
    monkeypatch.delenv("I2V_BEIT_ATTN")
    feats0, gx0 = _run_twin(eng, spec, sd, hooks, x, hg)
    assert all(_rel(a, b) < 1e-5 for a, b in zip(feats, feats0)) and _rel(gx, gx0) < 1e-5


@pytest.mark.parametrize("what", ["bias", "gamma"])
def test_leaving_the_new_arithmetic_out_is_seen(eng, twin_refs, what):
    """The position bias and LayerScale carry arithmetic: the reference with a table of zeros, or with gamma = 1, misses every hooked
    feature of beit_test by more than 100 x the bound, and so does the library's result."""
    spec, sd, x, hooks, rf, hg, _ = twin_refs["beit_test"]
    feats, _ = _run_twin(eng, spec, sd, hooks, x, hg)
    without = BeitReference(spec, sd, hooks, skip=(what,)).forward(x)
    for got, want, wo, cpu in zip(feats, rf, without, FP32["beit_test"]["hooks"]):
        assert _rel(wo, want) > 100 * bound(cpu, NET_FLOOR) and _rel(got, wo) > 100 * bound(cpu, NET_FLOOR)
    blind = dict(sd)                                                       # ... and through the packing: the same state dict with the term silenced
    for i in range(spec.blocks):
        p = f"blocks.{i}."
        if what == "bias":
            blind[p + "attn.relative_position_bias_table"] = torch.zeros_like(sd[p + "attn.relative_position_bias_table"])
        else:
            blind[p + "gamma_1"], blind[p + "gamma_2"] = torch.ones(spec.dim), torch.ones(spec.dim)
    fb, _ = _run_twin(eng, spec, blind, hooks, x, hg)
    for got, b, wo, cpu in zip(feats, fb, without, FP32["beit_test"]["hooks"]):
        assert _rel(b, got) > 100 * bound(cpu, NET_FLOOR) and _rel(b, wo) < bound(cpu, NET_FLOOR)


def test_planner_refusals_on_the_host_simulation(eng):
    spec = graphs.build_tiny(BASE, (64, 64))
    sd = weights.synthetic_state_dict(spec, 0)
    with pytest.raises(_lib.I2VError, match="hooked twice"):
        eng.build_beit_net(spec, sd, [1, 1], 2)
    with pytest.raises(_lib.I2VError, match="outside"):
        eng.build_beit_net(spec, sd, [8], 2)
    net = eng.build_beit_net(spec, sd, [1], 2)
    with pytest.raises(_lib.I2VError, match="planned for"):
        net.forward(torch.zeros(3, 3, 64, 64))
    with pytest.raises(_lib.I2VError):
        net.forward(torch.zeros(2, 3, 32, 32))
    net.close()
    h, one = C.c_void_p(), (C.c_int32 * 1)(0)
    create = lambda cfg: eng.capi.i2v_beit_create(0, C.byref(cfg), (C.c_void_p * 16)(), 16, one, 1, 1, C.byref(h))      # noqa: E731
    assert create(_lib.BeitConfig(240, 16, 3, 64, 2, 256, 4, 1e-6)) != 0 and b"226 tokens" in eng.capi.i2v_last_error()      # a 15 x 15 grid
    assert create(_lib.BeitConfig(64, 16, 3, 136, 2, 256, 4, 1e-6)) != 0 and b"heads of width 68" in eng.capi.i2v_last_error()
    assert create(_lib.BeitConfig(64, 16, 3, 60, 10, 256, 4, 1e-6)) != 0 and b"heads of width 6" in eng.capi.i2v_last_error()
    assert eng.capi.i2v_beit_create(0, C.byref(_lib.BeitConfig(64, 16, 3, 64, 2, 256, 4, 1e-6)), (C.c_void_p * 15)(), 15, one, 1, 1, C.byref(h)) != 0
    assert b"15 weight arrays given, 16 expected" in eng.capi.i2v_last_error()


def test_i2v_trajectory_on_the_twin_matches_the_reference(eng):
    """4 steps of the I2V attack at depth 4 against `restate.run_attack` on the float32 reference net (costs at rtol 2e-4, as
    tests/test_twins_cpu.py)."""
    torch.manual_seed(5)
    vid = torch.randn(1, 3, 2, 64, 64)
    atk = attacks.ImageGuidedFMDirection_Adam([BASE], depth=4, step_size=0.005, steps=4, engine=eng, graph_builder=graphs.build_tiny, weight_seed=0)
    adv = atk(vid, torch.zeros(1, dtype=torch.long), ["t"])
    g = graphs.build_tiny(BASE, (64, 64))
    check_trajectory(atk, adv, BeitReference(g, weights.synthetic_state_dict(g, 0), [g.hook_for(4)], dtype=torch.float32), vid, rtol=2e-4, steps=4)


def test_aens_of_the_twin_with_tiny_resnet_matches_the_oracle(eng):
    torch.manual_seed(6)
    vid = torch.randn(1, 3, 2, 96, 96)
    depths = {BASE: [1, 4], "resnet": [2, 3]}
    atk = attacks.AENS_I2V_MF([BASE, "resnet"], depths=depths, step_size=0.005, steps=3, momentum=0.5, engine=eng, graph_builder=graphs.build_tiny,
                              weight_seed=0)
    _, _, costs = atk(vid, torch.zeros(1, dtype=torch.long), ["a"])
    cs, rs = (graphs.build_tiny(n, (96, 96)) for n in (BASE, "resnet"))
    nets = [BeitReference(cs, weights.synthetic_state_dict(cs, 0), [cs.hook_for(d) for d in depths[BASE]], dtype=torch.float32),
            restate.OracleNet(rs, weights.synthetic_state_dict(rs, 0), [rs.hook_for(d, True) for d in depths["resnet"]], dtype=torch.float32)]
    ref = restate.run_attack(nets, vid, steps=3, step_size=0.005, mode="aens", coeffs=torch.ones(4), momentum=0.5)
    np.testing.assert_allclose(costs, ref["costs"], rtol=2e-4)
