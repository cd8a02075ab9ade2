"""CPU: timm's plain ViT / DeiT family as image surrogates -- the family restatement pinned against the ViT-B/16
one and, for the distilled form, by construction; for every served name the spec, token count, hook blocks, key manifest and checkpoint
loading; the refusals; the test-size twins; and the new native symbols."""
import ctypes as C
import os

import pytest
import torch

from i2v_amd import attacks, graphs, weights
from i2v_amd import lib as _lib
from tests import vit_family_reference as fam
from tests.family_harness import rand as _rand
from tests.vit_family_reference import VitFamilyReference
from tests.vit_reference import VitReference

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

#: the issue's table: name -> (patch, dim, heads, mlp, blocks, prefix tokens, tokens)
TABLE = {
    "vit_tiny_patch16_224": (16, 192, 3, 768, 12, 1, 197),
    "deit_tiny_patch16_224": (16, 192, 3, 768, 12, 1, 197),
    "vit_small_patch16_224": (16, 384, 6, 1536, 12, 1, 197),
    "deit_small_patch16_224": (16, 384, 6, 1536, 12, 1, 197),
    "deit_base_patch16_224": (16, 768, 12, 3072, 12, 1, 197),
    "vit_large_patch16_224": (16, 1024, 16, 4096, 24, 1, 197),
    "vit_small_patch32_224": (32, 384, 6, 1536, 12, 1, 50),
    "vit_base_patch32_224": (32, 768, 12, 3072, 12, 1, 50),
    "vit_large_patch32_224": (32, 1024, 16, 4096, 24, 1, 50),
    "deit_tiny_distilled_patch16_224": (16, 192, 3, 768, 12, 2, 198),
    "deit_small_distilled_patch16_224": (16, 384, 6, 1536, 12, 2, 198),
    "deit_base_distilled_patch16_224": (16, 768, 12, 3072, 12, 2, 198),
}
NAMES = sorted(TABLE)
BLOCK_KEYS = ("norm1.weight", "norm1.bias", "attn.qkv.weight", "attn.qkv.bias", "attn.proj.weight", "attn.proj.bias", "norm2.weight",
              "norm2.bias", "mlp.fc1.weight", "mlp.fc1.bias", "mlp.fc2.weight", "mlp.fc2.bias")


def test_one_prefix_restatement_equals_the_vit_b16_restatement_exactly():
    spec = graphs.build_tiny(graphs.VIT_NAME, (64, 64))
    sd = weights.synthetic_state_dict(spec, 0)
    x = _rand(3, 3, 64, 64, seed=1)
    old, new = VitReference(spec, sd, [2, 5]), VitFamilyReference(spec, sd, [2, 5])
    fo, fn = old.forward(x), new.forward(x)
    assert all(a.dtype == torch.float64 and torch.equal(a, b) for a, b in zip(fo, fn))
    hg = [_rand(*f.shape, seed=2 + i) for i, f in enumerate(fo)]
    assert torch.equal(old.backward(hg), new.backward(hg))


def test_distilled_form_is_the_one_prefix_model_on_a_sequence_one_row_longer():
    """[cls; dist; patches] + pos_embed (tokens + 1 rows): with `dist_token` + its `pos_embed` row equal to an extra patch row's embedding,
    the distilled model is the one-prefix model's blocks run on the one-prefix sequence with that row inserted behind cls."""
    one = graphs.build_tiny(graphs.VIT_NAME, (64, 64))
    two = graphs.build_tiny("deit_base_distilled_patch16_224", (64, 64))
    assert (one.n_prefix, one.tokens, two.n_prefix, two.tokens) == (1, 17, 2, 18)
    sd = {k: v.double() for k, v in weights.synthetic_state_dict(one, 4).items()}
    x = _rand(2, 3, 64, 64, seed=5)
    extra_patch, extra_pos = _rand(1, 3, 16, 16, seed=6), _rand(1, 1, 64, seed=7) * 0.02
    e = fam.patch_rows(extra_patch, sd, one)                                     # (1, 1, 64): the extra patch row's embedding
    t1 = fam.embed(x, sd, one)
    longer = torch.cat([t1[:, :1], (e + extra_pos).expand(2, 1, 64), t1[:, 1:]], 1)
    want = fam.run_blocks(longer, sd, one, [2, 5])
    pos = sd["pos_embed"]
    sd2 = dict(sd, dist_token=e.reshape(1, 1, 64), pos_embed=torch.cat([pos[:, :1], extra_pos, pos[:, 1:]], 1))
    got = VitFamilyReference(two, sd2, [2, 5]).forward(x)
    for g, w in zip(got, want):
        assert g.shape == (2, 18 * 64)
        assert float((g - w.reshape(2, -1)).abs().max()) <= 1e-12 * float(w.abs().max())
    # and the dist row is row 1: moving it elsewhere is another model
    swapped = VitFamilyReference(two, dict(sd2, cls_token=sd2["dist_token"], dist_token=sd2["cls_token"]), [2]).forward(x)[0]
    assert float((swapped - got[0]).abs().max()) > 1e-6


@pytest.mark.parametrize("name", NAMES)
def test_spec_tokens_and_hooks_of_every_name(name):
    patch, dim, heads, mlp, blocks, n_prefix, tokens = TABLE[name]
    spec = graphs.build(name)
    assert isinstance(spec, graphs.VitSpec) and spec.arch == name
    assert (spec.img, spec.patch, spec.in_chans, spec.dim, spec.heads, spec.mlp, spec.blocks, spec.n_prefix) == \
        (224, patch, 3, dim, heads, mlp, blocks, n_prefix)
    assert spec.tokens == tokens == n_prefix + (224 // patch) ** 2
    assert spec.dim // spec.heads == 64 and spec.ln_eps == 1e-6
    want = {1: 2, 2: 5, 3: 8, 4: 11} if blocks == 12 else {1: 5, 2: 11, 3: 17, 4: 23}
    assert {d: spec.hook_for(d) for d in (1, 2, 3, 4)} == want == {d: d * blocks // 4 - 1 for d in (1, 2, 3, 4)}
    assert spec.hook_for(3, whole_module=True) == want[3]
    with pytest.raises(KeyError):
        spec.hook_for(5)
    assert graphs.vit_named(name, (224, 224)) == spec and graphs.build(name, (224, 224)) == spec


@pytest.mark.parametrize("name", NAMES)
def test_key_manifest_and_shapes_of_every_name(name):
    patch, dim, heads, mlp, blocks, n_prefix, tokens = TABLE[name]
    shapes = graphs.build(name).param_shapes()
    keys = ["patch_embed.proj.weight", "patch_embed.proj.bias", "cls_token"] + (["dist_token"] if n_prefix == 2 else []) + ["pos_embed"]
    keys += [f"blocks.{i}.{k}" for i in range(blocks) for k in BLOCK_KEYS]
    assert list(shapes) == keys
    assert shapes["patch_embed.proj.weight"] == (dim, 3, patch, patch) and shapes["patch_embed.proj.bias"] == (dim,)
    assert shapes["cls_token"] == (1, 1, dim) and shapes["pos_embed"] == (1, tokens, dim)
    assert ("dist_token" in shapes) == (n_prefix == 2) and shapes.get("dist_token", (1, 1, dim)) == (1, 1, dim)
    per_block = [(dim,), (dim,), (3 * dim, dim), (3 * dim,), (dim, dim), (dim,), (dim,), (dim,), (mlp, dim), (mlp,), (dim, mlp), (dim,)]
    for i in (0, blocks // 2, blocks - 1):
        assert [shapes[f"blocks.{i}.{k}"] for k in BLOCK_KEYS] == per_block
    assert not any(k.startswith(("norm.", "head.", "head_dist.")) for k in shapes)


def _checkpoint(spec):
    """A checkpoint of the spec's shapes that costs no memory on disk: every tensor is one zero expanded to its shape."""
    sd = {k: torch.zeros(1).expand(shp) for k, shp in spec.param_shapes().items()}
    sd.update({"norm.weight": torch.ones(spec.dim), "norm.bias": torch.zeros(spec.dim), "head.weight": torch.zeros(1000, spec.dim),
               "head.bias": torch.zeros(1000)})
    if spec.n_prefix == 2:
        sd.update({"head_dist.weight": torch.zeros(1000, spec.dim), "head_dist.bias": torch.zeros(1000)})
    return sd


@pytest.mark.parametrize("name", NAMES)
def test_checkpoint_of_every_name_loads_from_its_own_file(name, tmp_path, monkeypatch):
    spec = graphs.build(name)
    monkeypatch.delenv("I2V_SYNTHETIC_WEIGHTS", raising=False)
    monkeypatch.setenv("I2V_WEIGHTS_DIR", str(tmp_path))
    with pytest.raises(weights.MissingWeights, match=name):
        weights.load_state_dict(spec)
    sd = _checkpoint(spec)
    sd["cls_token"] = torch.full((1, 1, spec.dim), 0.25)
    torch.save(sd, tmp_path / f"{name}.pth")
    got = weights.load_state_dict(spec)
    assert list(got) == list(spec.param_shapes())
    assert all(tuple(got[k].shape) == shp and got[k].is_contiguous() for k, shp in spec.param_shapes().items())
    assert float(got["cls_token"].mean()) == 0.25
    # a model of the same shape under another name reads its own file, not this one
    twin = [n for n in NAMES + [graphs.VIT_NAME] if n != name and graphs.VIT_MODELS[n] == graphs.VIT_MODELS[name]]
    for n in twin:
        with pytest.raises(weights.MissingWeights, match=n):
            weights.load_state_dict(graphs.build(n))


@pytest.mark.parametrize("name", [n for n in NAMES if TABLE[n][5] == 2])
def test_missing_or_misshaped_dist_token_is_refused_by_name(name, tmp_path, monkeypatch):
    spec = graphs.build(name)
    monkeypatch.setenv("I2V_WEIGHTS_DIR", str(tmp_path))
    sd = _checkpoint(spec)
    del sd["dist_token"]
    torch.save(sd, tmp_path / f"{name}.pth")
    with pytest.raises(KeyError, match="dist_token"):
        weights.load_state_dict(spec)
    torch.save(dict(sd, dist_token=torch.zeros(1, 2, spec.dim)), tmp_path / f"{name}.pth")
    with pytest.raises(ValueError, match="dist_token"):
        weights.load_state_dict(spec)
    # the undistilled checkpoint's pos_embed (197 rows) under a distilled name is refused by name as well
    torch.save(dict(sd, dist_token=torch.zeros(1, 1, spec.dim), pos_embed=torch.zeros(1, 197, spec.dim)), tmp_path / f"{name}.pth")
    with pytest.raises(ValueError, match="pos_embed"):
        weights.load_state_dict(spec)


def test_synthetic_weights_of_every_layout_under_the_opt_in_only(monkeypatch, tmp_path):
    monkeypatch.setenv("I2V_WEIGHTS_DIR", str(tmp_path))
    monkeypatch.delenv("I2V_SYNTHETIC_WEIGHTS", raising=False)
    for name in ("deit_tiny_distilled_patch16_224", "vit_small_patch32_224"):
        spec = graphs.build(name)
        with pytest.raises(weights.MissingWeights):
            weights.load_state_dict(spec)
        sd = weights.load_state_dict(spec, seed=3)
        assert {k: tuple(v.shape) for k, v in sd.items()} == spec.param_shapes()
        assert all(torch.equal(sd[k], v) for k, v in weights.synthetic_state_dict(spec, 3).items())
        assert 0 < float(sd["pos_embed"].std()) < 0.05
    d = weights.synthetic_state_dict(graphs.build("deit_tiny_distilled_patch16_224"), 3)
    assert not torch.equal(d["dist_token"], d["cls_token"])


def test_refusals_name_the_reason_and_list_the_served_names():
    for name, why in (("vit_base_patch16_384", "384"), ("vit_base_patch32_384", "384"), ("deit_base_distilled_patch16_384", "384"),
                      ("vit_base_patch16_224_in21k", "in21k"), ("vit_base_r50_s16_224", "hybrid"), ("vit_small_r26_s32_224", "hybrid"),
                      ("vit_huge_patch14_224", "not a model"), ("deit_medium_patch16_224", "not a model")):
        with pytest.raises(ValueError, match=why) as ei:
            graphs.build(name)
        assert all(n in str(ei.value) for n in NAMES + [graphs.VIT_NAME])
        with pytest.raises(ValueError):
            graphs.vit_named(name)
        with pytest.raises(ValueError):
            graphs.build_tiny(name)
    for name in NAMES:
        for hw in ((384, 384), (112, 112), (224, 192)):
            with pytest.raises(ValueError, match="224 x 224"):
                graphs.build(name, hw)
    with pytest.raises(UnboundLocalError):            # a name outside the ViT vocabulary ends as it always did
        graphs.build("transformer")


def test_vit_base_patch16_224_builds_to_the_same_spec_as_before():
    spec = graphs.build(graphs.VIT_NAME)
    assert spec == graphs.vit() == graphs.vit((224, 224)) == graphs.vit_named(graphs.VIT_NAME)
    assert (spec.arch, spec.img, spec.patch, spec.in_chans, spec.dim, spec.heads, spec.mlp, spec.blocks, spec.ln_eps, spec.n_prefix,
            spec.tokens, spec.video) == ("vit_base_patch16_224", 224, 16, 3, 768, 12, 3072, 12, 1e-6, 1, 197, False)
    assert spec.hooks == {1: 2, 2: 5, 3: 8, 4: 11}
    assert list(spec.param_shapes())[:5] == ["patch_embed.proj.weight", "patch_embed.proj.bias", "cls_token", "pos_embed",
                                             "blocks.0.norm1.weight"]
    assert len(spec.param_shapes()) == 4 + 12 * 12
    assert graphs.VIT_MODELS[graphs.VIT_NAME] == (16, 768, 12, 3072, 12, 1) and set(graphs.VIT_MODELS) == set(NAMES) | {graphs.VIT_NAME}
    assert {n: graphs.VIT_MODELS[n] for n in NAMES} == {n: TABLE[n][:6] for n in NAMES}


def test_test_size_twins_are_kept_apart_from_timms_vit_tiny():
    plain, dist, p32 = (graphs.build_tiny(n, (64, 64)) for n in (graphs.VIT_NAME, "deit_small_distilled_patch16_224", "vit_base_patch32_224"))
    assert (plain.arch, dist.arch, p32.arch) == ("vit_tiny", "vit_tiny_distilled", "vit_tiny_patch32")
    assert (plain.tokens, dist.tokens, p32.tokens) == (17, 18, 5) and (dist.n_prefix, p32.patch) == (2, 32)
    for s in (plain, dist, p32):
        assert (s.dim, s.heads, s.mlp, s.blocks, s.hooks) == (64, 2, 256, 6, {1: 2, 2: 5})
    assert graphs.build_tiny("vit_tiny_patch16_224", (64, 64)) == plain           # a plain patch-16 name: the plain twin
    timm_tiny = graphs.build("vit_tiny_patch16_224")
    assert timm_tiny.arch != plain.arch and (timm_tiny.dim, timm_tiny.blocks) == (192, 12)
    assert "dist_token" in dist.param_shapes() and dist.param_shapes()["pos_embed"] == (1, 18, 64)
    assert p32.param_shapes()["patch_embed.proj.weight"] == (64, 3, 32, 32)
    with pytest.raises(ValueError):
        graphs.build_tiny("vit_base_patch32_224", (48, 48))
    sd = weights.synthetic_state_dict(p32, 0)
    f = VitFamilyReference(p32, sd, [2, 5]).forward(torch.randn(2, 3, 64, 64))
    assert [tuple(t.shape) for t in f] == [(2, 5 * 64)] * 2


def test_attack_classes_and_the_cli_take_the_names(tmp_path, monkeypatch):
    for name in NAMES:
        atk = attacks.ImageGuidedFMDirection_Adam([name], depth=4, step_size=0.005, steps=2, weight_seed=0)
        assert atk.model_names == [name]
    attacks.ImageGuidedStd_Adam(["vit_large_patch16_224"], depth=1, step_size=0.005, weight_seed=0)
    attacks.ImageGuidedFML2_Adam_MultiModels(["resnet", "deit_base_distilled_patch16_224", "vit_small_patch32_224"],
                                             depths={"resnet": 2, "deit_base_distilled_patch16_224": 3, "vit_small_patch32_224": 1},
                                             weight_seed=0)
    attacks.AENS_I2V_MF(["vit_tiny_patch16_224", "vgg"], depths={"vit_tiny_patch16_224": [2, 4], "vgg": [2, 3]}, step_size=0.005,
                        weight_seed=0)
    with pytest.raises(KeyError):
        attacks.ImageGuidedFMDirection_Adam(["vit_large_patch32_224"], depth=5, step_size=0.005, weight_seed=0)
    with pytest.raises(ValueError, match="384"):
        attacks.ImageGuidedFMDirection_Adam(["vit_base_patch16_384"], depth=2, step_size=0.005, weight_seed=0)
    import image_main
    monkeypatch.setattr(image_main, "OPT_PATH", str(tmp_path))
    base = ["--attack_method", "ImageGuidedFMDirection_Adam", "--step", "2"]
    a = image_main.arg_parse(base + ["--direction_image_model", "vit_large_patch16_224", "--depth", "4"])
    assert image_main.build_attack(a).model_names == ["vit_large_patch16_224"]
    for bad in (["--direction_image_model", "vit_base_patch16_384"], ["--direction_image_model", "vit_small_patch16_224", "--depth", "5"],
                ["--direction_image_model", "deit_base_patch16_224", "--hw", "112"]):
        with pytest.raises(SystemExit):
            image_main.arg_parse(base + bad)


def test_planned_bytes_are_counted_in_64_bits():
    """`VitSpec.workspace_bytes` restates the native plan (the GPU suite holds it to `i2v_vit_workspace_bytes`); the largest net is far
    beyond 32 bits and its per-frame, per-block saves are what DESIGN.md section 13 states for ViT-B (7.3 MB)."""
    big = graphs.build("vit_large_patch16_224")
    total = big.workspace_bytes([5, 11, 17, 23], 128)
    assert 2 ** 34 < total < 2 ** 36
    b = graphs.build(graphs.VIT_NAME)
    per = (b.workspace_bytes([11], 3) - b.workspace_bytes([11], 2)) - (b.workspace_bytes([10], 3) - b.workspace_bytes([10], 2))
    assert abs(per / 1e6 - 7.3) < 0.05


def test_new_native_symbols_are_exported_and_the_host_simulation_still_loads():
    import __graft_entry__ as ge
    new = ("i2v_vit_create_ex", "i2v_vit_embed_ex_f32", "i2v_vit_embed_bwd_ex_f32")
    assert all(n in _lib.VIT_EXPORTS for n in new)
    cd = C.CDLL(ge.LIB)
    assert all(hasattr(cd, n) for n in _lib.VIT_EXPORTS)
    assert not set(_lib.VIT_EXPORTS) & set(_lib.EXPORTS)
    hs = C.CDLL(os.path.join(ROOT, "tests", "hostsim", "libi2v_hostsim.so"))
    _lib.bind(hs)
    assert hs.i2v_backend() == b"hostsim"
