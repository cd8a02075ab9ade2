"""CPU: the ViT surrogate's definition -- the plain-torch restatement pinned against torch's own
TransformerEncoderLayer, the depth -> block hook mapping, the timm key manifest, the refusals, and the native symbols."""
import ctypes as C
import os

import pytest
import torch

from i2v_amd import graphs, weights
from i2v_amd import lib as _lib
from tests.vit_reference import VitReference, block, embed

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VIT = graphs.VIT_NAME


def test_block_matches_torch_transformer_encoder_layer_in_float64():
    spec = graphs.build(VIT)
    sd = {k: v.double() for k, v in weights.synthetic_state_dict(spec, 0).items()}
    layer = torch.nn.TransformerEncoderLayer(768, 12, 3072, dropout=0.0, activation="gelu", layer_norm_eps=1e-6, norm_first=True,
                                             batch_first=True).double().eval()
    k = "blocks.4."
    with torch.no_grad():
        layer.norm1.weight.copy_(sd[k + "norm1.weight"]); layer.norm1.bias.copy_(sd[k + "norm1.bias"])
        layer.self_attn.in_proj_weight.copy_(sd[k + "attn.qkv.weight"])          # timm's qkv rows [q; k; v] are exactly this layout
        layer.self_attn.in_proj_bias.copy_(sd[k + "attn.qkv.bias"])
        layer.self_attn.out_proj.weight.copy_(sd[k + "attn.proj.weight"]); layer.self_attn.out_proj.bias.copy_(sd[k + "attn.proj.bias"])
        layer.norm2.weight.copy_(sd[k + "norm2.weight"]); layer.norm2.bias.copy_(sd[k + "norm2.bias"])
        layer.linear1.weight.copy_(sd[k + "mlp.fc1.weight"]); layer.linear1.bias.copy_(sd[k + "mlp.fc1.bias"])
        layer.linear2.weight.copy_(sd[k + "mlp.fc2.weight"]); layer.linear2.bias.copy_(sd[k + "mlp.fc2.bias"])
        x = torch.randn(2, 197, 768, dtype=torch.float64, generator=torch.Generator().manual_seed(0))
        ref = layer(x)
        ours = block(x, sd, spec, 4)
    assert float((ours - ref).abs().max() / ref.abs().max()) < 1e-12


def test_patch_embedding_is_the_strided_convolution_with_cls_and_pos():
    spec = graphs.build_tiny(VIT, (64, 64))
    sd = {k: v.double() for k, v in weights.synthetic_state_dict(spec, 1).items()}
    x = torch.randn(2, 3, 64, 64, dtype=torch.float64)
    t = embed(x, sd, spec)
    assert t.shape == (2, 17, 64)
    patch = x[:, :, 16:32, 32:48]                                  # patch (1, 2) -> token 1 + 1 * 4 + 2
    want = (sd["patch_embed.proj.weight"] * patch[:, None]).sum((2, 3, 4)) + sd["patch_embed.proj.bias"] + sd["pos_embed"][0, 7]
    assert torch.allclose(t[:, 7], want, atol=1e-12)
    assert torch.allclose(t[:, 0], (sd["cls_token"][0, 0] + sd["pos_embed"][0, 0]).expand(2, -1), atol=1e-15)


def test_depth_hooks_the_output_of_block_3d_minus_1():
    spec = graphs.build(VIT)
    assert {d: spec.hook_for(d) for d in (1, 2, 3, 4)} == {1: 2, 2: 5, 3: 8, 4: 11}
    assert spec.hook_for(2, whole_module=True) == 5
    with pytest.raises(KeyError):
        spec.hook_for(5)
    tiny = graphs.build_tiny(VIT)
    assert (tiny.dim, tiny.heads, tiny.blocks, tiny.mlp, tiny.tokens) == (64, 2, 6, 256, 17) and tiny.hooks == {1: 2, 2: 5}
    # the hook is the whole residual stream after the block, cls token included, flattened per frame
    sd = weights.synthetic_state_dict(tiny, 0)
    ref = VitReference(tiny, sd, [2, 5])
    f = ref.forward(torch.randn(3, 3, 64, 64))
    assert [tuple(t.shape) for t in f] == [(3, 17 * 64), (3, 17 * 64)]


def test_timm_key_manifest_and_shapes():
    shapes = graphs.build(VIT).param_shapes()
    assert len(shapes) == 4 + 12 * 12
    assert shapes["patch_embed.proj.weight"] == (768, 3, 16, 16) and shapes["cls_token"] == (1, 1, 768)
    assert shapes["pos_embed"] == (1, 197, 768)
    assert shapes["blocks.11.attn.qkv.weight"] == (2304, 768) and shapes["blocks.0.mlp.fc1.weight"] == (3072, 768)
    assert shapes["blocks.3.mlp.fc2.weight"] == (768, 3072) and shapes["blocks.7.norm2.bias"] == (768,)
    assert not any(k.startswith(("norm.", "head.")) for k in shapes)


def test_only_224_frames_are_accepted():
    graphs.build(VIT, (224, 224))
    for hw in ((112, 112), (256, 256), (224, 192)):
        with pytest.raises(ValueError, match="224 x 224"):
            graphs.build(VIT, hw)


def test_weights_from_the_directory_and_the_synthetic_opt_in(tmp_path, monkeypatch):
    spec = graphs.build_tiny(VIT)
    monkeypatch.delenv("I2V_SYNTHETIC_WEIGHTS", raising=False)
    monkeypatch.setenv("I2V_WEIGHTS_DIR", str(tmp_path))
    with pytest.raises(weights.MissingWeights):
        weights.load_state_dict(spec)
    sd = weights.synthetic_state_dict(spec, 3)
    full = dict(sd, **{"norm.weight": torch.ones(64), "norm.bias": torch.zeros(64), "head.weight": torch.zeros(1000, 64),
                       "head.bias": torch.zeros(1000)})
    torch.save(full, tmp_path / f"{spec.arch}.pth")
    got = weights.load_state_dict(spec)
    assert set(got) == set(spec.param_shapes()) and all(torch.equal(got[k], sd[k]) for k in got)
    assert torch.equal(weights.load_state_dict(spec, seed=3)["pos_embed"], sd["pos_embed"])   # the file wins over a seed


def test_vit_symbols_in_the_library_and_the_host_simulation_still_loads():
    import __graft_entry__ as ge
    cd = C.CDLL(ge.LIB)
    assert all(hasattr(cd, n) for n in _lib.VIT_EXPORTS)
    assert not set(_lib.VIT_EXPORTS) & set(_lib.EXPORTS)
    hs = C.CDLL(os.path.join(ROOT, "tests", "hostsim", "libi2v_hostsim.so"))
    _lib.bind(hs)
    assert hs.i2v_backend() == b"hostsim"
