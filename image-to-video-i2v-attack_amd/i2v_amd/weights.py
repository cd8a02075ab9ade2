"""Backbone weights in torchvision `state_dict` layout.

The reference downloads ImageNet checkpoints with `models.<arch>(pretrained=True)`
(`/root/reference/image_attacks.py:88-101`).  There is no network here, so the default is a
seeded synthetic initialiser: Kaiming-normal(fan_out) convolutions and
randomised BatchNorm statistics, so that BN folding is actually exercised.  A real checkpoint
(`torch.save(model.state_dict())` of the torchvision model) is picked up from
`$I2V_WEIGHTS_DIR/<arch>.pth` when present; without one the synthetic initialiser must be asked
for explicitly (`load_state_dict`).
"""
import os
import zlib
from typing import Dict

import torch

from .graphs import BeitSpec, CaitSpec, CoatSpec, ConvitSpec, ConvNextSpec, Graph, MixerSpec, PitSpec, SwinSpec, TntSpec, TwinsSpec, VitSpec, XcitSpec

BN_EPS = 1e-5   # torchvision BatchNorm2d default, used by every ResNet BN


def _gen(seed: int, key: str) -> torch.Generator:
    """One generator per parameter, keyed by its state_dict name: the values do not depend on
    the order in which the graph lists its nodes."""
    g = torch.Generator(device="cpu")
    g.manual_seed((seed * 1000003 + zlib.crc32(key.encode())) % (2 ** 63))
    return g


def _vit_synthetic(spec: VitSpec, seed: int) -> Dict[str, torch.Tensor]:
    """Seeded stand-in for a trained ViT, drawn per key like the CNN initialiser: truncated-normal-like (clamped at 2 std) matrices of
    std 0.02 as timm initialises them, except qkv at 0.05 so that the attention logits reach O(1) and the softmax is not uniform;
    LayerNorm gains near 1; small biases.  The residual stream stays O(1) through the 12 blocks (the tests check the hooks)."""
    sd = {}
    for k, shp in spec.param_shapes().items():
        g = _gen(seed, k)
        if k.endswith("norm1.weight") or k.endswith("norm2.weight"):
            sd[k] = 1.0 + 0.1 * torch.randn(*shp, generator=g)
        elif k.endswith("bias"):
            sd[k] = 0.02 * torch.randn(*shp, generator=g)
        else:
            std = 0.05 if k.endswith("attn.qkv.weight") else 0.02
            sd[k] = torch.randn(*shp, generator=g).clamp_(-2.0, 2.0) * std
    return sd


def _swin_synthetic(spec: SwinSpec, seed: int) -> Dict[str, torch.Tensor]:
    """Seeded stand-in for a trained Swin, drawn per key: matrices of std 0.02 clamped at 2 std as timm initialises them, except qkv at
    width^-0.5, which puts the attention logits at O(1) at every stage's width (96 .. 1536), and the relative-position bias table at
    std 0.5, so that the bias visibly shapes the softmax; LayerNorm gains near 1; small biases.  Each block then adds a few tenths to a
    unit-variance stream, which stays O(1) through swin_small's 24 blocks (the tests check the hooks' spread)."""
    sd = {}
    for k, shp in spec.param_shapes().items():
        g = _gen(seed, k)
        if k.endswith("relative_position_bias_table"):
            sd[k] = torch.randn(*shp, generator=g).clamp_(-2.0, 2.0) * 0.5
        elif k.endswith(("norm1.weight", "norm2.weight", "norm.weight")):
            sd[k] = 1.0 + 0.1 * torch.randn(*shp, generator=g)
        elif k.endswith("bias"):
            sd[k] = 0.02 * torch.randn(*shp, generator=g)
        else:
            std = shp[1] ** -0.5 if k.endswith("attn.qkv.weight") else 0.02
            sd[k] = torch.randn(*shp, generator=g).clamp_(-2.0, 2.0) * std
    return sd


def _convnext_synthetic(spec: ConvNextSpec, seed: int) -> Dict[str, torch.Tensor]:
    """Seeded stand-in for a trained ConvNeXt, drawn per key: the stem and downsample convolutions at fan_in^-0.5 (a unit-variance
    stream stays one), depthwise filters at 1 / 7 (49 taps of unit inputs give unit outputs), fc1 at fan_in^-0.5 and fc2 at
    0.5 fan_in^-0.5, LayerNorm gains near 1, small biases, and `gamma` spread over 0.1 .. 0.5 with random signs -- far from the ones a
    forgotten fold would use.  Each block then adds a few tenths to its stream, which stays O(1) through 36 blocks."""
    sd = {}
    for k, shp in spec.param_shapes().items():
        g = _gen(seed, k)
        if k.endswith("gamma"):
            sd[k] = (0.1 + 0.4 * torch.rand(*shp, generator=g)) * (torch.randint(0, 2, shp, generator=g).float() * 2 - 1)
        elif k.endswith(("norm.weight", "stem.1.weight", "downsample.0.weight")):
            sd[k] = 1.0 + 0.1 * torch.randn(*shp, generator=g)
        elif k.endswith("bias"):
            sd[k] = 0.02 * torch.randn(*shp, generator=g)
        elif k.endswith("conv_dw.weight"):
            sd[k] = torch.randn(*shp, generator=g) / 7.0
        else:
            fan_in = 1
            for v in shp[1:]:
                fan_in *= v
            sd[k] = torch.randn(*shp, generator=g) * ((0.5 if k.endswith("fc2.weight") else 1.0) * fan_in ** -0.5)
    return sd


def _mixer_synthetic(spec: MixerSpec, seed: int) -> Dict[str, torch.Tensor]:
    """Seeded stand-in for a trained MLP-Mixer / ResMLP, drawn per key: Linears (the stem as one) at fan_in^-0.5, the second Linear of
    an MLP at 0.5 fan_in^-0.5, LayerNorm gains near 1, small biases.  ResMLP's `ls1` / `ls2` are spread over 0.1 .. 0.4 with random
    signs, `alpha` over 0.5 .. 1.5 and `beta` ~ 0.3 N(0, 1): far from timm's initial 1e-4 / 1 / 0 and from the ones and zeros a
    forgotten fold would use."""
    sd = {}
    for k, shp in spec.param_shapes().items():
        g = _gen(seed, k)
        if k.endswith((".ls1", ".ls2")):
            sd[k] = (0.1 + 0.3 * torch.rand(*shp, generator=g)) * (torch.randint(0, 2, shp, generator=g).float() * 2 - 1)
        elif k.endswith(".alpha"):
            sd[k] = 0.5 + torch.rand(*shp, generator=g)
        elif k.endswith(".beta"):
            sd[k] = 0.3 * torch.randn(*shp, generator=g)
        elif k.endswith(("norm1.weight", "norm2.weight")):
            sd[k] = 1.0 + 0.1 * torch.randn(*shp, generator=g)
        elif k.endswith("bias"):
            sd[k] = 0.02 * torch.randn(*shp, generator=g)
        else:
            fan_in = 1
            for v in shp[1:]:
                fan_in *= v
            sd[k] = torch.randn(*shp, generator=g) * ((0.5 if k.endswith("fc2.weight") else 1.0) * fan_in ** -0.5)
    return sd


def _cait_synthetic(spec: CaitSpec, seed: int) -> Dict[str, torch.Tensor]:
    """Seeded stand-in for a trained CaiT, drawn per key so that every piece of the block's arithmetic shows in the hooks: Linears (the
    patch embedding as one) ~ fan_in^-0.5 N(0, 1), which keeps a unit-variance stream and puts the attention logits at O(1); `attn.proj`
    and `mlp.fc2` at half that; LayerNorm gains 1 + 0.1 N(0, 1); biases 0.02 N(0, 1); pos_embed 0.5 N(0, 1).  The LayerScale vectors
    `gamma_1` / `gamma_2` are uniform on [0.5, 1] with random signs -- timm initialises them at 1e-5 or 1e-6, which would make every
    block an identity and the tests blind to the kernel.  The talking-heads mixes `attn.proj_l.weight` / `attn.proj_w.weight` are the
    identity plus 0.25 N(0, 1) per entry, with `proj_l.bias` ~ 0.5 N(0, 1) and `proj_w.bias` ~ 0.02 N(0, 1): far from the identity and
    the zeros a skipped mix would compute."""
    sd = {}
    for k, shp in spec.param_shapes().items():
        g = _gen(seed, k)
        if k.endswith((".gamma_1", ".gamma_2")):
            sd[k] = (0.5 + 0.5 * torch.rand(*shp, generator=g)) * (torch.randint(0, 2, shp, generator=g).float() * 2 - 1)
        elif k.endswith(("proj_l.weight", "proj_w.weight")):
            sd[k] = torch.eye(shp[0]) + 0.25 * torch.randn(*shp, generator=g)
        elif k.endswith("proj_l.bias"):
            sd[k] = 0.5 * torch.randn(*shp, generator=g)
        elif k == "pos_embed":
            sd[k] = 0.5 * torch.randn(*shp, generator=g)
        elif k.endswith(("norm1.weight", "norm2.weight")):
            sd[k] = 1.0 + 0.1 * torch.randn(*shp, generator=g)
        elif k.endswith("bias"):
            sd[k] = 0.02 * torch.randn(*shp, generator=g)
        else:
            fan_in = 1
            for v in shp[1:]:
                fan_in *= v
            sd[k] = torch.randn(*shp, generator=g) * ((0.5 if k.endswith(("fc2.weight", "attn.proj.weight")) else 1.0) * fan_in ** -0.5)
    return sd


def _convit_synthetic(spec: ConvitSpec, seed: int) -> Dict[str, torch.Tensor]:
    """Seeded stand-in for a trained ConViT, drawn per key as `_cait_synthetic` draws: Linears ~ fan_in^-0.5 N(0, 1) (`attn.proj` and
    `mlp.fc2` at half that), LayerNorm gains 1 + 0.1 N(0, 1), biases 0.02 N(0, 1), pos_embed and cls_token 0.5 N(0, 1).  `attn.v` is an
    ordinary Linear draw, not timm's identity.  `attn.pos_proj.weight` is timm's local initialisation -- column 2 = -1, and columns 0 /
    1 on the head's offset in a floor(sqrt(heads)) grid: head p = h1 + k h2 gets column 1 = 2 (h1 - centre) and column 0 = 2 (h2 -
    centre) -- plus seeded noise, 0.3 N(0, 1) on the two offset columns and 0.1 N(0, 1) on the distance column, so that the x and y
    columns of every head differ and a transposed grid convention shows.  `attn.gating_param` ~ N(0, 1), so sigma(g) spans the range
    (timm starts it at 1); `attn.pos_proj.bias` ~ 0.5 N(0, 1), far from the zero a dropped bias would equal."""
    sd = {}
    for k, shp in spec.param_shapes().items():
        g = _gen(seed, k)
        if k.endswith("pos_proj.weight"):
            H = shp[0]
            ks = int(H ** 0.5)
            centre = (ks - 1) / 2 if ks % 2 == 0 else ks // 2
            w = torch.zeros(H, 3)
            for h1 in range(ks):
                for h2 in range(ks):
                    w[h1 + ks * h2] = torch.tensor([2.0 * (h2 - centre), 2.0 * (h1 - centre), -1.0])
            sd[k] = w + torch.randn(H, 3, generator=g) * torch.tensor([0.3, 0.3, 0.1])
        elif k.endswith("gating_param"):
            sd[k] = torch.randn(*shp, generator=g)
        elif k.endswith("pos_proj.bias"):
            sd[k] = 0.5 * torch.randn(*shp, generator=g)
        elif k in ("pos_embed", "cls_token"):
            sd[k] = 0.5 * torch.randn(*shp, generator=g)
        elif k.endswith(("norm1.weight", "norm2.weight")):
            sd[k] = 1.0 + 0.1 * torch.randn(*shp, generator=g)
        elif k.endswith("bias"):
            sd[k] = 0.02 * torch.randn(*shp, generator=g)
        else:
            fan_in = 1
            for v in shp[1:]:
                fan_in *= v
            sd[k] = torch.randn(*shp, generator=g) * ((0.5 if k.endswith(("fc2.weight", "attn.proj.weight")) else 1.0) * fan_in ** -0.5)
    return sd


def _xcit_synthetic(spec: XcitSpec, seed: int) -> Dict[str, torch.Tensor]:
    """Seeded stand-in for a trained XCiT, drawn per key as `_cait_synthetic` draws: Linears and convolutions ~ fan_in^-0.5 N(0, 1)
    (`attn.proj` and `mlp.fc2` at half that), LayerNorm gains 1 + 0.1 N(0, 1), biases 0.02 N(0, 1) -- the depthwise convolutions' 0.1
    N(0, 1), so that a dropped bias shows --, BatchNorm gains uniform on (0.5, 1.5), shifts and running means 0.1 N(0, 1), running
    variances uniform on (0.5, 1.5).  The LayerScales gamma1 / gamma2 / gamma3 are uniform on (0.5, 1.5) -- timm starts them at 1 (or
    1e-5 for the 24-block models) and they train away from it --, each drawn on its own so that exchanging two of them shows;
    `attn.temperature` is uniform on (0.5, 4), so that the softmax over channels is neither flat nor one-hot."""
    sd = {}
    for k, shp in spec.param_shapes().items():
        g = _gen(seed, k)
        if k.endswith(("gamma1", "gamma2", "gamma3", "running_var")) or ".bn.weight" in k or (k.startswith("patch_embed") and k.endswith("1.weight")):
            sd[k] = 0.5 + torch.rand(*shp, generator=g)
        elif k.endswith("temperature"):
            sd[k] = 0.5 + 3.5 * torch.rand(*shp, generator=g)
        elif k.endswith("running_mean") or ".bn.bias" in k or (k.startswith("patch_embed") and k.endswith("1.bias")):
            sd[k] = 0.1 * torch.randn(*shp, generator=g)
        elif k.endswith(("norm1.weight", "norm2.weight", "norm3.weight")):
            sd[k] = 1.0 + 0.1 * torch.randn(*shp, generator=g)
        elif k.endswith(("conv1.bias", "conv2.bias")):
            sd[k] = 0.1 * torch.randn(*shp, generator=g)
        elif k.endswith("bias"):
            sd[k] = 0.02 * torch.randn(*shp, generator=g)
        else:
            fan_in = 1
            for v in shp[1:]:
                fan_in *= v
            sd[k] = torch.randn(*shp, generator=g) * ((0.5 if k.endswith(("fc2.weight", "attn.proj.weight")) else 1.0) * fan_in ** -0.5)
    return sd


def _twins_synthetic(spec: TwinsSpec, seed: int) -> Dict[str, torch.Tensor]:
    """Seeded stand-in for a trained Twins, drawn per key as `_xcit_synthetic` draws: Linears and the patch and sub-sampling
    convolutions ~ fan_in^-0.5 N(0, 1) (`attn.proj` and `mlp.fc2` at half that), the blocks' LayerNorm gains 1 + 0.1 N(0, 1), biases
    0.02 N(0, 1).  What is new shows: `attn.norm` and the patch embeddings' norms have gains uniform on (0.5, 1.5) and shifts 0.1
    N(0, 1), so that a sub-sampled plane that skipped its LayerNorm is seen; `attn.sr.bias` is 0.1 N(0, 1); the position encoding's
    depthwise filter is N(0, 1) / 3 with a bias of 0.1 N(0, 1), so that its term is of the size of the stream it is added to."""
    sd = {}
    for k, shp in spec.param_shapes().items():
        g = _gen(seed, k)
        if k.endswith("attn.norm.weight") or (k.startswith("patch_embeds") and k.endswith("norm.weight")):
            sd[k] = 0.5 + torch.rand(*shp, generator=g)
        elif k.endswith("attn.norm.bias") or (k.startswith("patch_embeds") and k.endswith("norm.bias")) or k.endswith("attn.sr.bias") \
                or (k.startswith("pos_block") and k.endswith("bias")):
            sd[k] = 0.1 * torch.randn(*shp, generator=g)
        elif k.startswith("pos_block"):
            sd[k] = torch.randn(*shp, generator=g) / 3.0
        elif k.endswith(("norm1.weight", "norm2.weight")):
            sd[k] = 1.0 + 0.1 * torch.randn(*shp, generator=g)
        elif k.endswith("bias"):
            sd[k] = 0.02 * torch.randn(*shp, generator=g)
        else:
            fan_in = 1
            for v in shp[1:]:
                fan_in *= v
            sd[k] = torch.randn(*shp, generator=g) * ((0.5 if k.endswith(("fc2.weight", "attn.proj.weight")) else 1.0) * fan_in ** -0.5)
    return sd


def _beit_synthetic(spec: BeitSpec, seed: int) -> Dict[str, torch.Tensor]:
    """Seeded stand-in for a trained BEiT, drawn per key as `_twins_synthetic` draws: Linears and the patch convolution ~ fan_in^-0.5
    N(0, 1) (`attn.proj` and `mlp.fc2` at half that), LayerNorm gains 1 + 0.1 N(0, 1), biases 0.02 N(0, 1), `cls_token` 0.02 N(0, 1).
    timm's initial values would blind the tests -- a zero bias table makes the bias a no-op, a LayerScale of 0.1 or 1e-5 silences the
    blocks -- so what is new shows: `relative_position_bias_table` is N(0, 1), `gamma_1` / `gamma_2` are uniform on (0.5, 1.5), and
    `q_bias` / `v_bias` are 0.1 N(0, 1).  The index buffers are not emitted: they are computed from the geometry."""
    sd = {}
    for k, shp in spec.param_shapes().items():
        g = _gen(seed, k)
        if k.endswith(("gamma_1", "gamma_2")):
            sd[k] = 0.5 + torch.rand(*shp, generator=g)
        elif k.endswith("relative_position_bias_table"):
            sd[k] = torch.randn(*shp, generator=g)
        elif k.endswith(("q_bias", "v_bias")):
            sd[k] = 0.1 * torch.randn(*shp, generator=g)
        elif k.endswith(("norm1.weight", "norm2.weight")):
            sd[k] = 1.0 + 0.1 * torch.randn(*shp, generator=g)
        elif k.endswith("bias") or k == "cls_token":
            sd[k] = 0.02 * torch.randn(*shp, generator=g)
        else:
            fan_in = 1
            for v in shp[1:]:
                fan_in *= v
            sd[k] = torch.randn(*shp, generator=g) * ((0.5 if k.endswith(("fc2.weight", "attn.proj.weight")) else 1.0) * fan_in ** -0.5)
    return sd


def _pit_synthetic(spec: PitSpec, seed: int) -> Dict[str, torch.Tensor]:
    """Seeded stand-in for a trained PiT, drawn per key as `_beit_synthetic` draws: Linears and the patch convolution ~ fan_in^-0.5
    N(0, 1) (`attn.proj` and `mlp.fc2` at half that), LayerNorm gains 1 + 0.1 N(0, 1), biases 0.02 N(0, 1).  What is new must show in the
    tests: `pos_embed` and `cls_token` are N(0, 1) (timm's 0.02 would leave the position table and the prefix tokens below the tests'
    bounds), and the pool filter `pool.conv.weight` is N(0, 1) / 3 over its 9 taps, so that a pooled token is of the size of its inputs."""
    sd = {}
    for k, shp in spec.param_shapes().items():
        g = _gen(seed, k)
        if k in ("pos_embed", "cls_token"):
            sd[k] = torch.randn(*shp, generator=g)
        elif k.endswith("pool.conv.weight"):
            sd[k] = torch.randn(*shp, generator=g) / 3.0
        elif k.endswith(("norm1.weight", "norm2.weight")):
            sd[k] = 1.0 + 0.1 * torch.randn(*shp, generator=g)
        elif k.endswith("bias"):
            sd[k] = 0.02 * torch.randn(*shp, generator=g)
        else:
            fan_in = 1
            for v in shp[1:]:
                fan_in *= v
            sd[k] = torch.randn(*shp, generator=g) * ((0.5 if k.endswith(("fc2.weight", "attn.proj.weight")) else 1.0) * fan_in ** -0.5)
    return sd


def _coat_synthetic(spec: CoatSpec, seed: int) -> Dict[str, torch.Tensor]:
    """Seeded stand-in for a trained CoaT-Lite, drawn per key as `_pit_synthetic` draws: Linears and the patch convolutions ~ fan_in^-0.5
    N(0, 1) (`factoratt_crpe.proj` and `mlp.fc2` at half that), LayerNorm gains 1 + 0.1 N(0, 1), biases 0.02 N(0, 1).  What is new must
    show in the tests: the class tokens are N(0, 1) and the filters of `cpe` and `crpe` N(0, 1) / window over their window^2 taps, so
    that each window moves the features."""
    sd = {}
    for k, shp in spec.param_shapes().items():
        g = _gen(seed, k)
        if k.startswith("cls_token"):
            sd[k] = torch.randn(*shp, generator=g)
        elif k.startswith(("cpe", "crpe")) and k.endswith("weight"):
            sd[k] = torch.randn(*shp, generator=g) / shp[-1]
        elif k.endswith(("norm1.weight", "norm2.weight", "norm.weight")):
            sd[k] = 1.0 + 0.1 * torch.randn(*shp, generator=g)
        elif k.endswith("bias"):
            sd[k] = 0.02 * torch.randn(*shp, generator=g)
        else:
            fan_in = 1
            for v in shp[1:]:
                fan_in *= v
            sd[k] = torch.randn(*shp, generator=g) * ((0.5 if k.endswith(("fc2.weight", "factoratt_crpe.proj.weight")) else 1.0) * fan_in ** -0.5)
    return sd


def _tnt_synthetic(spec: TntSpec, seed: int) -> Dict[str, torch.Tensor]:
    """Seeded stand-in for a trained TNT, drawn per key as `_coat_synthetic` draws: Linears and the pixel convolution ~ fan_in^-0.5
    N(0, 1) (every attention's `proj`, the step's `proj` and every `fc2` at half that), LayerNorm gains 1 + 0.1 N(0, 1), biases
    0.02 N(0, 1).  What is new must show in the tests: `cls_token` is N(0, 1) and the two position tables 0.5 N(0, 1), so that the
    pixel order inside a patch moves the features."""
    sd = {}
    for k, shp in spec.param_shapes().items():
        g = _gen(seed, k)
        if k == "cls_token":
            sd[k] = torch.randn(*shp, generator=g)
        elif k in ("patch_pos", "pixel_pos"):
            sd[k] = 0.5 * torch.randn(*shp, generator=g)
        elif "norm" in k and k.endswith("weight"):
            sd[k] = 1.0 + 0.1 * torch.randn(*shp, generator=g)
        elif k.endswith("bias"):
            sd[k] = 0.02 * torch.randn(*shp, generator=g)
        else:
            fan_in = 1
            for v in shp[1:]:
                fan_in *= v
            half = k.endswith(("fc2.weight", "proj.weight")) and not k.startswith("pixel_embed")
            sd[k] = torch.randn(*shp, generator=g) * ((0.5 if half else 1.0) * fan_in ** -0.5)
    return sd


def check_coat_duplicates(spec: CoatSpec, sd, where: str) -> None:
    """timm registers a stage's shared `cpe` and `crpe` again inside every serial block, so its checkpoints carry them under block-level
    keys too.  The stage-level keys are the ones loaded; a block-level duplicate that differs describes another model: refused by key
    name.  An absent one is fine."""
    for dup, key in spec.shared_duplicates().items():
        if dup in sd and not (tuple(sd[dup].shape) == tuple(sd[key].shape) and torch.equal(sd[dup].float(), sd[key].float())):
            raise ValueError(f"{where}: {dup} differs from the stage's shared {key}")


def check_beit_buffers(spec: BeitSpec, sd, where: str) -> None:
    """timm's BEiT checkpoints carry the buffer `attn.relative_position_index` per block; it is computed from the geometry here and
    never loaded, so one that differs describes another model: refused by key name.  An absent one is fine."""
    idx = spec.relative_position_index()
    for i in range(spec.blocks):
        k = spec.index_key(i)
        if k in sd and not (tuple(sd[k].shape) == tuple(idx.shape) and torch.equal(sd[k].long(), idx)):
            raise ValueError(f"{where}: buffer {k} differs from the index computed for a {spec.grid} x {spec.grid} grid")


#: timm renamed XCiT's `pos_embeder` to `pos_embed` after 0.5.0: the later spelling of the same two arrays is accepted
XCIT_KEY_ALIASES = {"pos_embed.token_projection.weight": "pos_embeder.token_projection.weight",
                    "pos_embed.token_projection.bias": "pos_embeder.token_projection.bias"}


def check_swin_buffers(spec: SwinSpec, sd, where: str) -> None:
    """timm's Swin checkpoints carry the buffers `relative_position_index` and `attn_mask`; they are computed from the geometry here
    and never loaded, so one that differs describes another model: refused by key name."""
    idx = spec.relative_position_index()
    for i in range(spec.stages):
        for j in range(spec.depths[i]):
            p = f"layers.{i}.blocks.{j}."
            k = p + "attn.relative_position_index"
            if k in sd and not (tuple(sd[k].shape) == tuple(idx.shape) and torch.equal(sd[k].long(), idx)):
                raise ValueError(f"{where}: buffer {k} differs from the index computed for window {spec.window}")
            k = p + "attn_mask"
            if k in sd and sd[k] is not None:
                if spec.shift(i, j) == 0:
                    raise ValueError(f"{where}: buffer {k} is a mask, but block {j} of stage {i} is not shifted")
                want = spec.attn_mask(i)
                if not (tuple(sd[k].shape) == tuple(want.shape) and torch.equal(sd[k].float(), want)):
                    raise ValueError(f"{where}: buffer {k} differs from the mask computed for a {spec.grid(i)} x {spec.grid(i)} grid, "
                                     f"window {spec.window}, shift {spec.shift(i, j)}")


def synthetic_state_dict(graph: Graph, seed: int = 0) -> Dict[str, torch.Tensor]:
    """Seeded stand-in for trained weights, one generator per key.  Convolutions: Kaiming-normal(fan_out); BatchNorms: randomised
    statistics.  Squeeze-and-excitation nodes (`{p}.se.fc1.*`, `{p}.se.fc2.*`) are drawn so that the gates are neither saturated nor
    flat: fc1.weight ~ N(0, 4 / C) (the squeezed pre-activations are O(1) for O(1/2) channel means), fc1.bias ~ 0.1 N(0, 1),
    fc2.weight ~ N(0, 1 / rd), and fc2.bias a random permutation of C points evenly spaced over [-2, 2]: the bias alone spreads the
    gates over sigmoid(-2) .. sigmoid(2) = 0.12 .. 0.88 whatever the input, and the fc2 term moves each gate with the frame."""
    if isinstance(graph, VitSpec):
        return _vit_synthetic(graph, seed)
    if isinstance(graph, SwinSpec):
        return _swin_synthetic(graph, seed)
    if isinstance(graph, ConvNextSpec):
        return _convnext_synthetic(graph, seed)
    if isinstance(graph, MixerSpec):
        return _mixer_synthetic(graph, seed)
    if isinstance(graph, CaitSpec):
        return _cait_synthetic(graph, seed)
    if isinstance(graph, ConvitSpec):
        return _convit_synthetic(graph, seed)
    if isinstance(graph, XcitSpec):
        return _xcit_synthetic(graph, seed)
    if isinstance(graph, TwinsSpec):
        return _twins_synthetic(graph, seed)
    if isinstance(graph, BeitSpec):
        return _beit_synthetic(graph, seed)
    if isinstance(graph, PitSpec):
        return _pit_synthetic(graph, seed)
    if isinstance(graph, CoatSpec):
        return _coat_synthetic(graph, seed)
    if isinstance(graph, TntSpec):
        return _tnt_synthetic(graph, seed)
    sd = {}
    for nd in graph.nodes:
        if nd.op == "se":
            k1, k2 = nd.fc1 + ".weight", nd.fc2 + ".weight"
            sd[k1] = torch.randn(nd.rd, nd.C, 1, 1, generator=_gen(seed, k1)) * (2.0 / nd.C ** 0.5)
            sd[nd.fc1 + ".bias"] = torch.randn(nd.rd, generator=_gen(seed, nd.fc1 + ".bias")) * 0.1
            sd[k2] = torch.randn(nd.C, nd.rd, 1, 1, generator=_gen(seed, k2)) * (1.0 / nd.rd ** 0.5)
            sd[nd.fc2 + ".bias"] = torch.linspace(-2.0, 2.0, nd.C)[torch.randperm(nd.C, generator=_gen(seed, nd.fc2 + ".bias"))].contiguous()
        if nd.op != "conv":
            continue
        fan_out = nd.cout * nd.kt * nd.kh * nd.kw
        std = (2.0 / fan_out) ** 0.5
        # Non-local blocks: gluoncv zero-initialises the BatchNorm behind W (the block starts as the identity) and a trained
        # block stays a correction to its input, with attention logits of moderate size.  Kaiming-sized theta / phi and a unit
        # BatchNorm make the un-normalised softmax one-hot and the whole network chaotic instead (two float32 evaluations of a
        # 4-step ILAF run then differ by percents): smaller embeddings, and a small BatchNorm gain below.
        nl = ".nonlocal_block." in nd.weight
        if nl and (".theta." in nd.weight or ".phi." in nd.weight):
            std *= 0.1
        shape = (nd.cout, nd.cin, nd.kt, nd.kh, nd.kw) if graph.video else (nd.cout, nd.cin // nd.groups, nd.kh, nd.kw)
        sd[nd.weight] = torch.randn(*shape, generator=_gen(seed, nd.weight)) * std
        if nd.bias:
            sd[nd.bias] = torch.randn(nd.cout, generator=_gen(seed, nd.bias)) * 0.05
        if nd.bn:
            g = _gen(seed, nd.bn)
            sd[nd.bn + ".weight"] = (torch.rand(nd.cout, generator=g) + 0.5) * (0.1 if nl else 1.0)
            sd[nd.bn + ".bias"] = torch.randn(nd.cout, generator=g) * 0.1
            sd[nd.bn + ".running_mean"] = torch.randn(nd.cout, generator=g) * 0.1
            sd[nd.bn + ".running_var"] = torch.rand(nd.cout, generator=g) + 0.5
        if nd.pre_bn:
            g = _gen(seed, nd.pre_bn)
            sd[nd.pre_bn + ".weight"] = torch.rand(nd.cin, generator=g) + 0.5
            sd[nd.pre_bn + ".bias"] = torch.randn(nd.cin, generator=g) * 0.1
            sd[nd.pre_bn + ".running_mean"] = torch.randn(nd.cin, generator=g) * 0.1
            sd[nd.pre_bn + ".running_var"] = torch.rand(nd.cin, generator=g) + 0.5
    return sd


class MissingWeights(FileNotFoundError):
    pass


#: classifier-head parameters (torchvision and gluoncv both name the last Linear `fc`); not part of any graph's
#: `param_shapes()`, kept next to the backbone's tensors whenever the checkpoint has them
HEAD_KEYS = ("fc.weight", "fc.bias")


#: arch -> where its weights came from in this process ("<path>" or "synthetic(seed=N)"); printed once per arch
SOURCES: Dict[str, str] = {}


def synthetic_allowed() -> bool:
    return os.environ.get("I2V_SYNTHETIC_WEIGHTS", "") not in ("", "0")


def load_state_dict(graph: Graph, seed=None, keep_head: bool = False) -> Dict[str, torch.Tensor]:
    """`$I2V_WEIGHTS_DIR/<arch>.pth` (a torchvision-layout `state_dict`; extra keys such as `layer4.*`, `fc.*`,
    `num_batches_tracked` are ignored; with `keep_head` the classifier's `fc.weight` / `fc.bias` are returned as well) when it exists.  Otherwise the seeded synthetic initialiser -- but only when
    the caller asked for it: an explicit integer `seed` (tests, bench) or `I2V_SYNTHETIC_WEIGHTS=1`.  The reference
    attacks ImageNet-pretrained backbones (`pretrained=True`, image_attacks.py:88-101); silently perturbing clips
    against random weights would produce valid-looking but meaningless `*-adv.npy` files, so that case raises."""
    root = os.environ.get("I2V_WEIGHTS_DIR", "")
    path = os.path.join(root, graph.arch + ".pth") if root else ""
    if path and os.path.exists(path):
        sd = torch.load(path, map_location="cpu", weights_only=True)
        if isinstance(sd, dict) and "state_dict" in sd and isinstance(sd["state_dict"], dict):
            sd = sd["state_dict"]
        shapes = graph.param_shapes()
        if isinstance(graph, XcitSpec):
            sd = dict(sd, **{new: sd[old] for old, new in XCIT_KEY_ALIASES.items() if old in sd and new not in sd})
        missing = [k for k in shapes if k not in sd]
        if missing:
            raise KeyError(f"{path}: missing keys {missing[:4]}...")
        if isinstance(graph, SwinSpec):
            check_swin_buffers(graph, sd, path)
        if isinstance(graph, BeitSpec):
            check_beit_buffers(graph, sd, path)
        if isinstance(graph, CoatSpec):
            check_coat_duplicates(graph, sd, path)
        for k, shp in shapes.items():
            if tuple(sd[k].shape) != tuple(shp):
                raise ValueError(f"{path}: {k} has shape {tuple(sd[k].shape)}, expected {shp}")
        _note(graph.arch, path)
        out = {k: sd[k].float().contiguous() for k in shapes}
        for k in HEAD_KEYS if keep_head else ():      # the classifier head travels with its backbone (video.VideoModel.head_weights)
            if k in sd:
                out[k] = sd[k].float().contiguous()
        return out
    explicit = seed is not None
    if seed is None:
        if not synthetic_allowed():
            raise MissingWeights(
                f"no pretrained weights for {graph.arch!r}: put the torchvision state_dict at "
                f"$I2V_WEIGHTS_DIR/{graph.arch}.pth (I2V_WEIGHTS_DIR={root!r}), or opt in to seeded SYNTHETIC weights "
                "with I2V_SYNTHETIC_WEIGHTS=1 / --synthetic_weights / an explicit weight_seed")
        seed = 0
    _note(graph.arch, f"synthetic(seed={seed})", warn=not explicit)
    return synthetic_state_dict(graph, seed)


def _note(arch: str, source: str, warn: bool = True):
    if SOURCES.get(arch) != source:
        SOURCES[arch] = source
        if source.startswith("synthetic") and warn and os.environ.get("I2V_QUIET_WEIGHTS", "") in ("", "0"):
            import sys
            print(f"[i2v_amd] WARNING: backbone {arch} runs on {source} weights, not an ImageNet checkpoint", file=sys.stderr)
        elif not source.startswith("synthetic"):
            print(f"[i2v_amd] backbone {arch}: weights from {source}")


def convert_gluoncv_state_dict(graph: Graph, sd: Dict[str, torch.Tensor], rules=None) -> Dict[str, torch.Tensor]:
    """Map a gluoncv-torch video checkpoint (the reference builds its white-box models with
    `gluoncv.torch.model_zoo.get_model(cfg)`, `image_fine_tune_attack.py:58-66`) onto the key layout of the video graph IR
    (`graphs.i3d_resnet` / `graphs.slowfast_res2`): unwraps `{'state_dict': ...}`, strips a DataParallel `module.` prefix,
    applies `rules` -- `(regex, replacement)` pairs, first match wins -- and then REQUIRES every parameter the graph reads
    to be present with the right shape.  Dropped: `num_batches_tracked`, and parameters of stages the graph does not
    contain at all (later stages when the graph stops at a hook).  The classifier head (`fc.*`) is kept.  NOT dropped:
    a checkpoint parameter that lives INSIDE a stage the graph builds but that the graph does not read (e.g. the
    `res_layers.1.*` non-local block of an `i3d_nl5` checkpoint offered to a plain I3D graph) -- the checkpoint then
    describes another network than the graph and loading it "successfully" would attack the wrong model: KeyError.

    The graph's own names follow the attributes the reference dereferences on those models (`res_layers`, `slow_res2`,
    `fast_res2`, `image_attacks.py:513-519`) and the Bottleneck layout of gluoncv's action-recognition ResNets
    (`conv1/bn1/conv2/bn2/conv3/bn3/downsample.{0,1}`), so the default rule set is the identity.  gluoncv is not
    installed and cannot be fetched here: the mapping is therefore UNPINNED against a real checkpoint -- which is why a
    key that does not land, or lands with another shape, is an error and never a silent re-initialisation."""
    import re
    if isinstance(sd, dict) and isinstance(sd.get("state_dict"), dict):
        sd = sd["state_dict"]
    rules = [(re.compile(a), b) for a, b in (rules or [])]
    renamed = {}
    for k, v in sd.items():
        k = k[len("module."):] if k.startswith("module.") else k
        for rx, rep in rules:
            if rx.search(k):
                k = rx.sub(rep, k)
                break
        renamed[k] = v
    out, missing, wrong = {}, [], []
    shapes = graph.param_shapes()
    for k, shp in shapes.items():
        if k not in renamed:
            missing.append(k)
        elif tuple(renamed[k].shape) != tuple(shp):
            wrong.append((k, tuple(renamed[k].shape), tuple(shp)))
        else:
            out[k] = renamed[k].float().contiguous()
    if missing or wrong:
        raise KeyError(f"checkpoint does not cover the {graph.arch} graph: {len(missing)} missing (e.g. {missing[:3]}), "
                       f"{len(wrong)} with another shape (e.g. {wrong[:2]}); pass `rules=[(regex, replacement), ...]` to rename")
    stages = {_stage(k) for k in shapes}
    unread = sorted(k for k in renamed if k not in shapes and k not in HEAD_KEYS and not k.endswith("num_batches_tracked")
                    and _stage(k) in stages)
    if unread:
        raise KeyError(f"checkpoint has {len(unread)} parameters inside stages the {graph.arch} graph builds but does not read "
                       f"(e.g. {unread[:3]}): it describes a different network (non-local blocks?) than this graph")
    for k in HEAD_KEYS:
        if k in renamed:
            out[k] = renamed[k].float().contiguous()
    return out


def _stage(key: str) -> str:
    """The stage a parameter belongs to: its first path component, plus the second when that is an index
    (`res_layers.1.0.conv1.weight` -> `res_layers.1`, `slow_res2.0.conv1.weight` -> `slow_res2`, `first_stage.conv1.weight`
    -> `first_stage`)."""
    parts = key.split(".")
    return ".".join(parts[:2]) if len(parts) > 2 and parts[1].isdigit() else parts[0]


def fold_affine(nd, sd):
    """Per-output-channel (scale, shift) such that the node computes
    `y = conv(x, W) * scale + shift` -- BatchNorm in eval mode
    (`image_attacks.py:253-256` freezes every BN) or the conv bias."""
    if nd.bn:
        g = sd[nd.bn + ".weight"].double()
        b = sd[nd.bn + ".bias"].double()
        m = sd[nd.bn + ".running_mean"].double()
        v = sd[nd.bn + ".running_var"].double()
        s = g / torch.sqrt(v + BN_EPS)
        t = b - m * s
        if nd.bias:                 # conv WITH bias followed by BatchNorm (the non-local block's W): BN(conv + bias)
            t = t + sd[nd.bias].double() * s
        return s.float(), t.float()
    s = torch.ones(nd.cout)
    t = sd[nd.bias].float() if nd.bias else torch.zeros(nd.cout)
    return s, t


def fold_pre_affine(nd, sd):
    """(scale, shift) of the eval-mode BatchNorm in FRONT of a pre-activation conv: the conv reads
    relu(x*scale + shift) (torchvision `_DenseLayer`: norm1 -> relu1 -> conv1)."""
    g = sd[nd.pre_bn + ".weight"].double()
    b = sd[nd.pre_bn + ".bias"].double()
    m = sd[nd.pre_bn + ".running_mean"].double()
    v = sd[nd.pre_bn + ".running_var"].double()
    s = g / torch.sqrt(v + BN_EPS)
    return s.float(), (b - m * s).float()
