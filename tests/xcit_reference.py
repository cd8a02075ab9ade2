"""timm 0.5.0's `XCiT` up to its last cross-covariance block, written from the architecture definition in plain torch on the CPU (DESIGN.md
section 23): the float64 reference of the XCiT tests.  Token-major (frames, tokens, dim) as timm computes it, and with timm's LITERAL
arithmetic -- every BatchNorm is a separate eval-mode `batch_norm`, the position features go through their 1 x 1 convolution at run time,
the three LayerScales multiply their branch's output, q and k are normalised BEFORE the product -- so that the folds of
`XcitSpec.native_arrays` are tested, not assumed.

  stem       four conv 3 x 3 / 2 / pad 1 without bias, each + BatchNorm2d (eval, eps 1e-5), GELU (erf) after the first three; flatten to
             (tokens, dim); + token_projection(Fourier features of the grid)
  Fourier    y = cumsum of ones down the rows, x along the columns (1 .. grid); each / (last + 1e-6) * 2 pi; dim_t = 10000^(2 (i // 2) / 32);
             pos = coordinate / dim_t; sin of the even features and cos of the odd ones, interleaved; y features, then x features
  block      x = x + gamma1 * proj(XCA(LN1 x));  x = x + gamma3 * LPI(LN3 x);  x = x + gamma2 * fc2(gelu(fc1(LN2 x)));  LayerNorm eps 1e-6
  XCA        q, k, v = qkv(x) split (3, heads, dh), transposed to (dh, tokens); q, k = normalize(., dim = tokens) (eps 1e-12);
             attn = softmax((q @ k^T) * temperature);  out = (attn @ v) back to (tokens, heads dh)
  LPI        on the (grid, grid) plane: conv1 depthwise 3 x 3 pad 1 with bias, GELU, BatchNorm2d (eval), conv2 depthwise 3 x 3 pad 1 with bias
The class-attention blocks, `cls_token`, `norm` and `head` lie behind every hook and are not restated.
"""
import math

import torch
import torch.nn.functional as F

from tests.family_harness import StreamsReference

BN_EPS = 1e-5


def fourier(grid: int, dtype=torch.float64, hidden: int = 32, temperature: float = 10000.0):
    """timm's `PositionalEncodingFourier.forward` before `token_projection`, as timm builds it -> (1, 2 hidden, grid, grid)."""
    ones = torch.ones(1, grid, grid, dtype=dtype)
    y_embed, x_embed = ones.cumsum(1), ones.cumsum(2)
    eps, scale = 1e-6, 2 * math.pi
    y_embed = y_embed / (y_embed[:, -1:, :] + eps) * scale
    x_embed = x_embed / (x_embed[:, :, -1:] + eps) * scale
    dim_t = torch.arange(hidden, dtype=dtype)
    dim_t = temperature ** (2 * torch.div(dim_t, 2, rounding_mode="floor") / hidden)
    pos_x = x_embed[:, :, :, None] / dim_t
    pos_y = y_embed[:, :, :, None] / dim_t
    pos_x = torch.stack([pos_x[:, :, :, 0::2].sin(), pos_x[:, :, :, 1::2].cos()], dim=4).flatten(3)
    pos_y = torch.stack([pos_y[:, :, :, 0::2].sin(), pos_y[:, :, :, 1::2].cos()], dim=4).flatten(3)
    return torch.cat((pos_y, pos_x), dim=3).permute(0, 3, 1, 2)


def _bn(x, sd, p):
    return F.batch_norm(x, sd[p + "running_mean"], sd[p + "running_var"], sd[p + "weight"], sd[p + "bias"], False, 0.0, BN_EPS)


def stem(x, sd, spec, skip=()):
    for k in range(4):
        p = f"patch_embed.proj.{2 * k}."
        x = F.conv2d(x, sd[p + "0.weight"], None, stride=2, padding=1)
        if "stem_bn" not in skip:
            x = _bn(x, sd, p + "1.")
        if k < 3:
            x = F.gelu(x)
    t = x.flatten(2).transpose(1, 2)
    if "pos" in skip:
        return t
    pos = F.conv2d(fourier(spec.grid, x.dtype).to(x.device), sd["pos_embeder.token_projection.weight"], sd["pos_embeder.token_projection.bias"])
    return t + pos.flatten(2).transpose(1, 2)


def xca_core(qkv, heads, temperature):
    """timm's `XCA.forward` between its two Linears, on qkv (frames, T, 3 heads dh), temperature (heads) or (heads, 1, 1) ->
    (out (frames, T, heads dh), attn (frames, heads, dh, dh))."""
    n, T, C3 = qkv.shape
    dh = C3 // (3 * heads)
    q, k, v = qkv.reshape(n, T, 3, heads, dh).permute(2, 0, 3, 1, 4).unbind(0)
    q, k, v = q.transpose(-2, -1), k.transpose(-2, -1), v.transpose(-2, -1)
    q = F.normalize(q, dim=-1)
    k = F.normalize(k, dim=-1)
    attn = ((q @ k.transpose(-2, -1)) * temperature.reshape(1, heads, 1, 1)).softmax(dim=-1)
    return (attn @ v).permute(0, 3, 1, 2).reshape(n, T, heads * dh), attn


def lpi(t, sd, p, grid, skip=()):
    n, T, D = t.shape
    x = t.permute(0, 2, 1).reshape(n, D, grid, grid)
    x = F.gelu(F.conv2d(x, sd[p + "conv1.weight"], sd[p + "conv1.bias"], padding=1, groups=D))
    if "lpi_bn" not in skip:
        x = _bn(x, sd, p + "bn.")
    x = F.conv2d(x, sd[p + "conv2.weight"], sd[p + "conv2.bias"], padding=1, groups=D)
    return x.reshape(n, D, T).permute(0, 2, 1)


def block(x, sd, spec, i: int, skip=()):
    p = f"blocks.{i}."
    D = x.shape[-1]
    one = torch.ones(D, dtype=x.dtype, device=x.device)
    g1, g2, g3 = (one if n in skip else sd[p + n] for n in ("gamma1", "gamma2", "gamma3"))
    temp = torch.ones_like(sd[p + "attn.temperature"]) if "temperature" in skip else sd[p + "attn.temperature"]
    t = F.layer_norm(x, (D,), sd[p + "norm1.weight"], sd[p + "norm1.bias"], spec.ln_eps)
    a, _ = xca_core(F.linear(t, sd[p + "attn.qkv.weight"], sd[p + "attn.qkv.bias"]), spec.heads, temp)
    x = x + g1 * F.linear(a, sd[p + "attn.proj.weight"], sd[p + "attn.proj.bias"])
    t = F.layer_norm(x, (D,), sd[p + "norm3.weight"], sd[p + "norm3.bias"], spec.ln_eps)
    x = x + g3 * lpi(t, sd, p + "local_mp.", spec.grid, skip)
    t = F.layer_norm(x, (D,), sd[p + "norm2.weight"], sd[p + "norm2.bias"], spec.ln_eps)
    return x + g2 * F.linear(F.gelu(F.linear(t, sd[p + "mlp.fc1.weight"], sd[p + "mlp.fc1.bias"])), sd[p + "mlp.fc2.weight"], sd[p + "mlp.fc2.bias"])


def streams(x, sd, spec, n_blocks, skip=()):
    """The residual streams behind the blocks 0 .. n_blocks - 1, each (frames, tokens, dim)."""
    t, outs = stem(x, sd, spec, skip), []
    for i in range(n_blocks):
        t = block(t, sd, spec, i, skip)
        outs.append(t)
    return outs


#: `skip` names what the sensitivity checks leave out, one fold each: "stem_bn", "pos", "gamma1", "gamma2", "gamma3", "lpi_bn",
#: "temperature" (a BatchNorm skipped, a LayerScale or temperature of one).
class XcitReference(StreamsReference):
    streams = staticmethod(streams)
