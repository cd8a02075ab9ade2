"""Plain-torch restatement of the Swin surrogates -- the yardstick of the Swin tests.  Written from the model's
definition (timm 0.5.0 `SwinTransformer`, `swin_*_patch4_window7_224`), parametrised by the spec alone and independent of the HIP path:
the bias index and the shift mask are built here by the roll / slice / broadcast construction, where the native code and
`graphs.SwinSpec` use closed formulas.

What the spec says: `img`, `patch`, `dim`, `window`, `depths`, `heads`, `ln_eps`.  A frame becomes an (img / patch)^2 grid of tokens by a
patch x patch convolution with stride patch, then LayerNorm; no class token, no position embedding.  Stage i: `depths[i]` blocks at
width dim * 2^i; patch merging behind every stage but the last.  Even blocks of a stage are unshifted, odd ones shifted by window // 2;
where the grid is not larger than the window the window is the grid and nothing is shifted.

`SwinReference` has the interface of `oracle.restate.OracleNet` that `oracle.restate.run_attack` drives: `.dtype`, `.hooks`,
`.forward(x) -> [hook features]` and `.backward(hook_grads) -> d cost / d x`; a hook feature is (frames, grid_i^2 * width_i), the stream
after the last block of stage i, before that stage's patch merging."""
from typing import Sequence

import torch
import torch.nn.functional as F

from tests.family_harness import StreamsReference
from tests.vit_family_reference import gelu, layer_norm


def relative_position_index(ws: int) -> torch.Tensor:
    """(ws^2, ws^2): pairwise coordinate differences, shifted to start at 0, the row difference scaled by 2 ws - 1."""
    coords = torch.stack(torch.meshgrid(torch.arange(ws), torch.arange(ws), indexing="ij")).flatten(1)      # (2, ws^2)
    rel = (coords[:, :, None] - coords[:, None, :]).permute(1, 2, 0).contiguous()                               # (ws^2, ws^2, 2)
    rel[:, :, 0] += ws - 1
    rel[:, :, 1] += ws - 1
    rel[:, :, 0] *= 2 * ws - 1
    return rel.sum(-1)


def window_partition(x, ws: int):
    """(N, H, W, C) -> (N * windows, ws * ws, C), windows in row-major order."""
    N, H, W, C = x.shape
    x = x.reshape(N, H // ws, ws, W // ws, ws, C)
    return x.permute(0, 1, 3, 2, 4, 5).reshape(-1, ws * ws, C)


def window_reverse(w, ws: int, H: int, W: int):
    N = w.shape[0] // ((H // ws) * (W // ws))
    x = w.reshape(N, H // ws, W // ws, ws, ws, -1)
    return x.permute(0, 1, 3, 2, 4, 5).reshape(N, H, W, -1)


def shift_mask(H: int, W: int, ws: int, shift: int, dtype=torch.float64) -> torch.Tensor:
    """(windows, ws^2, ws^2): an image of region numbers filled slice by slice, cut into windows, compared pairwise."""
    img = torch.zeros(1, H, W, 1, dtype=dtype)
    cnt = 0
    for hs in (slice(0, -ws), slice(-ws, -shift), slice(-shift, None)):
        for wsl in (slice(0, -ws), slice(-ws, -shift), slice(-shift, None)):
            img[:, hs, wsl, :] = cnt
            cnt += 1
    mw = window_partition(img, ws).reshape(-1, ws * ws)
    diff = mw[:, None, :] - mw[:, :, None]
    return torch.where(diff != 0, torch.full_like(diff, -100.0), torch.zeros_like(diff))


def window_attention(qkv, H: int, W: int, ws: int, shift: int, heads: int, table):
    """The attention core on qkv (N, H * W, 3 C), C = heads * dh, rows [q; k; v], with its roll, partition, bias, mask and roll back:
    (N, H * W, C).  table: ((2 ws - 1)^2, heads)."""
    N, T, C3 = qkv.shape
    C = C3 // 3
    dh = C // heads
    g = qkv.reshape(N, H, W, C3)
    if shift:
        g = torch.roll(g, shifts=(-shift, -shift), dims=(1, 2))
    w = window_partition(g, ws)                                                   # (B, ws^2, 3C)
    B, n = w.shape[0], ws * ws
    q, k, v = w.reshape(B, n, 3, heads, dh).permute(2, 0, 3, 1, 4)                # (B, heads, n, dh) each
    att = (q * dh ** -0.5) @ k.transpose(-2, -1)
    bias = table[relative_position_index(ws).reshape(-1).to(table.device)].reshape(n, n, heads).permute(2, 0, 1)
    att = att + bias.unsqueeze(0)
    if shift:
        m = shift_mask(H, W, ws, shift, qkv.dtype).to(qkv.device)
        att = (att.reshape(B // m.shape[0], m.shape[0], heads, n, n) + m[None, :, None]).reshape(B, heads, n, n)
    o = (torch.softmax(att, -1) @ v).transpose(1, 2).reshape(B, n, C)
    o = window_reverse(o, ws, H, W)
    if shift:
        o = torch.roll(o, shifts=(shift, shift), dims=(1, 2))
    return o.reshape(N, T, C)


def patch_merge_gather(x, H: int, W: int):
    """(N, H * W, C) -> (N, H/2 * W/2, 4C): the cell's tokens in the order (0,0), (1,0), (0,1), (1,1) as (row, column) offsets."""
    N, T, C = x.shape
    g = x.reshape(N, H, W, C)
    return torch.cat([g[:, 0::2, 0::2], g[:, 1::2, 0::2], g[:, 0::2, 1::2], g[:, 1::2, 1::2]], -1).reshape(N, T // 4, 4 * C)


def embed(x, sd, spec):
    p = F.conv2d(x, sd["patch_embed.proj.weight"], sd["patch_embed.proj.bias"], stride=spec.patch).flatten(2).transpose(1, 2)
    return layer_norm(p, sd["patch_embed.norm.weight"], sd["patch_embed.norm.bias"], spec.ln_eps)


def block(x, sd, spec, i: int, j: int, shift=None, zero_bias: bool = False):
    k = f"layers.{i}.blocks.{j}."
    g, D, heads = spec.grid(i), spec.width(i), spec.heads[i]
    ws = min(spec.window, g)
    if shift is None:
        shift = spec.window // 2 if (j % 2 == 1 and g > spec.window) else 0
    a = layer_norm(x, sd[k + "norm1.weight"], sd[k + "norm1.bias"], spec.ln_eps)
    qkv = a @ sd[k + "attn.qkv.weight"].T + sd[k + "attn.qkv.bias"]
    table = sd[k + "attn.relative_position_bias_table"]
    o = window_attention(qkv, g, g, ws, shift, heads, torch.zeros_like(table) if zero_bias else table)
    x = x + (o @ sd[k + "attn.proj.weight"].T + sd[k + "attn.proj.bias"])
    c = layer_norm(x, sd[k + "norm2.weight"], sd[k + "norm2.bias"], spec.ln_eps)
    h = gelu(c @ sd[k + "mlp.fc1.weight"].T + sd[k + "mlp.fc1.bias"])
    return x + (h @ sd[k + "mlp.fc2.weight"].T + sd[k + "mlp.fc2.bias"])


def merge(x, sd, spec, i: int):
    p = f"layers.{i}.downsample."
    m = patch_merge_gather(x, spec.grid(i), spec.grid(i))
    return layer_norm(m, sd[p + "norm.weight"], sd[p + "norm.bias"], spec.ln_eps) @ sd[p + "reduction.weight"].T


def run_stages(t, sd, spec, hook_stages: Sequence[int]):
    outs = {}
    for i in range(max(hook_stages) + 1):
        for j in range(spec.depths[i]):
            t = block(t, sd, spec, i, j)
        outs[i] = t
        if i < max(hook_stages):
            t = merge(t, sd, spec, i)
    return [outs[s] for s in hook_stages]


def streams(x, sd, spec, n_stages):
    """The streams behind the stages 0 .. n_stages - 1 (the hooks of this family number stages), each before its patch merging."""
    return run_stages(embed(x, sd, spec), sd, spec, list(range(n_stages)))


class SwinReference(StreamsReference):
    streams = staticmethod(streams)
