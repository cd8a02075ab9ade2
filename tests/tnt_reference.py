"""timm 0.5.0's `TNT` (Transformer in Transformer) up to its last block, written from the model description in plain torch on the CPU
(restated from memory of tnt.py, UNCHECKED against timm): the float64 reference of the TNT tests, and the float64 /
float32 restatement of the new kernels.  Written from the description, not from i2v_amd.graphs and without a call into product code: the
pixel embedding is a `conv2d` and an `unfold`, qk and v are separate Linears, the heads are split off with reshapes -- so that the packing
of `TntSpec.native_arrays` (qk stacked on v, the padded filter rows, pixel_pos pixel-major) and the kernels' layouts are tested, not assumed.

  pixels     conv2d(3 -> in_dim, 7, stride 4, padding 3) | unfold(4, 4): patch n = g py + px, pixel p = 4 i + j at conv output
             (4 py + i, 4 px + j) | + pixel_pos (1, in_dim, 4, 4) | inner (frames g^2, 16, in_dim)
  patches    norm2_proj(proj(norm1_proj(inner as (frames, g^2, 16 in_dim)))), columns p in_dim + c | cls_token in front | + patch_pos
  block      inner += attn_in(norm_in inner); inner += mlp_in(norm_mlp_in inner);
             outer[:, 1:] += proj(norm1_proj(inner) as (frames, g^2, 16 in_dim)), norm1_proj over in_dim;
             outer += attn_out(norm_out outer); outer += mlp(norm_mlp outer)
  attention  qk = Linear(dim, 2 dim) without bias, split (2, heads, dh); v = Linear(dim, dim) without bias; softmax(dh^-0.5 q k^T) v; proj
`norm` and `head` lie behind every hook and are not restated.
"""
import torch
import torch.nn.functional as F

from tests.family_harness import StreamsReference


def attention_core(qkv, heads):
    """qkv (seqs, T, 3 heads dh) in the kernel's layout -> softmax(dh^-0.5 q k^T) v as (seqs, T, heads dh)."""
    n, T, C3 = qkv.shape
    dh = C3 // 3 // heads
    q, k, v = qkv.reshape(n, T, 3, heads, dh).permute(2, 0, 3, 1, 4).unbind(0)
    p = ((q @ k.transpose(-2, -1)) * dh ** -0.5).softmax(dim=-1)
    return (p @ v).transpose(1, 2).reshape(n, T, heads * dh)


def pixel_rows(x):
    """The rows of the 7 x 7, stride 4, padding 3 convolution in (patch, pixel) order: x (frames, C, side, side) ->
    (frames g^2 16, C 49), column c 49 + ky 7 + kx."""
    n, C, side, _ = x.shape
    g = side // 16
    cols = F.unfold(x, 7, padding=3, stride=4)                             # (n, C 49, (4 g)^2), position oy 4 g + ox
    cols = cols.reshape(n, C * 49, g, 4, g, 4).permute(0, 2, 4, 3, 5, 1)   # (n, py, px, i, j, C 49)
    return cols.reshape(n * g * g * 16, C * 49)


def attention(x, sd, p, heads):
    n, T, D = x.shape
    dh = D // heads
    qk = F.linear(x, sd[p + "qk.weight"]).reshape(n, T, 2, heads, dh).permute(2, 0, 3, 1, 4)
    v = F.linear(x, sd[p + "v.weight"]).reshape(n, T, heads, dh).transpose(1, 2)
    a = ((qk[0] @ qk[1].transpose(-2, -1)) * dh ** -0.5).softmax(dim=-1)
    return F.linear((a @ v).transpose(1, 2).reshape(n, T, D), sd[p + "proj.weight"], sd[p + "proj.bias"])


def half(x, sd, p, norm, attn, norm_mlp, mlp, heads, eps):
    D = x.shape[-1]
    x = x + attention(F.layer_norm(x, (D,), sd[p + norm + ".weight"], sd[p + norm + ".bias"], eps), sd, p + attn + ".", heads)
    t = F.layer_norm(x, (D,), sd[p + norm_mlp + ".weight"], sd[p + norm_mlp + ".bias"], eps)
    return x + F.linear(F.gelu(F.linear(t, sd[p + mlp + ".fc1.weight"], sd[p + mlp + ".fc1.bias"])), sd[p + mlp + ".fc2.weight"], sd[p + mlp + ".fc2.bias"])


def streams(x, sd, spec, n_blocks, skip=()):
    """The outer residual streams behind the blocks 0 .. n_blocks - 1, each (frames, 1 + g^2, dim)."""
    n, d, D, eps = x.shape[0], spec.in_dim, spec.dim, spec.ln_eps
    y = F.conv2d(x, sd["pixel_embed.proj.weight"], sd["pixel_embed.proj.bias"], stride=4, padding=3)
    g = y.shape[-1] // 4
    y = F.unfold(y, 4, stride=4)                                           # (n, d 16, g^2), row c 16 + 4 i + j
    y = y.transpose(1, 2).reshape(n * g * g, d, 4, 4)
    if "pixel_pos" not in skip:
        y = y + sd["pixel_pos"]
    inner = y.reshape(n * g * g, d, 16).transpose(1, 2)                    # (n g^2, 16, d)
    patch = F.layer_norm(inner.reshape(n, g * g, 16 * d), (16 * d,), sd["norm1_proj.weight"], sd["norm1_proj.bias"], eps)
    patch = F.layer_norm(F.linear(patch, sd["proj.weight"], sd["proj.bias"]), (D,), sd["norm2_proj.weight"], sd["norm2_proj.bias"], eps)
    outer = torch.cat((sd["cls_token"].expand(n, -1, -1), patch), dim=1) + sd["patch_pos"]
    outs = []
    for i in range(n_blocks):
        p = f"blocks.{i}."
        if "inner" not in skip:
            inner = half(inner, sd, p, "norm_in", "attn_in", "norm_mlp_in", "mlp_in", spec.in_heads, eps)
        t = F.layer_norm(inner, (d,), sd[p + "norm1_proj.weight"], sd[p + "norm1_proj.bias"], eps).reshape(n, g * g, 16 * d)
        outer = torch.cat((outer[:, :1], outer[:, 1:] + F.linear(t, sd[p + "proj.weight"], sd[p + "proj.bias"])), dim=1)
        outer = half(outer, sd, p, "norm_out", "attn_out", "norm_mlp", "mlp", spec.heads, eps)
        outs.append(outer)
    return outs


#: `skip` names what the sensitivity checks leave out: "inner" (no inner transformer: the pixel tokens reach every block's proj as
#: embedded), "pixel_pos" (no pixel position table).
class TntReference(StreamsReference):
    streams = staticmethod(streams)
