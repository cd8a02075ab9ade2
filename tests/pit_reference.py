"""timm 0.5.0's `PoolingVisionTransformer` up to its last block, written from the model description in plain torch on the CPU (DESIGN.md
section 29; restated from the architecture, UNCHECKED against timm): the float64 reference of the PiT tests, and the float64 / float32
restatement of the three new kernels.  Written from the description, not from i2v_amd.graphs: the patch embedding and the pooling are
`conv2d` calls on (frames, C, g, g) planes, the position table is added to the plane before the tokens are flattened, the prefix tokens
are concatenated in front -- so that the packing of `PitSpec.native_arrays` (the token-major position table with zero prefix rows, the
(2 C, 9) filter) and the token-major kernels are tested, not assumed.

  embed      x = patch_embed.conv: conv2d(kernel patch, stride stride, padding 0) -> (C, g, g);  x = x + pos_embed;  tokens = flatten;
             cls_token (1, prefix, C) in front
  block      x = x + proj(attn(LN1 x));  x = x + fc2(gelu(fc1(LN2 x)));  LayerNorm eps 1e-6, exact GELU
  attn       qkv = Linear(x) split (3, heads, dh);  softmax(q k^T dh^-0.5) v
  pool       behind stages 0 and 1: grid tokens back to (C, g, g), conv2d(C -> 2 C, kernel 3, stride 2, padding 1, groups C), flattened;
             prefix tokens through the Linear pool.fc
`norm`, `head` and `head_dist` lie behind every hook and are not restated.
"""
import torch
import torch.nn.functional as F

from tests.family_harness import StreamsReference


def attn_core(qkv, heads):
    """Plain attention between the Linears: qkv (frames, T, 3 heads dh) -> (frames, T, heads dh)."""
    n, T, C3 = qkv.shape
    C = C3 // 3
    dh = C // heads
    q, k, v = qkv.reshape(n, T, 3, heads, dh).permute(2, 0, 3, 1, 4).unbind(0)
    attn = (q @ k.transpose(-2, -1)) * dh ** -0.5
    return (attn.softmax(dim=-1) @ v).transpose(1, 2).reshape(n, T, C)


def pool_tokens(x, w, b, g, prefix):
    """The pooling convolution on token-major rows: x (frames, prefix + g^2, C), w (2 C, 1, 3, 3) -> the pooled GRID rows
    (frames, go^2, 2 C)."""
    n, _, C = x.shape
    plane = x[:, prefix:].transpose(1, 2).reshape(n, C, g, g)
    y = F.conv2d(plane, w, b, stride=2, padding=1, groups=C)
    return y.flatten(2).transpose(1, 2)


def patch_rows(img, p, s):
    """Overlapping patch rows: img (frames, C, side, side) -> (frames g^2, C p^2), column (c p + dy) p + dx (F.unfold's order)."""
    n, C = img.shape[:2]
    cols = F.unfold(img, kernel_size=p, stride=s)                          # frames, C p^2, g^2
    return cols.transpose(1, 2).reshape(-1, C * p * p)


def block(x, sd, p, heads, eps):
    D = x.shape[-1]
    t = F.layer_norm(x, (D,), sd[p + "norm1.weight"], sd[p + "norm1.bias"], eps)
    a = attn_core(F.linear(t, sd[p + "attn.qkv.weight"], sd[p + "attn.qkv.bias"]), heads)
    x = x + F.linear(a, sd[p + "attn.proj.weight"], sd[p + "attn.proj.bias"])
    t = F.layer_norm(x, (D,), sd[p + "norm2.weight"], sd[p + "norm2.bias"], eps)
    return x + F.linear(F.gelu(F.linear(t, sd[p + "mlp.fc1.weight"], sd[p + "mlp.fc1.bias"])), sd[p + "mlp.fc2.weight"], sd[p + "mlp.fc2.bias"])


def streams(x, sd, spec, n_blocks, skip=()):
    """The residual streams after the flat blocks 0 .. n_blocks - 1, each (frames, tokens of its stage, width of its stage)."""
    n = x.shape[0]
    x = F.conv2d(x, sd["patch_embed.conv.weight"], sd["patch_embed.conv.bias"], stride=spec.stride)
    g = x.shape[-1]
    if "pos" not in skip:
        x = x + sd["pos_embed"]
    cls = sd["cls_token"]
    if "swap" in skip:
        cls = cls.flip(1)
    x = torch.cat((cls.expand(n, -1, -1), x.flatten(2).transpose(1, 2)), dim=1)
    prefix = cls.shape[1]
    outs, done = [], 0
    for st in range(3):
        for j in range(spec.depths[st]):
            if done == n_blocks:
                return outs
            x = block(x, sd, f"transformers.{st}.blocks.{j}.", spec.heads[st], spec.ln_eps)
            outs.append(x)
            done += 1
        if st < 2 and done < n_blocks:
            p = f"transformers.{st}.pool."
            w = sd[p + "conv.weight"]
            if "pool" in skip:
                w = torch.zeros_like(w)
            grid = pool_tokens(x, w, sd[p + "conv.bias"], g, prefix)
            x = torch.cat((F.linear(x[:, :prefix], sd[p + "fc.weight"], sd[p + "fc.bias"]), grid), dim=1)
            g = (g - 1) // 2 + 1
    return outs


#: `skip` names what the sensitivity checks leave out: "pos" (no position table), "pool" (a pool filter of zeros), "swap" (the two
#: prefix tokens exchanged).
class PitReference(StreamsReference):
    streams = staticmethod(streams)
