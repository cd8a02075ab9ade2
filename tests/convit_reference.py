"""timm 0.5.0's `ConViT` up to its last block, written from the architecture definition in plain torch on the CPU:
the float64 reference of the ConViT tests.  Token-major (frames, tokens, dim) as timm computes it, and with timm's LITERAL arithmetic: the
positional scores keep `pos_proj.bias`, the blended attention is divided by its row sum, and `attn.qk` / `attn.v` are separate Linears --
so that the folds of `ConvitSpec.native_arrays` (no bias, no division, one stacked qkv) are tested, not assumed.

  stem                    conv patch x patch / patch with bias, flattened to (tokens, dim), + pos_embed; no cls_token in the stream yet
  Block                   x = x + attn(LN1(x));  x = x + mlp(LN2(x));  LayerNorm eps 1e-6, GELU (erf)
  GPSA (blocks < local)   q, k = qk(x) split (2, heads, dh);  v = v(x) split (heads, dh);  patch = softmax((q @ k^T) * scale);
                          pos = softmax(pos_proj(rel_indices) over keys);  a = (1 - sigmoid(g)) patch + sigmoid(g) pos;  a /= a.sum(keys);
                          out = proj((a @ v) heads joined);  rel_indices[i][j] = (jx - ix, jy - iy, dx^2 + dy^2), token = y * grid + x
  join                    x = cat(cls_token, x) before block `local`
  MHSA (blocks >= local)  q, k, v = qkv(x) split (3, heads, dh);  a = softmax((q @ k^T) * scale);  out = proj((a @ v) heads joined)
`norm` and `head` lie behind every hook and are not restated.
"""
import torch
import torch.nn.functional as F

from tests.family_harness import StreamsReference


def rel_indices(grid: int, dtype=torch.float64):
    """timm's `GPSA.get_rel_indices`, as timm builds it (repeat / repeat_interleave)."""
    n = grid * grid
    ind = torch.arange(grid).view(1, -1) - torch.arange(grid).view(-1, 1)
    indx = ind.repeat(grid, grid)
    indy = ind.repeat_interleave(grid, dim=0).repeat_interleave(grid, dim=1)
    out = torch.zeros(n, n, 3, dtype=dtype)
    out[:, :, 2] = (indx ** 2 + indy ** 2).to(dtype)
    out[:, :, 1] = indy.to(dtype)
    out[:, :, 0] = indx.to(dtype)
    return out


def gpsa_core(q, k, v, scale, pos_w, pos_b, gating, rel):
    """timm's `GPSA.get_attention` and the product with v on (frames, heads, T, dh) tensors -> (frames, T, heads dh)."""
    n, H, T, dh = q.shape
    pos = F.linear(rel, pos_w, pos_b).permute(2, 0, 1).unsqueeze(0).expand(n, -1, -1, -1)
    patch = ((q @ k.transpose(-2, -1)) * scale).softmax(dim=-1)
    pos = pos.softmax(dim=-1)
    g = torch.sigmoid(gating).view(1, -1, 1, 1)
    a = (1.0 - g) * patch + g * pos
    a = a / a.sum(dim=-1).unsqueeze(-1)
    return (a @ v).transpose(1, 2).reshape(n, T, H * dh)


def blend_attention(qkv, heads, scale, c=None, table=None):
    """The DEFINITION of the library's attention entry on qkv (frames, T, 3 heads dh): out = (c_h softmax(scale q k^T) + table_h) v, no
    division, any non-negative table (heads, T, T); c and table None: plain attention -> (out, Ppatch (frames, heads, T, T))."""
    n, T, C3 = qkv.shape
    dh = C3 // (3 * heads)
    q, k, v = qkv.reshape(n, T, 3, heads, dh).permute(2, 0, 3, 1, 4)
    p = ((q * scale) @ k.transpose(-2, -1)).softmax(dim=-1)
    a = p if table is None else c.view(1, -1, 1, 1) * p + table.unsqueeze(0)
    return (a @ v).transpose(1, 2).reshape(n, T, heads * dh), p


def stem(x, sd, spec):
    t = F.conv2d(x, sd["patch_embed.proj.weight"], sd["patch_embed.proj.bias"], stride=spec.patch).flatten(2).transpose(1, 2)
    return t + sd["pos_embed"]


def block(x, sd, spec, i: int, local: bool, rel, plain: bool = False, swap_xy: bool = False):
    p = f"blocks.{i}."
    n, T, D = x.shape
    H, dh = spec.heads, D // spec.heads
    t = F.layer_norm(x, (D,), sd[p + "norm1.weight"], sd[p + "norm1.bias"], spec.ln_eps)
    if local:
        qk = F.linear(t, sd[p + "attn.qk.weight"]).reshape(n, T, 2, H, dh).permute(2, 0, 3, 1, 4)
        v = F.linear(t, sd[p + "attn.v.weight"]).reshape(n, T, H, dh).permute(0, 2, 1, 3)
        w, gating = sd[p + "attn.pos_proj.weight"], sd[p + "attn.gating_param"]
        if swap_xy:
            w = w[:, [1, 0, 2]]
        if plain:                                                       # sigmoid(-inf) = 0: content attention only
            gating = torch.full_like(gating, -float("inf"))
        a = gpsa_core(qk[0], qk[1], v, dh ** -0.5, w, sd[p + "attn.pos_proj.bias"], gating, rel)
    else:
        q, k, v = F.linear(t, sd[p + "attn.qkv.weight"]).reshape(n, T, 3, H, dh).permute(2, 0, 3, 1, 4)
        a = (((q @ k.transpose(-2, -1)) * dh ** -0.5).softmax(dim=-1) @ v).transpose(1, 2).reshape(n, T, D)
    x = x + F.linear(a, sd[p + "attn.proj.weight"], sd[p + "attn.proj.bias"])
    t = F.layer_norm(x, (D,), sd[p + "norm2.weight"], sd[p + "norm2.bias"], spec.ln_eps)
    return x + F.linear(F.gelu(F.linear(t, sd[p + "mlp.fc1.weight"], sd[p + "mlp.fc1.bias"])), sd[p + "mlp.fc2.weight"], sd[p + "mlp.fc2.bias"])


def streams(x, sd, spec, n_blocks, plain: bool = False, swap_xy: bool = False):
    """The residual streams behind the blocks 0 .. n_blocks - 1, each (frames, tokens, dim)."""
    rel = rel_indices(spec.grid, x.dtype).to(x.device)
    t, outs = stem(x, sd, spec), []
    for i in range(n_blocks):
        if i == spec.local_blocks:          # the class token joins here: a spec with another `local_blocks` moves the join
            t = torch.cat([sd["cls_token"].expand(t.shape[0], -1, -1), t], dim=1)
        t = block(t, sd, spec, i, i < spec.local_blocks, rel, plain, swap_xy)
        outs.append(t)
    return outs


#: What the sensitivity checks compare against: `plain` -- every GPSA block computes content attention only (c = 1 with a zero table);
#: `swap_xy` -- the x and y columns of `pos_proj.weight` exchanged.
class ConvitReference(StreamsReference):
    streams = staticmethod(streams)
