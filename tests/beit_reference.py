"""timm 0.5.0's `Beit` up to its last block, written from the architecture definition in plain torch on the CPU:
the float64 reference of the BEiT tests.  Token-major (frames, tokens, dim) as timm computes it, and with timm's LITERAL arithmetic -- the
patch embedding is a `conv2d` call, the qkv bias is concatenated per call, q is scaled before the product, the bias is gathered from the
table through an index built with `beit.py`'s own construction (meshgrid, flatten, the three special values), and gamma_1 / gamma_2
multiply AFTER `proj` / `fc2` -- so that the packing of `BeitSpec.native_arrays` (the dense bias, the folded LayerScale, the built qkv
bias) is tested, not assumed.

  embed      x = patch_embed.proj: conv2d(kernel = stride = patch) -> (tokens, dim);  cls_token in front;  no pos_embed
  block      x = x + gamma_1 * proj(attn(LN1 x));  x = x + gamma_2 * fc2(gelu(fc1(LN2 x)));  LayerNorm eps 1e-6
  attn       qkv = F.linear(x, qkv.weight, cat(q_bias, 0, v_bias)) split (3, heads, dh);  q = q * dh^-0.5;  a = q @ k^T;
             a = a + table[index].view(T, T, heads).permute(2, 0, 1);  softmax;  a @ v
`norm` / `fc_norm` and `head` lie behind every hook and are not restated.
"""
import torch
import torch.nn.functional as F

from tests.family_harness import StreamsReference


def relative_position_index(g: int) -> torch.Tensor:
    """`beit.Attention.__init__`'s construction for a window of (g, g), independent of `BeitSpec.relative_position_index`."""
    n = (2 * g - 1) * (2 * g - 1) + 3
    coords = torch.stack(torch.meshgrid([torch.arange(g), torch.arange(g)], indexing="ij"))      # 2, g, g
    flat = torch.flatten(coords, 1)
    rel = (flat[:, :, None] - flat[:, None, :]).permute(1, 2, 0).contiguous()                   # g g, g g, 2
    rel[:, :, 0] += g - 1
    rel[:, :, 1] += g - 1
    rel[:, :, 0] *= 2 * g - 1
    idx = torch.zeros((g * g + 1,) * 2, dtype=rel.dtype)
    idx[1:, 1:] = rel.sum(-1)
    idx[0, 0:] = n - 3
    idx[0:, 0] = n - 2
    idx[0, 0] = n - 1
    return idx


_INDEX = {}      # (g, device) -> the index, as the module's registered buffer is: built once, kept where the table lives


def gathered_bias(table: torch.Tensor, g: int) -> torch.Tensor:
    """(heads, T, T) from a (rows, heads) table, as `beit.Attention.forward` gathers it."""
    T = g * g + 1
    key = (g, str(table.device))
    if key not in _INDEX:
        _INDEX[key] = relative_position_index(g).to(table.device)
    return table[_INDEX[key].view(-1)].view(T, T, -1).permute(2, 0, 1).contiguous()


def attn_core(qkv, bias, heads):
    """`beit.Attention.forward` between its Linears: qkv (frames, T, 3 heads dh), bias (heads, T, T) or None -> (frames, T, heads dh)."""
    n, T, C3 = qkv.shape
    C = C3 // 3
    dh = C // heads
    q, k, v = qkv.reshape(n, T, 3, heads, dh).permute(2, 0, 3, 1, 4).unbind(0)
    q = q * dh ** -0.5
    attn = q @ k.transpose(-2, -1)
    if bias is not None:
        attn = attn + bias.unsqueeze(0)
    return (attn.softmax(dim=-1) @ v).transpose(1, 2).reshape(n, T, C)


def block(x, sd, spec, i, skip=()):
    p = f"blocks.{i}."
    D = x.shape[-1]
    g1, g2 = sd[p + "gamma_1"], sd[p + "gamma_2"]
    if "gamma" in skip:
        g1, g2 = torch.ones_like(g1), torch.ones_like(g2)
    table = sd[p + "attn.relative_position_bias_table"]
    if "bias" in skip:
        table = torch.zeros_like(table)
    t = F.layer_norm(x, (D,), sd[p + "norm1.weight"], sd[p + "norm1.bias"], spec.ln_eps)
    qkv_bias = torch.cat((sd[p + "attn.q_bias"], torch.zeros_like(sd[p + "attn.v_bias"]), sd[p + "attn.v_bias"]))
    a = attn_core(F.linear(t, sd[p + "attn.qkv.weight"], qkv_bias), gathered_bias(table, spec.grid), spec.heads)
    x = x + g1 * F.linear(a, sd[p + "attn.proj.weight"], sd[p + "attn.proj.bias"])
    t = F.layer_norm(x, (D,), sd[p + "norm2.weight"], sd[p + "norm2.bias"], spec.ln_eps)
    return x + g2 * F.linear(F.gelu(F.linear(t, sd[p + "mlp.fc1.weight"], sd[p + "mlp.fc1.bias"])), sd[p + "mlp.fc2.weight"], sd[p + "mlp.fc2.bias"])


def streams(x, sd, spec, n_blocks, skip=()):
    """The residual streams after blocks 0 .. n_blocks - 1, each (frames, tokens, dim)."""
    x = F.conv2d(x, sd["patch_embed.proj.weight"], sd["patch_embed.proj.bias"], stride=spec.patch).flatten(2).transpose(1, 2)
    x = torch.cat((sd["cls_token"].expand(x.shape[0], -1, -1), x), dim=1)
    outs = []
    for i in range(n_blocks):
        x = block(x, sd, spec, i, skip)
        outs.append(x)
    return outs


#: `skip` names what the sensitivity checks leave out: "bias" (a table of zeros), "gamma" (LayerScale of 1).
class BeitReference(StreamsReference):
    streams = staticmethod(streams)
