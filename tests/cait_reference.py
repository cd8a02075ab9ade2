"""timm 0.5.0's `Cait` up to its last self-attention block, written from the architecture definition in plain torch on the CPU (DESIGN.md
section 21): the float64 reference of the CaiT tests.  Token-major (frames, tokens, dim) as timm computes it; talking-heads attention is
written as timm writes it -- the two `nn.Linear`s over the head axis applied to the permuted score tensor -- not as the kernel tiles it.

  stem                    conv patch x patch / patch with bias, flattened to (tokens, dim), + pos_embed; no cls_token in the stream
  LayerScale_Block        x = x + gamma_1 * attn(LN1(x));  x = x + gamma_2 * mlp(LN2(x));  LayerNorm eps 1e-6, GELU (erf)
  TalkingHeadAttn         q, k, v = qkv(x) split (3, heads, dh);  a = (q * scale) @ k^T;  a = proj_l(a over heads);  a = softmax(a, keys);
                          a = proj_w(a over heads);  out = proj((a @ v) heads joined)
The class-attention blocks, `norm` and `head` lie behind every hook and are not restated.
"""
import torch.nn.functional as F

from tests.family_harness import StreamsReference


def talking_heads(qkv, heads, scale, wl, bl, ww, bw, identity_mix: bool = False):
    """The attention core on qkv (frames, T, 3 heads dh) -> (out (frames, T, heads dh), P (frames, heads, T, T): post-softmax, pre-mix).
    `identity_mix`: plain multi-head attention -- what a skipped pair of head mixes computes."""
    n, T, C3 = qkv.shape
    dh = C3 // (3 * heads)
    q, k, v = qkv.reshape(n, T, 3, heads, dh).permute(2, 0, 3, 1, 4)
    a = (q * scale) @ k.transpose(-2, -1)
    if not identity_mix:
        a = F.linear(a.permute(0, 2, 3, 1), wl, bl).permute(0, 3, 1, 2)
    p = a.softmax(dim=-1)
    a = p if identity_mix else F.linear(p.permute(0, 2, 3, 1), ww, bw).permute(0, 3, 1, 2)
    return (a @ v).transpose(1, 2).reshape(n, T, heads * dh), p


def stem(x, sd, spec):
    t = F.conv2d(x, sd["patch_embed.proj.weight"], sd["patch_embed.proj.bias"], stride=spec.patch).flatten(2).transpose(1, 2)
    return t + sd["pos_embed"]


def block(x, sd, spec, i: int, identity_mix: bool = False, gamma=None):
    p = f"blocks.{i}."
    D = x.shape[-1]
    g1, g2 = (sd[p + "gamma_1"], sd[p + "gamma_2"]) if gamma is None else (gamma, gamma)
    t = F.layer_norm(x, (D,), sd[p + "norm1.weight"], sd[p + "norm1.bias"], spec.ln_eps)
    qkv = F.linear(t, sd[p + "attn.qkv.weight"], sd[p + "attn.qkv.bias"])
    a, _ = talking_heads(qkv, spec.heads, (D // spec.heads) ** -0.5, sd[p + "attn.proj_l.weight"], sd[p + "attn.proj_l.bias"],
                         sd[p + "attn.proj_w.weight"], sd[p + "attn.proj_w.bias"], identity_mix)
    x = x + g1 * F.linear(a, sd[p + "attn.proj.weight"], sd[p + "attn.proj.bias"])
    t = F.layer_norm(x, (D,), sd[p + "norm2.weight"], sd[p + "norm2.bias"], spec.ln_eps)
    t = F.linear(F.gelu(F.linear(t, sd[p + "mlp.fc1.weight"], sd[p + "mlp.fc1.bias"])), sd[p + "mlp.fc2.weight"], sd[p + "mlp.fc2.bias"])
    return x + g2 * t


def streams(x, sd, spec, n_blocks, identity_mix: bool = False, gamma=None):
    """The residual streams behind the blocks 0 .. n_blocks - 1, each (frames, tokens, dim)."""
    t, outs = stem(x, sd, spec), []
    for i in range(n_blocks):
        t = block(t, sd, spec, i, identity_mix, gamma)
        outs.append(t)
    return outs


#: What the sensitivity checks compare against: `identity_mix` -- both head mixes replaced by the identity with zero biases; `gamma` --
#: both LayerScale vectors replaced by this constant.
class CaitReference(StreamsReference):
    streams = staticmethod(streams)
