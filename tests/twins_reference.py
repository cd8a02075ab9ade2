"""timm 0.5.0's `Twins` (PCPVT and SVT) up to its last block, written from the architecture definition in plain torch on the CPU (DESIGN.md
section 25): the float64 reference of the Twins tests.  Token-major (frames, tokens, dim) as timm computes it, and with timm's LITERAL
arithmetic -- the patch embeddings, the sub-sampling `attn.sr` and the position encoding are `conv2d` calls on the plane, q and kv are
separate products, the windows are cut by reshape and transpose -- so that the gathers and repacks of `TwinsSpec.native_arrays` are
tested, not assumed.

  stage k    x = patch_embeds.k: conv2d(kernel = stride = patch) -> (tokens, dim) -> LayerNorm (eps 1e-5);  the blocks;  after block 0
             pos_block.k: x = x + dwconv3x3(x) + bias on the (grid, grid) plane;  then back to a plane for the next stage
  block      x = x + attn(LN1 x);  x = x + fc2(gelu(fc1(LN2 x)));  LayerNorm eps 1e-6
  GSA        q = q(x) split (heads, dh);  where sr > 1: x = LayerNorm(sr(x as a plane) as tokens) (eps 1e-5);  k, v = kv(x) split
             (2, heads, dh);  softmax((q @ k^T) * dh^-0.5) @ v;  proj
  LSA        the plane cut into window x window groups;  qkv split (3, heads, dh) per group;  softmax((q @ k^T) * dh^-0.5) @ v;  the
             groups put back;  proj
`norm` and `head` lie behind every hook and are not restated.
"""
import torch.nn.functional as F

from tests.family_harness import StreamsReference

PE_EPS = 1e-5


def gsa_core(q, kv, heads):
    """timm's `GlobalSubSampleAttn.forward` between its Linears: q (frames, Tq, heads dh), kv (frames, Tk, 2 heads dh) -> (frames, Tq,
    heads dh)."""
    n, Tq, C = q.shape
    dh = C // heads
    qh = q.reshape(n, Tq, heads, dh).permute(0, 2, 1, 3)
    k, v = kv.reshape(n, -1, 2, heads, dh).permute(2, 0, 3, 1, 4).unbind(0)
    attn = ((qh @ k.transpose(-2, -1)) * dh ** -0.5).softmax(dim=-1)
    return (attn @ v).transpose(1, 2).reshape(n, Tq, C)


def lsa_core(qkv, heads, grid, ws):
    """timm's `LocallyGroupedAttn.forward` between its Linears, on qkv (frames, grid^2, 3 heads dh) in plane order -> (frames, grid^2,
    heads dh).  (timm applies qkv to the grouped plane; a Linear commutes with the regrouping.)"""
    n, T, C3 = qkv.shape
    C, hg = C3 // 3, grid // ws
    dh = C // heads
    x = qkv.reshape(n, hg, ws, hg, ws, C3).transpose(2, 3)
    q, k, v = x.reshape(n, hg * hg, ws * ws, 3, heads, dh).permute(3, 0, 1, 4, 2, 5).unbind(0)
    attn = ((q @ k.transpose(-2, -1)) * dh ** -0.5).softmax(dim=-1)
    out = (attn @ v).transpose(2, 3).reshape(n, hg, hg, ws, ws, C)
    return out.transpose(2, 3).reshape(n, T, C)


def block(x, sd, spec, k, j, skip=()):
    p = f"blocks.{k}.{j}."
    n, T, D = x.shape
    g, sr = spec.grid(k), spec.sr_ratios[k]
    t = F.layer_norm(x, (D,), sd[p + "norm1.weight"], sd[p + "norm1.bias"], spec.ln_eps)
    if spec.is_lsa(k, j):
        a = lsa_core(F.linear(t, sd[p + "attn.qkv.weight"], sd[p + "attn.qkv.bias"]), spec.heads[k], g, spec.window)
    else:
        q = F.linear(t, sd[p + "attn.q.weight"], sd[p + "attn.q.bias"])
        u = t
        if sr > 1:
            plane = t.permute(0, 2, 1).reshape(n, D, g, g)
            u = F.conv2d(plane, sd[p + "attn.sr.weight"], sd[p + "attn.sr.bias"], stride=sr).reshape(n, D, -1).permute(0, 2, 1)
            if "sr_norm" not in skip:
                u = F.layer_norm(u, (D,), sd[p + "attn.norm.weight"], sd[p + "attn.norm.bias"], PE_EPS)
        a = gsa_core(q, F.linear(u, sd[p + "attn.kv.weight"], sd[p + "attn.kv.bias"]), spec.heads[k])
    x = x + F.linear(a, sd[p + "attn.proj.weight"], sd[p + "attn.proj.bias"])
    t = F.layer_norm(x, (D,), sd[p + "norm2.weight"], sd[p + "norm2.bias"], spec.ln_eps)
    return x + F.linear(F.gelu(F.linear(t, sd[p + "mlp.fc1.weight"], sd[p + "mlp.fc1.bias"])), sd[p + "mlp.fc2.weight"], sd[p + "mlp.fc2.bias"])


def peg(x, sd, spec, k):
    n, T, D = x.shape
    plane = x.transpose(1, 2).reshape(n, D, spec.grid(k), spec.grid(k))
    y = F.conv2d(plane, sd[f"pos_block.{k}.proj.0.weight"], sd[f"pos_block.{k}.proj.0.bias"], padding=1, groups=D) + plane
    return y.flatten(2).transpose(1, 2)


def stages(x, sd, spec, n_stages, skip=()):
    """The streams after the last block of stages 0 .. n_stages - 1, each (frames, tokens, dim)."""
    outs = []
    for k in range(n_stages):
        p = f"patch_embeds.{k}."
        x = F.conv2d(x, sd[p + "proj.weight"], sd[p + "proj.bias"], stride=2 if k else spec.patch).flatten(2).transpose(1, 2)
        x = F.layer_norm(x, (spec.dims[k],), sd[p + "norm.weight"], sd[p + "norm.bias"], PE_EPS)
        for j in range(spec.depths[k]):
            x = block(x, sd, spec, k, j, skip)
            if j == 0 and "peg" not in skip:
                x = peg(x, sd, spec, k)
        outs.append(x)
        x = x.reshape(x.shape[0], spec.grid(k), spec.grid(k), -1).permute(0, 3, 1, 2)
    return outs


#: `skip` names what the sensitivity checks leave out: "peg" (no position encoding), "sr_norm" (the sub-sampled plane without its
#: LayerNorm).
class TwinsReference(StreamsReference):
    streams = staticmethod(stages)
