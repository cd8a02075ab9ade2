"""timm 0.5.0's serial `CoaT` (CoaT-Lite) up to its last block, written from the model description in plain torch on the CPU (DESIGN.md
section 30; restated from memory of coat.py, UNCHECKED against timm): the float64 reference of the CoaT tests, and the float64 / float32
restatement of the new kernels.  Written from the description, not from i2v_amd.graphs: the patch embeddings, cpe and crpe are `conv2d`
calls on (frames, C, g, g) planes, the heads are split off with reshapes, the class token is concatenated in front -- so that the packing
of `CoatSpec.native_arrays` (tap-major filters, the cell gather's column order, crpe's concatenated biases) and the token-major kernels
are tested, not assumed.

  embed      stage 1: conv2d(3 -> C, 4, stride 4) on the frame; stage k > 1: conv2d(C' -> C, 2, stride 2) on the previous stage's grid
             tokens as a plane, the class token dropped; flattened, LayerNorm, `cls_token{k}` in front
  block      x = cpe(x);  x = x + proj(FA(LN1 x));  x = x + fc2(gelu(fc1(LN2 x)));  LayerNorm eps 1e-6, exact GELU
  cpe        grid tokens as a plane: plane + conv2d(plane, 3 x 3, padding 1, groups C); the class row passes through
  FA         qkv = Linear(x) split (3, heads, dh);  Ks = softmax of k over the tokens;  G = Ks^T v;  out = dh^-0.5 q G + q o E
  E          0 on the class row; v's grid rows as a plane, channel = head dh + column, split by head runs into conv_list.0 / 1 / 2
             (3 x 3, 5 x 5, 7 x 7 depthwise, "same" padding, bias)
`norm*`, `head` and `aggregate` lie behind every hook and are not restated.
"""
import torch
import torch.nn.functional as F

from tests.family_harness import StreamsReference

def crpe(v, filters, biases, g, prefix=1):
    """E of v (frames, prefix + g^2, C): `filters[i]` (n_i, 1, K_i, K_i) on the next n_i channels; zeros on the prefix rows."""
    n, _, C = v.shape
    plane = v[:, prefix:].transpose(1, 2).reshape(n, C, g, g)
    parts, at = [], 0
    for w, b in zip(filters, biases):
        if w is not None and w.shape[0]:
            parts.append(F.conv2d(plane[:, at:at + w.shape[0]], w, b, padding=w.shape[-1] // 2, groups=w.shape[0]))
            at += w.shape[0]
    e = torch.cat(parts, dim=1).flatten(2).transpose(1, 2)
    return torch.cat((torch.zeros(n, prefix, C, dtype=v.dtype, device=v.device), e), dim=1)


def cpe(x, w, b, g, prefix=1):
    """x (frames, prefix + g^2, C) -> the prefix rows as they are, the grid rows plus their depthwise 3 x 3."""
    n, _, C = x.shape
    plane = x[:, prefix:].transpose(1, 2).reshape(n, C, g, g)
    plane = plane + F.conv2d(plane, w, b, padding=1, groups=C)
    return torch.cat((x[:, :prefix], plane.flatten(2).transpose(1, 2)), dim=1)


def factor_parts(qkv, heads):
    """q, k, v (frames, heads, T, dh), Ks and G (frames, heads, dh, dh) of the factorized attention."""
    n, T, C3 = qkv.shape
    dh = C3 // 3 // heads
    q, k, v = qkv.reshape(n, T, 3, heads, dh).permute(2, 0, 3, 1, 4).unbind(0)
    ks = k.softmax(dim=2)                                                  # over the TOKENS, per channel
    return q, k, v, ks, ks.transpose(-2, -1) @ v


def factor_core(qkv, E, heads):
    """qkv (frames, T, 3 heads dh), E (frames, T, heads dh) -> out (frames, T, heads dh)."""
    n, T, C3 = qkv.shape
    q, _, _, _, G = factor_parts(qkv, heads)
    dh = q.shape[-1]
    e = E.reshape(n, T, heads, dh).transpose(1, 2)
    return (dh ** -0.5 * (q @ G) + q * e).transpose(1, 2).reshape(n, T, C3 // 3)


def cells(x, g, s, prefix=1):
    """The s x s cells of the grid rows: x (frames, prefix + g^2, C) -> (frames (g / s)^2, s^2 C), column (dy s + dx) C + c."""
    n, _, C = x.shape
    p = x[:, prefix:].reshape(n, g // s, s, g // s, s, C).permute(0, 1, 3, 2, 4, 5)
    return p.reshape(n * (g // s) ** 2, s * s * C)


def block(x, sd, p, s, spec, g, skip=()):
    D, heads = x.shape[-1], spec.heads
    cw = sd[f"cpe{s}.proj.weight"]
    x = cpe(x, torch.zeros_like(cw) if "cpe" in skip else cw, None if "cpe" in skip else sd[f"cpe{s}.proj.bias"], g)
    t = F.layer_norm(x, (D,), sd[p + "norm1.weight"], sd[p + "norm1.bias"], spec.ln_eps)
    qkv = F.linear(t, sd[p + "factoratt_crpe.qkv.weight"], sd[p + "factoratt_crpe.qkv.bias"])
    filt = [sd[f"crpe{s}.conv_list.{i}.weight"] for i in range(3)]
    for i in range(3):
        if f"crpe{i}" in skip:
            filt[i] = torch.zeros_like(filt[i])
    E = crpe(qkv[:, :, 2 * D:], filt, [sd[f"crpe{s}.conv_list.{i}.bias"] for i in range(3)], g)
    x = x + F.linear(factor_core(qkv, E, heads), sd[p + "factoratt_crpe.proj.weight"], sd[p + "factoratt_crpe.proj.bias"])
    t = F.layer_norm(x, (D,), sd[p + "norm2.weight"], sd[p + "norm2.bias"], spec.ln_eps)
    return x + F.linear(F.gelu(F.linear(t, sd[p + "mlp.fc1.weight"], sd[p + "mlp.fc1.bias"])), sd[p + "mlp.fc2.weight"], sd[p + "mlp.fc2.bias"])


def streams(x, sd, spec, n_stages, skip=()):
    """The residual streams behind the stages 0 .. n_stages - 1, each (frames, 1 + g^2, width)."""
    n, outs = x.shape[0], []
    plane = x
    for k in range(n_stages):
        s, D = k + 1, spec.widths[k]
        plane = F.conv2d(plane, sd[f"patch_embed{s}.proj.weight"], sd[f"patch_embed{s}.proj.bias"], stride=2 if k else 4)
        g = plane.shape[-1]
        tok = F.layer_norm(plane.flatten(2).transpose(1, 2), (D,), sd[f"patch_embed{s}.norm.weight"], sd[f"patch_embed{s}.norm.bias"], spec.ln_eps)
        cls = sd[f"cls_token{s}"]
        if "cls" in skip:
            cls = torch.zeros_like(cls)
        t = torch.cat((cls.expand(n, -1, -1), tok), dim=1)
        for j in range(spec.depths[k]):
            t = block(t, sd, f"serial_blocks{s}.{j}.", s, spec, g, skip)
        outs.append(t)
        plane = t[:, 1:].transpose(1, 2).reshape(n, D, g, g)               # the class token is dropped
    return outs


#: `skip` names what the sensitivity checks leave out: "cpe" (no convolutional position encoding), "crpe0" / "crpe1" / "crpe2" (one
#: window's filter zero), "cls" (class tokens of zeros).
class CoatReference(StreamsReference):
    streams = staticmethod(streams)
