"""timm 0.5.0's `MlpMixer` (MLP-Mixer and ResMLP) written from the architecture definition in plain torch on the CPU (DESIGN.md section
19): the float64 reference of the Mixer tests.  Token-major (frames, tokens, dim) as timm computes it; the token mixing is written as
timm writes it, with the two transposes around an `nn.Linear`-style product -- not as the packed arrays or the kernel lay it out.

  stem                 conv patch x patch / patch with bias, flattened to (tokens, dim); no norm, no prefix token, no pos_embed
  MixerBlock           x = x + mlp_tokens(LN1(x)^T)^T        mlp_tokens: fc1 (tokens -> dim / 2), GELU (erf), fc2
                       x = x + mlp_channels(LN2(x))          mlp_channels: fc1 (dim -> 4 dim), GELU, fc2;  LayerNorm eps 1e-6
  ResBlock (ResMLP)    x = x + ls1 * linear_tokens(Affine1(x)^T)^T            Affine(x) = alpha * x + beta
                       x = x + ls2 * mlp_channels(Affine2(x))
"""
import torch
import torch.nn.functional as F

from tests.family_harness import StreamsReference


def stem(x, sd, spec):
    return F.conv2d(x, sd["stem.proj.weight"], sd["stem.proj.bias"], stride=spec.patch).flatten(2).transpose(1, 2)


def mlp(x, sd, p):
    return F.linear(F.gelu(F.linear(x, sd[p + "fc1.weight"], sd[p + "fc1.bias"])), sd[p + "fc2.weight"], sd[p + "fc2.bias"])


def mixer_block(x, sd, spec, i: int):
    p = f"blocks.{i}."
    D = x.shape[-1]
    t = F.layer_norm(x, (D,), sd[p + "norm1.weight"], sd[p + "norm1.bias"], spec.ln_eps)
    x = x + mlp(t.transpose(1, 2), sd, p + "mlp_tokens.").transpose(1, 2)
    t = F.layer_norm(x, (D,), sd[p + "norm2.weight"], sd[p + "norm2.bias"], spec.ln_eps)
    return x + mlp(t, sd, p + "mlp_channels.")


def res_block(x, sd, spec, i: int, unit_ls: bool = False, no_norm2: bool = False):
    p = f"blocks.{i}."
    ls1, ls2 = (torch.ones_like(sd[p + k]) if unit_ls else sd[p + k] for k in ("ls1", "ls2"))
    t = sd[p + "norm1.alpha"] * x + sd[p + "norm1.beta"]
    x = x + ls1 * F.linear(t.transpose(1, 2), sd[p + "linear_tokens.weight"], sd[p + "linear_tokens.bias"]).transpose(1, 2)
    t = x if no_norm2 else sd[p + "norm2.alpha"] * x + sd[p + "norm2.beta"]
    return x + ls2 * mlp(t, sd, p + "mlp_channels.")


def token_mix(z, residual, w1, b1, w2=None, b2=None, in_scale=None, in_shift=None, out_scale=None):
    """The token-mixing launch of include/i2v_mixer.h on (frames, S, C) tensors, through F.linear on the transposed tile."""
    t = z if in_scale is None else in_scale * z + in_shift
    u = F.linear(t.transpose(1, 2), w1, b1)
    if w2 is not None:
        u = F.linear(F.gelu(u), w2, b2)
    u = u.transpose(1, 2)
    return residual + (u if out_scale is None else out_scale * u)


def streams(x, sd, spec, n_blocks, unit_ls: bool = False, no_norm2: bool = False):
    """The residual streams behind the blocks 0 .. n_blocks - 1, each (frames, tokens, dim)."""
    t, outs = stem(x, sd, spec), []
    for i in range(n_blocks):
        t = mixer_block(t, sd, spec, i) if spec.kind == "mixer" else res_block(t, sd, spec, i, unit_ls, no_norm2)
        outs.append(t)
    return outs


#: `unit_ls` / `no_norm2`: a ResMLP with its layer scales set to one, or without the affine in front of its channel MLP -- what a
#: dropped fold would compute.
class MixerReference(StreamsReference):
    streams = staticmethod(streams)
