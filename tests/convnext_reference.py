"""timm's ConvNeXt written from the architecture definition in plain torch on the CPU: the float64 reference of
the ConvNeXt tests.  NCHW throughout, as timm computes it; the hooked features are handed out token-major -- (row, column, channel)
flattened -- the layout the engine hands to the loss kernels.

  stem        conv 4 x 4 / 4 with bias, LayerNorm over channels (eps 1e-6)
  stage i     [i >= 1: LayerNorm over channels, conv 2 x 2 / 2 with bias]  then depths[i] blocks
  block       x + gamma * fc2(GELU(fc1(LN(dwconv7x7(x)))))      depthwise: groups = C, padding 3, bias; LN, fc1, GELU (erf), fc2 per position
"""
from typing import Sequence

import torch.nn.functional as F

from tests.family_harness import StreamsReference


def layer_norm_c(x, w, b, eps):
    """LayerNorm over the channels of an NCHW tensor."""
    return F.layer_norm(x.permute(0, 2, 3, 1), (x.shape[1],), w, b, eps).permute(0, 3, 1, 2)


def stem(x, sd, spec):
    return layer_norm_c(F.conv2d(x, sd["stem.0.weight"], sd["stem.0.bias"], stride=spec.patch), sd["stem.1.weight"], sd["stem.1.bias"], spec.ln_eps)


def downsample(x, sd, spec, i: int):
    p = f"stages.{i}.downsample."
    return F.conv2d(layer_norm_c(x, sd[p + "0.weight"], sd[p + "0.bias"], spec.ln_eps), sd[p + "1.weight"], sd[p + "1.bias"], stride=2)


def block(x, sd, spec, i: int, j: int, unit_gamma: bool = False):
    p = f"stages.{i}.blocks.{j}."
    C = x.shape[1]
    u = F.conv2d(x, sd[p + "conv_dw.weight"], sd[p + "conv_dw.bias"], padding=3, groups=C)
    t = F.layer_norm(u.permute(0, 2, 3, 1), (C,), sd[p + "norm.weight"], sd[p + "norm.bias"], spec.ln_eps)
    t = F.linear(F.gelu(F.linear(t, sd[p + "mlp.fc1.weight"], sd[p + "mlp.fc1.bias"])), sd[p + "mlp.fc2.weight"], sd[p + "mlp.fc2.bias"])
    if not unit_gamma:
        t = t * sd[p + "gamma"]
    return x + t.permute(0, 3, 1, 2)


def run_stages(t, sd, spec, hook_stages: Sequence[int], unit_gamma: bool = False):
    outs = {}
    for i in range(max(hook_stages) + 1):
        if i > 0:
            t = downsample(t, sd, spec, i)
        for j in range(spec.depths[i]):
            t = block(t, sd, spec, i, j, unit_gamma)
        outs[i] = t
    return [outs[s] for s in hook_stages]


def dwconv_token_major(x, filt, bias=None):
    """The depthwise node on a token-major tensor: x (N, H, W, C), filt (49, C) -> (N, H, W, C), through F.conv2d(groups=C)."""
    C = x.shape[-1]
    w = filt.t().reshape(C, 1, 7, 7)
    return F.conv2d(x.permute(0, 3, 1, 2), w, bias, padding=3, groups=C).permute(0, 2, 3, 1)


def streams(x, sd, spec, n_stages, unit_gamma: bool = False):
    """The planes behind the stages 0 .. n_stages - 1, token-major: each (frames, H, W, C)."""
    return [o.permute(0, 2, 3, 1) for o in run_stages(stem(x, sd, spec), sd, spec, list(range(n_stages)), unit_gamma)]


class ConvNextReference(StreamsReference):
    streams = staticmethod(streams)
