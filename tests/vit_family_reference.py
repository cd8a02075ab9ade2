"""Plain-torch restatement of the ViT / DeiT family of surrogates -- the yardstick of the family's tests.  Written
from the models' definition (timm 0.5.0 `VisionTransformer`: `vit_*_patch{16,32}_224`, `deit_*_patch16_224` and the distilled
`deit_*_distilled_patch16_224`), parametrised by the spec alone and independent of the HIP path.

What the spec says: `patch`, `dim`, `heads`, `mlp`, `blocks`, `ln_eps` and `n_prefix`.  The token sequence of a frame is
`[cls_token; dist_token (n_prefix = 2 only); patch embeddings in row-major patch order] + pos_embed`, `pos_embed` being
`(n_prefix + (img / patch) ** 2, dim)`; then pre-norm blocks.  Nothing but the prefix differs between a plain and a distilled model, and
nothing but the numbers between the sizes.  For `n_prefix = 1` this file computes exactly what `tests/vit_reference.py` does
(`tests/test_vit_family_cpu.py` holds the two to equality).

`VitFamilyReference` has the interface of `oracle.restate.OracleNet` that `oracle.restate.run_attack` drives: `.dtype`, `.hooks`,
`.forward(x) -> [hook features]` and `.backward(hook_grads) -> d cost / d x`; a hook feature is (frames, tokens * dim), the residual
stream after its block, every prefix token included."""
from typing import Sequence

import torch
import torch.nn.functional as F

from tests.family_harness import StreamsReference

PREFIX_KEYS = ("cls_token", "dist_token")


def layer_norm(x, w, b, eps):
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)                  # biased
    return (x - mu) / torch.sqrt(var + eps) * w + b


def gelu(x):
    return 0.5 * x * (1.0 + torch.erf(x / 2 ** 0.5))              # exact form


def patch_rows(x, sd, spec):
    """(N, 3, H, W) -> (N, (H / patch) (W / patch), dim): the patch x patch convolution with stride patch, flattened row-major."""
    p = F.conv2d(x, sd["patch_embed.proj.weight"], sd["patch_embed.proj.bias"], stride=spec.patch)
    return p.flatten(2).transpose(1, 2)


def embed(x, sd, spec):
    """(N, 3, H, W) -> (N, tokens, dim): the prefix tokens ahead of the patch rows, pos_embed added to all of them."""
    prefix = [sd[k].reshape(1, 1, -1).expand(x.shape[0], 1, spec.dim) for k in PREFIX_KEYS[:spec.n_prefix]]
    return torch.cat(prefix + [patch_rows(x, sd, spec)], 1) + sd["pos_embed"].reshape(1, spec.tokens, spec.dim)


def block(x, sd, spec, i):
    k = f"blocks.{i}."
    N, T, D = x.shape
    H, dh = spec.heads, spec.dim // spec.heads
    a = layer_norm(x, sd[k + "norm1.weight"], sd[k + "norm1.bias"], spec.ln_eps)
    qkv = (a @ sd[k + "attn.qkv.weight"].T + sd[k + "attn.qkv.bias"]).reshape(N, T, 3, H, dh).permute(2, 0, 3, 1, 4)
    q, kk, v = qkv[0], qkv[1], qkv[2]                             # (N, H, T, dh): rows [q; k; v], head h at h*dh..
    att = torch.softmax((q @ kk.transpose(-2, -1)) * dh ** -0.5, dim=-1)
    o = (att @ v).transpose(1, 2).reshape(N, T, D)
    x = x + (o @ sd[k + "attn.proj.weight"].T + sd[k + "attn.proj.bias"])
    c = layer_norm(x, sd[k + "norm2.weight"], sd[k + "norm2.bias"], spec.ln_eps)
    h = gelu(c @ sd[k + "mlp.fc1.weight"].T + sd[k + "mlp.fc1.bias"])
    return x + (h @ sd[k + "mlp.fc2.weight"].T + sd[k + "mlp.fc2.bias"])


def run_blocks(t, sd, spec, hook_blocks: Sequence[int]):
    """The streams after the hooked blocks for a token sequence `t` (N, any length, dim) -- the blocks do not know the sequence's make-up."""
    outs = {}
    for i in range(max(hook_blocks) + 1):
        t = block(t, sd, spec, i)
        outs[i] = t
    return [outs[b] for b in hook_blocks]


def streams(x, sd, spec, n_blocks):
    return run_blocks(embed(x, sd, spec), sd, spec, list(range(n_blocks)))


class VitFamilyReference(StreamsReference):
    streams = staticmethod(streams)
