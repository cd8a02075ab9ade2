"""Plain-torch restatement of the ViT surrogate -- the yardstick of the ViT tests.  Written from the model's
definition (timm `VisionTransformer`, `vit_base_patch16_224`), independent of the HIP path.  It has the interface of
`oracle.restate.OracleNet` that `oracle.restate.run_attack` drives: `.dtype`, `.hooks`, `.forward(x) -> [hook features]` and
`.backward(hook_grads) -> d cost / d x`; every hook feature is (frames, tokens * dim), the residual stream after its block."""
import torch
import torch.nn.functional as F

from tests.family_harness import StreamsReference


def layer_norm(x, w, b, eps):
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)                  # biased
    return (x - mu) / torch.sqrt(var + eps) * w + b


def gelu(x):
    return 0.5 * x * (1.0 + torch.erf(x / 2 ** 0.5))              # exact form


def embed(x, sd, spec):
    """(N, 3, H, W) -> (N, tokens, dim): patch x patch convolution with stride patch, flatten, cls prepended, pos_embed added."""
    p = F.conv2d(x, sd["patch_embed.proj.weight"], sd["patch_embed.proj.bias"], stride=spec.patch)
    p = p.flatten(2).transpose(1, 2)
    cls = sd["cls_token"].reshape(1, 1, -1).expand(x.shape[0], 1, spec.dim)
    return torch.cat([cls, p], 1) + sd["pos_embed"].reshape(1, spec.tokens, spec.dim)


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


def streams(x, sd, spec, n_blocks):
    """The residual streams behind the blocks 0 .. n_blocks - 1, each (frames, tokens, dim)."""
    t, outs = embed(x, sd, spec), []
    for i in range(n_blocks):
        t = block(t, sd, spec, i)
        outs.append(t)
    return outs


class VitReference(StreamsReference):
    streams = staticmethod(streams)
