"""Architecture IR for the image backbones the attack classes hook.

The reference obtains its backbones from torchvision 0.10.1
(`/root/reference/image_attacks.py:84-108`, `TPAMI_attack.py:100-124`); torchvision
is third-party and not vendored, so the graphs are restated here from the public
architecture definitions as a flat list of nodes.  The same IR is consumed by

  * the HIP engine (`engine.py` -> `i2v_net_add_*` of the C-ABI), and
  * the CPU oracle (`oracle/restate.py`) -- test infrastructure only.

Only what lies at or before a hook layer is ever executed; everything behind the
deepest hook (layer4 / avgpool / fc / classifier tails) cannot influence the loss
(`image_attacks.py:336-347`) and is never emitted.

Tensor ids index `Graph.tensors`.  A tensor is a channel-slice *view* of a buffer
(`buf`, `c_off`, buffer width `Graph.buffers[buf]`) so that SqueezeNet Fire
concatenation needs no copy.

Weight keys follow the torchvision `state_dict` layout, so a real ImageNet
checkpoint loads unchanged when one is supplied.
"""
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence, Tuple

from .family import clamped, clamped_tail, ends, Family, fan_in_tail, keys, normal, normal_over, signed_uniform, StagedSpec, starts, TokenSpec, uniform


@dataclass
class TensorSpec:
    C: int
    H: int
    W: int
    buf: int            # buffer id
    c_off: int          # channel offset inside the buffer
    post_relu: bool     # values are outputs of a ReLU (gradient mask = value > 0)
    name: str = ""
    T: int = 1          # frames per clip (video backbones; 1 for image backbones)


@dataclass
class ConvNode:
    src: int
    dst: int
    cin: int
    cout: int
    kh: int
    kw: int
    stride: int
    pad: int
    weight: str                 # state_dict key of the conv weight
    bias: Optional[str]         # state_dict key of the conv bias (VGG/AlexNet/SqueezeNet)
    bn: Optional[str]           # state_dict prefix of the BatchNorm2d that follows (ResNet)
    relu: bool                  # ReLU applied after (bias/bn [+ residual])
    residual: Optional[int] = None   # tensor added before the ReLU (Bottleneck identity)
    pre_bn: Optional[str] = None     # DenseNet pre-activation: relu(BatchNorm(x)) applied to the conv INPUT
    op: str = "conv"
    # video backbones: temporal extent of the kernel (output frame t reads input frames t*stride_t - pad_t + q*dil_t)
    kt: int = 1
    stride_t: int = 1
    pad_t: int = 0
    dil_t: int = 1
    groups: int = 1             # grouped convolution (ResNeXt; depthwise: groups == cin == cout): the weight is (cout, cin // groups, kh, kw)


@dataclass
class PoolNode:
    src: int
    dst: int
    k: int
    stride: int
    pad: int
    ceil_mode: bool
    op: str = "maxpool"
    kt: int = 1
    stride_t: int = 1
    pad_t: int = 0


@dataclass
class AttnNode:
    """Core of a non-local block: dst[c][i] = sum_j g[c][j] softmax_j(scale * <theta[:, i], phi[:, j]>) per clip (`i2v_net_add_attention`)."""
    src: int                    # theta
    phi: int
    g: int
    dst: int
    scale: float = 1.0
    op: str = "attention"

    @property
    def extra_srcs(self):
        return (self.phi, self.g)


@dataclass
class SENode:
    """Squeeze-and-excitation with the block's shortcut add and final ReLU (`i2v_net_add_se`; timm 0.5.0 `SEModule`):
    dst = act(src * sigmoid(fc2(relu(fc1(mean_hw src)))) + residual).  `fc1` / `fc2` are state_dict prefixes of 1x1 convolutions
    with bias: `{fc1}.weight` (rd, C, 1, 1), `{fc2}.weight` (C, rd, 1, 1)."""
    src: int
    dst: int
    C: int
    rd: int
    fc1: str
    fc2: str
    relu: bool
    residual: Optional[int] = None
    op: str = "se"


@dataclass
class Graph:
    arch: str
    in_hw: Tuple[int, int]
    tensors: List[TensorSpec] = field(default_factory=list)
    buffers: List[int] = field(default_factory=list)          # channel width per buffer
    nodes: list = field(default_factory=list)
    hooks: Dict[int, int] = field(default_factory=dict)       # depth (1..4) -> tensor id
    # depth -> tensor id of the WHOLE hooked module's output where that differs from `hooks[depth]`: the list-depth
    # lookup of the adaptive attack hooks the Fire module itself (TPAMI_attack.py:195-197), i.e. cat(expand1x1,
    # expand3x3), while the scalar-depth lookup takes `.expand3x3_activation` only (:199, image_attacks.py:269-271)
    hooks_module: Dict[int, int] = field(default_factory=dict)
    input: int = 0
    video: bool = False                                       # 3-D backbone: conv weights are (cout,cin,kt,kh,kw)
    classifier_feats: List[int] = field(default_factory=list)  # tensors a classifier head pools and concatenates (video graphs built to their last stage)

    # -- construction helpers -------------------------------------------------
    def new_buffer(self, C: int) -> int:
        self.buffers.append(C)
        return len(self.buffers) - 1

    def new_tensor(self, C, H, W, post_relu, name="", buf=None, c_off=0, T=1) -> int:
        if buf is None:
            buf = self.new_buffer(C)
        self.tensors.append(TensorSpec(C, H, W, buf, c_off, post_relu, name, T))
        return len(self.tensors) - 1

    def conv(self, src, cout, k, stride, pad, weight, bias=None, bn=None, relu=True,
             residual=None, name="", dst_buf=None, dst_c_off=0, pre_bn=None, groups=1) -> int:
        s = self.tensors[src]
        assert s.C % groups == 0 and cout % groups == 0, "channels must be divisible by groups"
        Ho = (s.H + 2 * pad - k) // stride + 1
        Wo = (s.W + 2 * pad - k) // stride + 1
        dst = self.new_tensor(cout, Ho, Wo, relu, name, dst_buf, dst_c_off)
        assert pre_bn is None or (k == 1 and stride == 1 and pad == 0), "pre-activation only on 1x1 convs"
        self.nodes.append(ConvNode(src, dst, s.C, cout, k, k, stride, pad, weight, bias, bn,
                                   relu, residual, pre_bn, groups=groups))
        return dst

    def maxpool(self, src, k, stride, pad=0, ceil_mode=False, name="", dst_buf=None, dst_c_off=0, op="maxpool") -> int:
        s = self.tensors[src]

        def out(n):
            if ceil_mode:
                o = -(-(n + 2 * pad - k) // stride) + 1
                if (o - 1) * stride >= n + pad:     # last window must start inside the input
                    o -= 1
            else:
                o = (n + 2 * pad - k) // stride + 1
            return o
        dst = self.new_tensor(s.C, out(s.H), out(s.W), False, name, dst_buf, dst_c_off)
        self.nodes.append(PoolNode(src, dst, k, stride, pad, ceil_mode, op))
        return dst

    def avgpool(self, src, k, stride, name="", dst_buf=None, dst_c_off=0) -> int:
        return self.maxpool(src, k, stride, 0, False, name, dst_buf, dst_c_off, op="avgpool")

    def conv3d(self, src, cout, k, stride, pad, weight, bn=None, relu=True, residual=None, name="",
               dst_buf=None, dst_c_off=0, dil_t=1, bias=None) -> int:
        """k / stride / pad are (temporal, spatial) pairs, as in `nn.Conv3d((kt,k,k), (st,s,s), (pt,p,p))`."""
        (kt, ks), (st, ss), (pt, ps) = k, stride, pad
        s = self.tensors[src]
        To = (s.T + 2 * pt - dil_t * (kt - 1) - 1) // st + 1
        Ho = (s.H + 2 * ps - ks) // ss + 1
        Wo = (s.W + 2 * ps - ks) // ss + 1
        dst = self.new_tensor(cout, Ho, Wo, relu, name, dst_buf, dst_c_off, T=To)
        self.nodes.append(ConvNode(src, dst, s.C, cout, ks, ks, ss, ps, weight, bias, bn, relu, residual, None,
                                   "conv", kt, st, pt, dil_t))
        return dst

    def se(self, src, rd, prefix, relu=True, residual=None, name="") -> int:
        """A squeeze-and-excitation node over `src` (the linear output of a convolution) with keys `{prefix}.fc1.*` / `{prefix}.fc2.*`."""
        s = self.tensors[src]
        assert not s.post_relu and s.T == 1 and rd >= 1
        dst = self.new_tensor(s.C, s.H, s.W, relu, name)
        self.nodes.append(SENode(src, dst, s.C, rd, f"{prefix}.fc1", f"{prefix}.fc2", relu, residual))
        return dst

    def attention(self, theta, phi, gg, name="", scale=1.0) -> int:
        t = self.tensors[theta]
        assert t.C == self.tensors[phi].C == self.tensors[gg].C
        dst = self.new_tensor(t.C, t.H, t.W, False, name, T=t.T)
        self.nodes.append(AttnNode(theta, phi, gg, dst, scale))
        return dst

    def nonlocal_block(self, x, prefix) -> int:
        """gluoncv / mmaction `NonLocalModule` (embedded gaussian, sub-sampled, with BatchNorm): theta = conv1x1x1(x); phi, g =
        conv1x1x1(maxpool 1x2x2 (x)); y = g softmax(theta^T phi)^T; z = BN(W y) + x.  Node order matters to the planner: a
        convolution (theta) must be the LAST contributor to x's gradient, i.e. the first consumer listed."""
        c = self.tensors[x].C
        e = c // 2
        theta = self.conv3d(x, e, (1, 1), (1, 1), (0, 0), f"{prefix}.theta.weight", relu=False, name=f"{prefix}.theta", bias=f"{prefix}.theta.bias")
        xp = self.maxpool3d(x, (1, 2), (1, 2), (0, 0), name=f"{prefix}.max_pool")
        phi = self.conv3d(xp, e, (1, 1), (1, 1), (0, 0), f"{prefix}.phi.1.weight", relu=False, name=f"{prefix}.phi", bias=f"{prefix}.phi.1.bias")
        gg = self.conv3d(xp, e, (1, 1), (1, 1), (0, 0), f"{prefix}.g.1.weight", relu=False, name=f"{prefix}.g", bias=f"{prefix}.g.1.bias")
        y = self.attention(theta, phi, gg, name=f"{prefix}.y")
        return self.conv3d(y, c, (1, 1), (1, 1), (0, 0), f"{prefix}.W.0.weight", bn=f"{prefix}.W.1", relu=False, residual=x,
                           name=f"{prefix}.out", bias=f"{prefix}.W.0.bias")

    def maxpool3d(self, src, k, stride, pad=(0, 0), name="") -> int:
        (kt, ks), (st, ss), (pt, ps) = k, stride, pad
        s = self.tensors[src]
        dst = self.new_tensor(s.C, (s.H + 2 * ps - ks) // ss + 1, (s.W + 2 * ps - ks) // ss + 1, False, name,
                              T=(s.T + 2 * pt - kt) // st + 1)
        self.nodes.append(PoolNode(src, dst, ks, ss, ps, False, "maxpool", kt, st, pt))
        return dst

    # -- analysis -------------------------------------------------------------
    def truncated(self, hook_tensors: List[int]) -> "Graph":
        """Copy of the graph holding only the nodes some hook tensor depends on."""
        needed_bufs = set()
        keep = [False] * len(self.nodes)
        needed = set(hook_tensors)
        for i in range(len(self.nodes) - 1, -1, -1):
            nd = self.nodes[i]
            d = self.tensors[nd.dst]
            hit = nd.dst in needed or any(
                self.tensors[t].buf == d.buf and _overlap(self.tensors[t], d) for t in needed)
            if hit:
                keep[i] = True
                needed.add(nd.src)
                needed.update(getattr(nd, "extra_srcs", ()))
                if getattr(nd, "residual", None) is not None:
                    needed.add(nd.residual)
        g = Graph(self.arch, self.in_hw, self.tensors, self.buffers,
                  [n for n, k in zip(self.nodes, keep) if k], dict(self.hooks), dict(self.hooks_module), self.input,
                  self.video, list(self.classifier_feats))
        return g

    def hook_for(self, depth: int, whole_module: bool = False) -> int:
        """Hooked tensor of `depth`; `whole_module` selects the list-depth lookup of `AENS_I2V_MF`
        (`/root/reference/TPAMI_attack.py:176-200`), which differs from the scalar one for SqueezeNet only."""
        if depth not in self.hooks:
            raise KeyError(depth)
        return self.hooks_module.get(depth, self.hooks[depth]) if whole_module else self.hooks[depth]

    def macs_per_frame(self) -> int:
        """Multiply-adds of one forward pass per input frame (image backbones) / per input CLIP (video)."""
        tot = 0
        for nd in self.nodes:
            if nd.op == "conv":
                d = self.tensors[nd.dst]
                tot += d.T * d.H * d.W * nd.cout * (nd.cin // nd.groups) * nd.kt * nd.kh * nd.kw
            elif nd.op == "attention":          # theta^T phi and g P^T
                t, k = self.tensors[nd.src], self.tensors[nd.phi]
                tot += 2 * t.C * (t.T * t.H * t.W) * (k.T * k.H * k.W)
            elif nd.op == "se":                 # fc1 and fc2 on the squeezed vector; nothing per position
                tot += 2 * nd.C * nd.rd
        return tot

    def param_shapes(self) -> Dict[str, Tuple[int, ...]]:
        """state_dict key -> shape for every parameter the nodes reference."""
        out = {}
        for nd in self.nodes:
            if nd.op == "se":
                out[nd.fc1 + ".weight"], out[nd.fc1 + ".bias"] = (nd.rd, nd.C, 1, 1), (nd.rd,)
                out[nd.fc2 + ".weight"], out[nd.fc2 + ".bias"] = (nd.C, nd.rd, 1, 1), (nd.C,)
            if nd.op != "conv":
                continue
            out[nd.weight] = (nd.cout, nd.cin, nd.kt, nd.kh, nd.kw) if self.video else (nd.cout, nd.cin // nd.groups, nd.kh, nd.kw)
            if nd.bias:
                out[nd.bias] = (nd.cout,)
            if nd.bn:
                for s in ("weight", "bias", "running_mean", "running_var"):
                    out[f"{nd.bn}.{s}"] = (nd.cout,)
            if nd.pre_bn:
                for s in ("weight", "bias", "running_mean", "running_var"):
                    out[f"{nd.pre_bn}.{s}"] = (nd.cin,)
        return out


def _overlap(a: TensorSpec, b: TensorSpec) -> bool:
    return a.c_off < b.c_off + b.C and b.c_off < a.c_off + a.C


# ---------------------------------------------------------------------------
# The torchvision ResNet family: ResNet-18 ... -152, Wide ResNet, ResNeXt (v1.5: the stride sits on the 3x3)
# ---------------------------------------------------------------------------
def se_reduced_width(C: int) -> int:
    """timm's `make_divisible(C / 16, 8, round_limit=0.)`: the squeezed width of `SEModule(C)` with its defaults."""
    return max(8, int(C / 16 + 4) // 8 * 8)


def resnet(layers=(3, 4, 23, 3), width=64, in_hw=(224, 224), arch="resnet101", block="bottleneck", groups=1,
           width_per_group=64, se=False) -> Graph:
    """torchvision `ResNet(block, layers, groups=, width_per_group=)` up to `layer4`.  Hook d = output of `layer{d}[-1]` (post-ReLU),
    as in `/root/reference/image_attacks.py:261-262`.
      bottleneck: conv1 1x1 inplanes -> w, conv2 3x3 / stride / `groups` w -> w, conv3 1x1 w -> 4 planes (+ shortcut, ReLU) with
                  w = int(planes * width_per_group / 64) * groups (Wide ResNet: width_per_group 128; ResNeXt: groups 32);
      basic:      conv1 3x3 / stride -> BN -> ReLU, conv2 3x3 -> BN (+ shortcut, ReLU), expansion 1.
    `width` scales every stage (64 for the real nets; the test-size twins use less).
    `se`: timm's SE-ResNet / SE-ResNeXt -- the block's last convolution + BN stays linear and a squeeze-and-excitation node `{p}.se`
    (squeezed width `se_reduced_width`) scales it, adds the shortcut and applies the ReLU; the hook is that node's output."""
    assert block in ("bottleneck", "basic")
    expansion = 4 if block == "bottleneck" else 1
    g = Graph(arch, in_hw)
    x = g.new_tensor(3, in_hw[0], in_hw[1], False, "input")
    g.input = x
    x = g.conv(x, width, 7, 2, 3, "conv1.weight", bn="bn1", relu=True, name="stem")
    x = g.maxpool(x, 3, 2, 1, name="maxpool")
    inplanes = width
    for li, nblocks in enumerate(layers):
        planes = width * (2 ** li)
        for b in range(nblocks):
            stride = 2 if (b == 0 and li > 0) else 1
            p = f"layer{li + 1}.{b}"
            project = stride != 1 or inplanes != planes * expansion
            if block == "bottleneck":
                w = int(planes * width_per_group / 64) * groups
                a = g.conv(x, w, 1, 1, 0, f"{p}.conv1.weight", bn=f"{p}.bn1", relu=True, name=f"{p}.conv1")
                a = g.conv(a, w, 3, stride, 1, f"{p}.conv2.weight", bn=f"{p}.bn2", relu=True, name=f"{p}.conv2", groups=groups)
            else:
                a = g.conv(x, planes, 3, stride, 1, f"{p}.conv1.weight", bn=f"{p}.bn1", relu=True, name=f"{p}.conv1")
            # the projection shortcut is emitted AFTER conv1/conv2: in the reversed (gradient)
            # order its input-gradient is then a pending addend of conv1's, which finalises x
            if project:
                idt = g.conv(x, planes * expansion, 1, stride, 0, f"{p}.downsample.0.weight",
                             bn=f"{p}.downsample.1", relu=False, name=f"{p}.downsample")
            else:
                idt = x
            if se:
                if block == "bottleneck":
                    a = g.conv(a, planes * 4, 1, 1, 0, f"{p}.conv3.weight", bn=f"{p}.bn3", relu=False, name=f"{p}.conv3")
                else:
                    a = g.conv(a, planes, 3, 1, 1, f"{p}.conv2.weight", bn=f"{p}.bn2", relu=False, name=f"{p}.conv2")
                x = g.se(a, se_reduced_width(planes * expansion), f"{p}.se", relu=True, residual=idt, name=f"{p}.out")
            elif block == "bottleneck":
                x = g.conv(a, planes * 4, 1, 1, 0, f"{p}.conv3.weight", bn=f"{p}.bn3", relu=True, residual=idt, name=f"{p}.out")
            else:
                x = g.conv(a, planes, 3, 1, 1, f"{p}.conv2.weight", bn=f"{p}.bn2", relu=True, residual=idt, name=f"{p}.out")
            inplanes = planes * expansion
        g.hooks[li + 1] = x
    return g


#: the torchvision names `build` serves through `resnet()`: name -> (block, layers, groups, width_per_group).  `arch` is the name.
RESNET_FAMILY: Dict[str, Tuple[str, Tuple[int, ...], int, int]] = {
    "resnet18": ("basic", (2, 2, 2, 2), 1, 64),
    "resnet34": ("basic", (3, 4, 6, 3), 1, 64),
    "resnet152": ("bottleneck", (3, 8, 36, 3), 1, 64),
    "wide_resnet50_2": ("bottleneck", (3, 4, 6, 3), 1, 128),
    "wide_resnet101_2": ("bottleneck", (3, 4, 23, 3), 1, 128),
    "resnext50_32x4d": ("bottleneck", (3, 4, 6, 3), 32, 4),
    "resnext101_32x8d": ("bottleneck", (3, 4, 23, 3), 32, 8),
}


#: timm's SE-ResNets and SE-ResNeXts `build` serves through `resnet(se=True)`: name -> (block, layers, groups, width_per_group).  `arch`
#: and the checkpoint file are the timm name; the keys are timm's (`layer{i}.{j}.se.fc1.weight` ...).
SERESNET_FAMILY: Dict[str, Tuple[str, Tuple[int, ...], int, int]] = {
    "seresnet18": ("basic", (2, 2, 2, 2), 1, 64),
    "seresnet34": ("basic", (3, 4, 6, 3), 1, 64),
    "seresnet50": ("bottleneck", (3, 4, 6, 3), 1, 64),
    "seresnet101": ("bottleneck", (3, 4, 23, 3), 1, 64),
    "seresnet152": ("bottleneck", (3, 8, 36, 3), 1, 64),
    "seresnext50_32x4d": ("bottleneck", (3, 4, 6, 3), 32, 4),
    "seresnext101_32x4d": ("bottleneck", (3, 4, 23, 3), 32, 4),
    "seresnext101_32x8d": ("bottleneck", (3, 4, 23, 3), 32, 8),
}
#: names of the line that are not served, each with what it still needs (matched by prefix, the longest first)
SE_NOT_SERVED = (("legacy_senet154", "legacy_senet154 needs the grouped 3x3 convolution at group width 8 with a different (three-convolution) stem"),
                 ("legacy_se", "the legacy_se* nets are the original SENet port, with a block, stem and key layout of their own that is not restated here"),
                 ("senet", "senet154 needs the grouped 3x3 convolution at group width 8 with a different (three-convolution) stem"))


def is_seresnet_name(model_name: str) -> bool:
    return model_name in SERESNET_FAMILY or model_name.startswith(("seresne", "legacy_se", "senet"))


def seresnet_named(model_name: str, in_hw=(224, 224)) -> Graph:
    if model_name in SERESNET_FAMILY:
        block, layers, groups, wpg = SERESNET_FAMILY[model_name]
        return resnet(layers, 64, in_hw, model_name, block, groups, wpg, se=True)
    why = ""
    if model_name.startswith("seresne") and model_name.split("_")[0].endswith(("d", "t")) and model_name.split("_")[0][-2].isdigit():
        why = ": the d / t deep-stem variants need the three-convolution stem and the average-pool downsample"
    for prefix, reason in SE_NOT_SERVED:
        if not why and model_name.startswith(prefix):
            why = ": " + reason
    raise ValueError(f"{model_name!r} is not served{why}; the squeeze-and-excitation names served: " + ", ".join(SERESNET_FAMILY))


# ---------------------------------------------------------------------------
# torchvision MNASNet (`_version` 2): depthwise-separable inverted residuals
# ---------------------------------------------------------------------------
#: name -> alpha.  `arch` and the checkpoint file are the torchvision name.
MNASNET_MODELS: Dict[str, float] = {"mnasnet0_5": 0.5, "mnasnet0_75": 0.75, "mnasnet1_0": 1.0, "mnasnet1_3": 1.3}
#: torchvision's stacks `layers.8 .. layers.13`: (kernel, stride, expansion, repeats)
MNASNET_STACKS = ((3, 2, 3, 3), (5, 2, 3, 3), (5, 2, 6, 3), (3, 1, 6, 2), (5, 2, 6, 4), (3, 1, 6, 1))
#: depth d -> the stack hooked: the last block at ResNet's stride for that depth (4, 8, 16, 32)
MNASNET_HOOKS = {1: 8, 2: 9, 3: 11, 4: 13}


def _round_to_multiple_of(val, divisor, round_up_bias=0.9):
    new_val = max(divisor, int(val + divisor / 2) // divisor * divisor)
    return new_val if new_val >= round_up_bias * val else new_val + divisor


def mnasnet_depths(alpha: float) -> List[int]:
    return [_round_to_multiple_of(d * alpha, 8) for d in (32, 16, 24, 40, 80, 96, 192, 320)]


def mnasnet(alpha=1.0, in_hw=(224, 224), arch="mnasnet1_0", depths=None, stacks=MNASNET_STACKS) -> Graph:
    """torchvision `MNASNet(alpha)` up to `layers.13`.  Stem `layers.0-2` 3x3 / 2 + BN + ReLU, `layers.3-5` depthwise 3x3 + BN + ReLU,
    `layers.6-7` 1x1 + BN (linear); then six stacks of `_InvertedResidual`: 1x1 expand + ReLU, depthwise k x k / stride + ReLU, 1x1
    project (linear), + the block's input when `in == out and stride == 1`.  Hook d = output of stack `MNASNET_HOOKS[d]` (a linear
    tensor: `post_relu` false).  `depths` / `stacks` override the widths and the stack table (the test-size twin)."""
    depths = list(depths) if depths is not None else mnasnet_depths(alpha)
    g = Graph(arch, in_hw)
    x = g.new_tensor(3, in_hw[0], in_hw[1], False, "input")
    g.input = x
    x = g.conv(x, depths[0], 3, 2, 1, "layers.0.weight", bn="layers.1", relu=True, name="layers.0")
    x = g.conv(x, depths[0], 3, 1, 1, "layers.3.weight", bn="layers.4", relu=True, name="layers.3", groups=depths[0])
    x = g.conv(x, depths[1], 1, 1, 0, "layers.6.weight", bn="layers.7", relu=False, name="layers.6")
    cin = depths[1]
    hook_of = {v: k for k, v in MNASNET_HOOKS.items()}
    for si, (k, stride, exp, repeats) in enumerate(stacks):
        cout = depths[si + 2]
        for b in range(repeats):
            p = f"layers.{si + 8}.{b}.layers"
            s = stride if b == 0 else 1
            mid = cin * exp
            a = g.conv(x, mid, 1, 1, 0, f"{p}.0.weight", bn=f"{p}.1", relu=True, name=f"{p}.0")
            a = g.conv(a, mid, k, s, k // 2, f"{p}.3.weight", bn=f"{p}.4", relu=True, name=f"{p}.3", groups=mid)
            x = g.conv(a, cout, 1, 1, 0, f"{p}.6.weight", bn=f"{p}.7", relu=False, residual=x if (cin == cout and s == 1) else None,
                       name=f"layers.{si + 8}.{b}")
            cin = cout
        if si + 8 in hook_of:
            g.hooks[hook_of[si + 8]] = x
    return g


def is_mnasnet_name(model_name: str) -> bool:
    return model_name in MNASNET_MODELS or model_name.startswith("mnasnet")


#: mobile-class families that are not served yet, each with the ingredient it still needs on top of the depthwise kernel
MOBILE_NOT_SERVED = (("mobilenet", "MobileNetV2 / V3 need a capped ReLU (ReLU6) and hard-swish, with their gates, in the convolution epilogue"),
                     ("shufflenet", "ShuffleNetV2 needs channel shuffle and split"),
                     ("efficientnet", "EfficientNet needs SiLU and squeeze-excite"))


def mnasnet_named(model_name: str, in_hw=(224, 224)) -> Graph:
    if model_name not in MNASNET_MODELS:
        raise ValueError(f"MNASNet surrogate {model_name!r}: not a torchvision MNASNet; served: " + ", ".join(MNASNET_MODELS))
    return mnasnet(MNASNET_MODELS[model_name], in_hw, model_name)


# ---------------------------------------------------------------------------
# VGG-16 `features`
# ---------------------------------------------------------------------------
VGG16_CFG = (64, 64, "M", 128, 128, "M", 256, 256, 256, "M", 512, 512, 512, "M", 512, 512, 512, "M")


def vgg(cfg=VGG16_CFG, in_hw=(224, 224), arch="vgg16", hook_index=None) -> Graph:
    """Hook d = ReLU module `features[{1:1,2:11,3:20,4:29}[d]]`
    (`/root/reference/image_attacks.py:266-268`)."""
    g = Graph(arch, in_hw)
    x = g.new_tensor(3, in_hw[0], in_hw[1], False, "input")
    g.input = x
    idx = 0
    relu_at = {}
    for v in cfg:
        if v == "M":
            x = g.maxpool(x, 2, 2, 0, name=f"features.{idx}")
            idx += 1
        else:
            x = g.conv(x, v, 3, 1, 1, f"features.{idx}.weight", bias=f"features.{idx}.bias",
                       relu=True, name=f"features.{idx + 1}")
            relu_at[idx + 1] = x
            idx += 2
    hook_index = hook_index or {1: 1, 2: 11, 3: 20, 4: 29}
    for d, i in hook_index.items():
        if i in relu_at:
            g.hooks[d] = relu_at[i]
    return g


# ---------------------------------------------------------------------------
# AlexNet `features`
# ---------------------------------------------------------------------------
def alexnet(width_div=1, in_hw=(224, 224), arch="alexnet") -> Graph:
    """Hook d = ReLU module `features[{1:1,2:4,3:7,4:11}[d]]`
    (`/root/reference/image_attacks.py:263-265`)."""
    c = [max(4, v // width_div) for v in (64, 192, 384, 256, 256)]
    g = Graph(arch, in_hw)
    x = g.new_tensor(3, in_hw[0], in_hw[1], False, "input")
    g.input = x
    x = g.conv(x, c[0], 11, 4, 2, "features.0.weight", bias="features.0.bias", name="features.1")
    g.hooks[1] = x
    x = g.maxpool(x, 3, 2, 0, name="features.2")
    x = g.conv(x, c[1], 5, 1, 2, "features.3.weight", bias="features.3.bias", name="features.4")
    g.hooks[2] = x
    x = g.maxpool(x, 3, 2, 0, name="features.5")
    x = g.conv(x, c[2], 3, 1, 1, "features.6.weight", bias="features.6.bias", name="features.7")
    g.hooks[3] = x
    x = g.conv(x, c[3], 3, 1, 1, "features.8.weight", bias="features.8.bias", name="features.9")
    x = g.conv(x, c[4], 3, 1, 1, "features.10.weight", bias="features.10.bias", name="features.11")
    g.hooks[4] = x
    return g


# ---------------------------------------------------------------------------
# SqueezeNet 1.1 `features`
# ---------------------------------------------------------------------------
def squeezenet(width_div=1, in_hw=(224, 224), arch="squeezenet1_1") -> Graph:
    """Hook d = `features[{1:3,2:6,3:9,4:12}[d]].expand3x3_activation`, i.e. only the
    3x3 branch of the Fire module (`/root/reference/image_attacks.py:269-271`)."""
    def ch(v):
        return max(4, v // width_div)
    g = Graph(arch, in_hw)
    x = g.new_tensor(3, in_hw[0], in_hw[1], False, "input")
    g.input = x
    x = g.conv(x, ch(64), 3, 2, 0, "features.0.weight", bias="features.0.bias", name="features.1")
    x = g.maxpool(x, 3, 2, 0, ceil_mode=True, name="features.2")
    fires = {3: (16, 64, 64), 4: (16, 64, 64), 6: (32, 128, 128), 7: (32, 128, 128),
             9: (48, 192, 192), 10: (48, 192, 192), 11: (64, 256, 256), 12: (64, 256, 256)}
    hook_of = {3: 1, 6: 2, 9: 3, 12: 4}
    for idx in range(3, 13):
        if idx in (5, 8):
            x = g.maxpool(x, 3, 2, 0, ceil_mode=True, name=f"features.{idx}")
            continue
        sq, e1, e3 = (ch(v) for v in fires[idx])
        p = f"features.{idx}"
        s = g.conv(x, sq, 1, 1, 0, f"{p}.squeeze.weight", bias=f"{p}.squeeze.bias",
                   name=f"{p}.squeeze_activation")
        st = g.tensors[s]
        cat_buf = g.new_buffer(e1 + e3)
        g.conv(s, e1, 1, 1, 0, f"{p}.expand1x1.weight", bias=f"{p}.expand1x1.bias",
               name=f"{p}.expand1x1_activation", dst_buf=cat_buf, dst_c_off=0)
        t3 = g.conv(s, e3, 3, 1, 1, f"{p}.expand3x3.weight", bias=f"{p}.expand3x3.bias",
                    name=f"{p}.expand3x3_activation", dst_buf=cat_buf, dst_c_off=e1)
        x = g.new_tensor(e1 + e3, st.H, st.W, True, f"{p}.cat", buf=cat_buf, c_off=0)
        if idx in hook_of:
            g.hooks[hook_of[idx]] = t3
            g.hooks_module[hook_of[idx]] = x
    return g


# ---------------------------------------------------------------------------
# DenseNet-BC (torchvision `densenet121` / `densenet161`) -- extension, see `build`
# ---------------------------------------------------------------------------
def densenet(growth=32, block_config=(6, 12, 24, 16), init_features=64, bn_size=4, in_hw=(224, 224),
             arch="densenet121") -> Graph:
    """Hook d = output of `features.denseblock{d}` (the raw concatenation, not a ReLU output) -- the
    only hint the reference gives for DenseNet (`image_attacks.py:98-99`).  A dense block is ONE buffer:
    layer l reads its first C_l channels through BN+ReLU (pre-activation, folded into the 1x1 conv's
    operand read) and appends `growth` channels."""
    g = Graph(arch, in_hw)
    x = g.new_tensor(3, in_hw[0], in_hw[1], False, "input")
    g.input = x
    x = g.conv(x, init_features, 7, 2, 3, "features.conv0.weight", bn="features.norm0", relu=True, name="features.relu0")
    C = init_features
    pending_pool = ("max", x)
    for bi, nlayers in enumerate(block_config):
        total = C + nlayers * growth
        cb = g.new_buffer(total)
        kind, src = pending_pool
        if kind == "max":
            v = g.maxpool(src, 3, 2, 1, name="features.pool0", dst_buf=cb, dst_c_off=0)
        else:
            v = g.avgpool(src, 2, 2, name=f"features.transition{bi}.pool", dst_buf=cb, dst_c_off=0)
        H, W = g.tensors[v].H, g.tensors[v].W
        for li in range(nlayers):
            p = f"features.denseblock{bi + 1}.denselayer{li + 1}"
            view = g.new_tensor(C, H, W, False, f"{p}.in", buf=cb, c_off=0)
            a = g.conv(view, bn_size * growth, 1, 1, 0, f"{p}.conv1.weight", bn=f"{p}.norm2", relu=True,
                       name=f"{p}.relu2", pre_bn=f"{p}.norm1")
            g.conv(a, growth, 3, 1, 1, f"{p}.conv2.weight", relu=False, name=f"{p}.conv2", dst_buf=cb, dst_c_off=C)
            C += growth
        full = g.new_tensor(C, H, W, False, f"features.denseblock{bi + 1}", buf=cb, c_off=0)
        g.hooks[bi + 1] = full
        if bi != len(block_config) - 1:
            p = f"features.transition{bi + 1}"
            t = g.conv(full, C // 2, 1, 1, 0, f"{p}.conv.weight", relu=False, name=f"{p}.conv", pre_bn=f"{p}.norm")
            C //= 2
            pending_pool = ("avg", t)
    return g


# ---------------------------------------------------------------------------
# Video backbones: the white-box models ILAF fine-tunes against (`image_attacks.py:513-519`).
# The reference takes them from gluoncv 0.10.4 (`image_fine_tune_attack.py:63`, configs `utils.py:9-14`), which is
# not vendored and not installed; the graphs below restate the PUBLIC architectures (I3D: Carreira & Zisserman /
# Wang et al. "3x1x1" inflation; SlowFast: Feichtenhofer et al.) up to the hooked stage.  Parity with gluoncv's
# exact module layout and checkpoints is therefore UNPINNED; what is pinned is the arithmetic of every node
# against `torch.nn.functional.conv3d / max_pool3d` (oracle/video_models.py).  The non-local blocks of the `i3d_nl5_*`
# configs ARE built (`NL5_FREQ` below, the attention core behind `i2v_net_add_attention`): `'i3d_resnet50'` is that
# network, `'i3d_plain_resnet50'` the one without them.  Not built: TPN's pyramid neck and heads (its ResNet backbone is).
# ---------------------------------------------------------------------------
NL5_FREQ = ((0, 0, 0), (0, 1, 0, 1), (0, 1, 0, 1, 0, 1), (0, 0, 0))     # gluoncv i3d_nl5: non-local blocks behind blocks 1, 3 of res3 and 1, 3, 5 of res4


def i3d_resnet(layers=(3, 4, 6, 3), width=64, in_thw=(32, 224, 224), arch="i3d_resnet50",
               inflate=((1, 1, 1), (1, 0, 1, 0), (1, 0, 1, 0, 1, 0), (0, 1, 0)), nonlocal_freq=None) -> Graph:
    """Inflated Bottleneck ResNet: stem 5x7x7 / (2,2,2), max-pool 1x3x3 / (2,2,2), pool2 2x1x1 after the first
    stage, `inflate[stage][block] == 1` turns that block's first 1x1x1 convolution into 3x1x1.  `hooks[d]` is the
    output of stage d; the reference hooks `res_layers._modules['1']`, i.e. d = 2 (`image_attacks.py:514`).
    `nonlocal_freq[stage][block] == 1` appends a non-local block to that Bottleneck (`Graph.nonlocal_block`): the reference's I3D
    configurations are gluoncv's `i3d_nl5_resnet50/101_v1` (`utils.py:9-10`), NL5_FREQ; for the 101-layer net the pattern of
    res4 repeats over its 23 blocks' first six only (gluoncv lists five blocks in all)."""
    T, H, W = in_thw
    g = Graph(arch, (H, W), video=True)
    x = g.new_tensor(3, H, W, False, "input", T=T)
    g.input = x
    x = g.conv3d(x, width, (5, 7), (2, 2), (2, 3), "conv1.weight", bn="bn1", name="stem")
    x = g.maxpool3d(x, (1, 3), (2, 2), (0, 1), name="maxpool")
    inplanes = width
    for li, nblocks in enumerate(layers):
        planes = width * (2 ** li)
        for b in range(nblocks):
            stride = 2 if (b == 0 and li > 0) else 1
            p = f"res_layers.{li}.{b}"
            infl = inflate[li][b % len(inflate[li])] if li < len(inflate) else 0
            a = g.conv3d(x, planes, (3, 1) if infl else (1, 1), (1, 1), (1, 0) if infl else (0, 0),
                         f"{p}.conv1.weight", bn=f"{p}.bn1", name=f"{p}.conv1")
            a = g.conv3d(a, planes, (1, 3), (1, stride), (0, 1), f"{p}.conv2.weight", bn=f"{p}.bn2", name=f"{p}.conv2")
            if stride != 1 or inplanes != planes * 4:
                idt = g.conv3d(x, planes * 4, (1, 1), (1, stride), (0, 0), f"{p}.downsample.0.weight",
                               bn=f"{p}.downsample.1", relu=False, name=f"{p}.downsample")
            else:
                idt = x
            x = g.conv3d(a, planes * 4, (1, 1), (1, 1), (0, 0), f"{p}.conv3.weight", bn=f"{p}.bn3", residual=idt,
                         name=f"{p}.out")
            if nonlocal_freq is not None and li < len(nonlocal_freq) and b < len(nonlocal_freq[li]) and nonlocal_freq[li][b]:
                x = g.nonlocal_block(x, f"{p}.nonlocal_block")
            inplanes = planes * 4
        g.hooks[li + 1] = x
        if li == 0:
            x = g.maxpool3d(x, (2, 1), (2, 1), (0, 0), name="pool2")
    return g


def slowfast_res2(width=64, in_thw=(32, 224, 224), arch="slowfast_resnet50", slow_stride=8, fast_stride=1,
                  beta_inv=8, fusion_ratio=2, fusion_kernel=5, blocks=3) -> Graph:
    """SlowFast up to its `res2` stages, the two tensors the reference hooks (`image_attacks.py:515-516`):
    hooks[1] = slow_res2, hooks[2] = fast_res2, in the order their forward hooks fire (the fast pathway runs first).
    The pathway inputs `x[:, :, ::stride]` are expressed as temporal stride / dilation of the stem convolutions,
    so both stems read the same frame tensor."""
    T, H, W = in_thw
    alpha = slow_stride // fast_stride
    fw = width // beta_inv
    g = Graph(arch, (H, W), video=True)
    x = g.new_tensor(3, H, W, False, "input", T=T)
    g.input = x
    # fast pathway: conv 5x7x7 over every `fast_stride`-th frame
    f = g.conv3d(x, fw, (5, 7), (fast_stride, 2), (2 * fast_stride, 3), "fast_conv1.weight", bn="fast_bn1",
                 name="fast_stem", dil_t=fast_stride)
    f = g.maxpool3d(f, (1, 3), (1, 2), (0, 1), name="fast_maxpool")
    # slow pathway: conv 1x7x7 over every `slow_stride`-th frame, concatenated with the lateral connection
    ft = g.tensors[f]
    cat = g.new_buffer(width + fw * fusion_ratio)
    s = g.conv3d(x, width, (1, 7), (slow_stride, 2), (0, 3), "slow_conv1.weight", bn="slow_bn1", name="slow_stem")
    st = g.tensors[s]
    sp_t = g.new_tensor(width, ft.H, ft.W, False, "slow_maxpool", buf=cat, c_off=0, T=st.T)
    g.nodes.append(PoolNode(s, sp_t, 3, 2, 1, False, "maxpool", 1, 1, 0))
    lat_t = g.new_tensor(fw * fusion_ratio, ft.H, ft.W, True, "lateral_p1", buf=cat, c_off=width, T=st.T)
    g.nodes.append(ConvNode(f, lat_t, fw, fw * fusion_ratio, 1, 1, 1, 0, "lateral_p1.0.weight", None, "lateral_p1.1",
                            True, None, None, "conv", fusion_kernel, alpha, fusion_kernel // 2, 1))
    assert (ft.T + 2 * (fusion_kernel // 2) - fusion_kernel) // alpha + 1 == st.T, "pathway frame counts disagree"
    xs = g.new_tensor(width + fw * fusion_ratio, ft.H, ft.W, False, "slow_cat", buf=cat, c_off=0, T=st.T)

    def stage(x, inplanes, planes, prefix, head_t):
        for b in range(blocks):
            p = f"{prefix}.{b}"
            a = g.conv3d(x, planes, (head_t, 1), (1, 1), (head_t // 2, 0), f"{p}.conv1.weight", bn=f"{p}.bn1", name=f"{p}.conv1")
            a = g.conv3d(a, planes, (1, 3), (1, 1), (0, 1), f"{p}.conv2.weight", bn=f"{p}.bn2", name=f"{p}.conv2")
            if inplanes != planes * 4:
                idt = g.conv3d(x, planes * 4, (1, 1), (1, 1), (0, 0), f"{p}.downsample.0.weight",
                               bn=f"{p}.downsample.1", relu=False, name=f"{p}.downsample")
            else:
                idt = x
            x = g.conv3d(a, planes * 4, (1, 1), (1, 1), (0, 0), f"{p}.conv3.weight", bn=f"{p}.bn3", residual=idt,
                         name=f"{p}.out")
            inplanes = planes * 4
        return x
    fr = stage(f, fw, fw, "fast_res2", 3)
    sr = stage(xs, width + fw * fusion_ratio, width, "slow_res2", 1)
    g.hooks[1] = fr
    g.hooks[2] = sr
    return g


def slowfast_resnet(layers=(3, 4, 6, 3), width=64, in_thw=(32, 224, 224), arch="slowfast_resnet50_full", slow_stride=8,
                    fast_stride=1, beta_inv=8, fusion_ratio=2, fusion_kernel=5) -> Graph:
    """The WHOLE SlowFast backbone (Feichtenhofer et al.; gluoncv `slowfast_4x16_resnet50/101_kinetics400`): both pathways
    through res2..res5 with a time-strided lateral convolution (5x1x1 / (alpha,1,1), BN, ReLU) from the fast into the slow
    pathway in front of every slow stage.  Slow pathway: temporal kernels only in res4 / res5; fast pathway: 3x1x1 in every
    block.  hooks[1] / hooks[2] = fast_res2 / slow_res2 as in `slowfast_res2` (same weight keys, same order), and
    `classifier_feats` = [slow_res5, fast_res5]: the head pools each over (T, H, W), concatenates them in that order and
    applies `fc` (the classifier of the white-box sign-step attacks, `attack.py:63-96`).  Parity with gluoncv's module
    layout unpinned, like the other video graphs."""
    T, H, W = in_thw
    alpha = slow_stride // fast_stride
    fw = width // beta_inv
    g = Graph(arch, (H, W), video=True)
    x = g.new_tensor(3, H, W, False, "input", T=T)
    g.input = x
    f = g.conv3d(x, fw, (5, 7), (fast_stride, 2), (2 * fast_stride, 3), "fast_conv1.weight", bn="fast_bn1",
                 name="fast_stem", dil_t=fast_stride)
    f = g.maxpool3d(f, (1, 3), (1, 2), (0, 1), name="fast_maxpool")
    ft = g.tensors[f]
    s = g.conv3d(x, width, (1, 7), (slow_stride, 2), (0, 3), "slow_conv1.weight", bn="slow_bn1", name="slow_stem")
    st = g.tensors[s]

    def lateral(src, cat, c_off, key):
        """fast feature -> 5x1x1 / alpha convolution + BN + ReLU into channels [c_off, ...) of the slow pathway's next input"""
        sp = g.tensors[src]
        t = g.new_tensor(sp.C * fusion_ratio, sp.H, sp.W, True, key, buf=cat, c_off=c_off,
                         T=(sp.T + 2 * (fusion_kernel // 2) - fusion_kernel) // alpha + 1)
        g.nodes.append(ConvNode(src, t, sp.C, sp.C * fusion_ratio, 1, 1, 1, 0, f"{key}.0.weight", None, f"{key}.1",
                                True, None, None, "conv", fusion_kernel, alpha, fusion_kernel // 2, 1))
        return t

    cat = g.new_buffer(width + fw * fusion_ratio)
    sp_t = g.new_tensor(width, ft.H, ft.W, False, "slow_maxpool", buf=cat, c_off=0, T=st.T)
    g.nodes.append(PoolNode(s, sp_t, 3, 2, 1, False, "maxpool", 1, 1, 0))
    lat = lateral(f, cat, width, "lateral_p1")
    assert g.tensors[lat].T == st.T, "pathway frame counts disagree"
    xs = g.new_tensor(width + fw * fusion_ratio, ft.H, ft.W, False, "slow_cat1", buf=cat, c_off=0, T=st.T)

    def stage(x, planes, nblocks, stride, prefix, head_t, out_buf=None):
        inplanes = g.tensors[x].C
        for b in range(nblocks):
            sb = stride if b == 0 else 1
            p = f"{prefix}.{b}"
            a = g.conv3d(x, planes, (head_t, 1), (1, 1), (head_t // 2, 0), f"{p}.conv1.weight", bn=f"{p}.bn1", name=f"{p}.conv1")
            a = g.conv3d(a, planes, (1, 3), (1, sb), (0, 1), f"{p}.conv2.weight", bn=f"{p}.bn2", name=f"{p}.conv2")
            if sb != 1 or inplanes != planes * 4:
                idt = g.conv3d(x, planes * 4, (1, 1), (1, sb), (0, 0), f"{p}.downsample.0.weight",
                               bn=f"{p}.downsample.1", relu=False, name=f"{p}.downsample")
            else:
                idt = x
            last = b == nblocks - 1 and out_buf is not None
            x = g.conv3d(a, planes * 4, (1, 1), (1, 1), (0, 0), f"{p}.conv3.weight", bn=f"{p}.bn3", residual=idt,
                         name=f"{p}.out", dst_buf=out_buf if last else None, dst_c_off=0)
            inplanes = planes * 4
        return x

    slow_t = (1, 1, 3, 3)                       # temporal kernel of conv1 in the slow pathway's stages
    fr, sr = f, xs
    for li, nb in enumerate(layers):
        stride = 1 if li == 0 else 2
        fr = stage(fr, fw * 2 ** li, nb, stride, f"fast_res{li + 2}", 3)
        nxt = None
        if li < len(layers) - 1:                # the slow stage's output lands next to the lateral it is concatenated with
            nxt = g.new_buffer(width * 4 * 2 ** li + g.tensors[fr].C * fusion_ratio)
        sr = stage(sr, width * 2 ** li, nb, stride, f"slow_res{li + 2}", slow_t[li], nxt)
        if li == 0:
            g.hooks[1], g.hooks[2] = fr, sr
        if nxt is not None:
            so = g.tensors[sr]
            lt = lateral(fr, nxt, so.C, f"lateral_res{li + 2}")
            assert (g.tensors[lt].T, g.tensors[lt].H) == (so.T, so.H), "pathway shapes disagree"
            sr = g.new_tensor(so.C + g.tensors[lt].C, so.H, so.W, False, f"slow_cat{li + 2}", buf=nxt, c_off=0, T=so.T)
    g.hooks[3], g.hooks[4] = sr, fr
    g.classifier_feats = [sr, fr]
    return g


def tpn_resnet(layers=(3, 4, 6, 3), width=64, in_thw=(32, 224, 224), arch="tpn_resnet50") -> Graph:
    """Backbone of TPN (Yang et al., "Temporal Pyramid Network") up to `layer2`, the module the reference hooks for
    'tpn' models (`image_attacks.py:517-518`).  TPN's backbone is a SlowOnly-style 3-D ResNet: stem 1x7x7 / (1,2,2),
    max-pool 1x3x3 / (1,2,2), and NO temporal convolution in `layer1` / `layer2` (the 3x1x1 inflation starts at
    `layer3`) -- up to the hook it is a per-frame 2-D ResNet, i.e. frame-major image launches.  Keys: torchvision-style
    `conv1 / bn1 / layer{i}.{b}.conv{1,2,3} / bn{1,2,3} / downsample.{0,1}` (parity with gluoncv's module layout
    unpinned, like the other video graphs)."""
    T, H, W = in_thw
    g = Graph(arch, (H, W), video=True)
    x = g.new_tensor(3, H, W, False, "input", T=T)
    g.input = x
    x = g.conv3d(x, width, (1, 7), (1, 2), (0, 3), "conv1.weight", bn="bn1", name="stem")
    x = g.maxpool3d(x, (1, 3), (1, 2), (0, 1), name="maxpool")
    inplanes = width
    for li, nblocks in enumerate(layers[:2]):
        planes = width * (2 ** li)
        for b in range(nblocks):
            stride = 2 if (b == 0 and li > 0) else 1
            p = f"layer{li + 1}.{b}"
            a = g.conv3d(x, planes, (1, 1), (1, 1), (0, 0), f"{p}.conv1.weight", bn=f"{p}.bn1", name=f"{p}.conv1")
            a = g.conv3d(a, planes, (1, 3), (1, stride), (0, 1), f"{p}.conv2.weight", bn=f"{p}.bn2", name=f"{p}.conv2")
            if stride != 1 or inplanes != planes * 4:
                idt = g.conv3d(x, planes * 4, (1, 1), (1, stride), (0, 0), f"{p}.downsample.0.weight",
                               bn=f"{p}.downsample.1", relu=False, name=f"{p}.downsample")
            else:
                idt = x
            x = g.conv3d(a, planes * 4, (1, 1), (1, 1), (0, 0), f"{p}.conv3.weight", bn=f"{p}.bn3", residual=idt,
                         name=f"{p}.out")
            inplanes = planes * 4
        g.hooks[li + 1] = x
    return g


# The reference's configs name `slowfast_8x8_resnet50/101_kinetics400` (`utils.py:11-12`): gluoncv's 8x8 variant samples the slow
# pathway every 8th and the fast pathway every 2nd frame (alpha = 4) and fuses with a 7x1x1 lateral kernel (the 4x16 variant: 16 / 2,
# alpha = 8, kernel 5).  On the 32-frame clips of this path that is 4 slow and 16 fast frames.
SLOWFAST_8X8 = dict(slow_stride=8, fast_stride=2, fusion_kernel=7)


def build_video(model_type: str, in_thw=(32, 224, 224), full: bool = False) -> Graph:
    """`model_type` follows `image_fine_tune_attack.py:53` / `utils.py:9-14`.  `full`: the graph to its last stage (what a
    classifier head needs); the I3D graphs always are, SlowFast then gets res3..res5 and its lateral connections."""
    if full and model_type in ("slowfast_resnet50", "slowfast_resnet101"):
        return slowfast_resnet((3, 4, 23, 3) if "101" in model_type else (3, 4, 6, 3), 64, in_thw, model_type + "_full", **SLOWFAST_8X8)
    # the reference's 'i3d_resnet50' / 'i3d_resnet101' ARE gluoncv's i3d_nl5_resnet50/101_v1 (utils.py:9-10): five non-local blocks
    if model_type in ("i3d_resnet50", "i3d_nl5_resnet50"):
        return i3d_resnet((3, 4, 6, 3), 64, in_thw, "i3d_nl5_resnet50", nonlocal_freq=NL5_FREQ)
    if model_type in ("i3d_resnet101", "i3d_nl5_resnet101"):
        return i3d_resnet((3, 4, 23, 3), 64, in_thw, "i3d_nl5_resnet101", nonlocal_freq=NL5_FREQ)
    if model_type == "i3d_plain_resnet50":          # the inflated ResNet without non-local blocks (not a reference configuration)
        return i3d_resnet((3, 4, 6, 3), 64, in_thw, "i3d_plain_resnet50")
    if model_type == "i3d_plain_resnet101":
        return i3d_resnet((3, 4, 23, 3), 64, in_thw, "i3d_plain_resnet101")
    if model_type == "slowfast_resnet50":
        return slowfast_res2(64, in_thw, "slowfast_resnet50", **SLOWFAST_8X8)
    if model_type == "slowfast_resnet101":          # res2 is identical for the 50- and 101-layer variants
        return slowfast_res2(64, in_thw, "slowfast_resnet101", **SLOWFAST_8X8)
    if model_type == "tpn_resnet50":
        return tpn_resnet((3, 4, 6, 3), 64, in_thw, "tpn_resnet50")
    if model_type == "tpn_resnet101":          # layer1 / layer2 are the same for the 50- and 101-layer backbones
        return tpn_resnet((3, 4, 23, 3), 64, in_thw, "tpn_resnet101")
    raise KeyError(f"video backbone {model_type!r} is not built")


TINY_NL_FREQ = ((0, 0), (1, 1), (1,), (0,))      # tiny I3D: a non-local block behind both blocks of the hooked stage and one in the next


def build_video_tiny(model_type: str, in_thw=(8, 32, 32), full: bool = False) -> Graph:
    if full and "slowfast" in model_type:
        return slowfast_resnet((2, 2, 1, 1), 16, in_thw, "slowfast_tiny_full", slow_stride=4, fast_stride=1, beta_inv=4)
    if "tpn" in model_type:
        return tpn_resnet((2, 2, 1, 1), 8, in_thw, "tpn_tiny")
    if "i3d" in model_type:
        plain = "plain" in model_type
        return i3d_resnet((2, 2, 1, 1), 8, in_thw, "i3d_plain_tiny" if plain else "i3d_tiny", inflate=((1, 1), (1, 0), (1,), (0,)),
                          nonlocal_freq=None if plain else TINY_NL_FREQ)
    return slowfast_res2(16, in_thw, "slowfast_tiny", slow_stride=4, fast_stride=1, beta_inv=4, blocks=2)


def relu_module_names(g: Graph) -> dict:
    """{output tensor of a ReLU convolution: qualified name of the gluoncv `nn.ReLU` module that applies it} for the video
    backbones -- what `base_attacks.SGM` (:511-513) selects its hooks by.  A residual block owns ONE ReLU module, `<block>.relu`,
    applied after each of its three convolutions; the stems' are top-level modules named `*relu` (`relu`; SlowFast: `fast_relu` /
    `slow_relu`); the ReLUs inside SlowFast's lateral `nn.Sequential`s are numbered children (`lateral_p1.2`), no `relu` in their
    names, and are left out."""
    out = {}
    for nd in g.nodes:
        if getattr(nd, "op", "") != "conv" or not nd.relu:
            continue
        parts = nd.weight.split(".")
        if len(parts) == 2 and parts[0].endswith("conv1"):                       # conv1 / fast_conv1 / slow_conv1
            out[nd.dst] = parts[0][:-len("conv1")] + "relu"
        elif len(parts) >= 3 and parts[-1] == "weight" and parts[-2] in ("conv1", "conv2", "conv3"):
            out[nd.dst] = ".".join(parts[:-2] + ["relu"])
    return out


def video_hooks(g: Graph, model_type: str) -> List[int]:
    """Hooked tensors (`image_attacks.py:513-519`).  ILAF's loss is a plain sum over the hooked layers, each paired
    with its own clean feature, so the order is immaterial."""
    if "i3d" in model_type or "tpn" in model_type:          # res_layers['1'] / layer2: the second stage
        return [g.hooks[2]]
    return [g.hooks[1], g.hooks[2]]


# ---------------------------------------------------------------------------
# the ViT surrogates: not graphs of this IR -- a fixed transformer stack, planned by its own library entry (include/i2v_vit.h)
# ---------------------------------------------------------------------------
VIT_NAME = "vit_base_patch16_224"       # the timm name `get_vits()` passes (TPAMI_attack.py:88-98)

#: timm 0.5.0's plain ViT / DeiT family at 224 x 224 (head width 64 throughout): name -> (patch, dim, heads, mlp, blocks, prefix tokens).
#: A ViT and a DeiT of one shape are the same stack with different weights: distinct names, distinct checkpoint files.  The distilled
#: DeiTs carry a second prefix token (`dist_token`) behind `cls_token`.
VIT_MODELS: Dict[str, Tuple[int, int, int, int, int, int]] = {
    "vit_tiny_patch16_224": (16, 192, 3, 768, 12, 1),
    "deit_tiny_patch16_224": (16, 192, 3, 768, 12, 1),
    "vit_small_patch16_224": (16, 384, 6, 1536, 12, 1),
    "deit_small_patch16_224": (16, 384, 6, 1536, 12, 1),
    VIT_NAME: (16, 768, 12, 3072, 12, 1),
    "deit_base_patch16_224": (16, 768, 12, 3072, 12, 1),
    "vit_large_patch16_224": (16, 1024, 16, 4096, 24, 1),
    "vit_small_patch32_224": (32, 384, 6, 1536, 12, 1),
    "vit_base_patch32_224": (32, 768, 12, 3072, 12, 1),
    "vit_large_patch32_224": (32, 1024, 16, 4096, 24, 1),
    "deit_tiny_distilled_patch16_224": (16, 192, 3, 768, 12, 2),
    "deit_small_distilled_patch16_224": (16, 384, 6, 1536, 12, 2),
    "deit_base_distilled_patch16_224": (16, 768, 12, 3072, 12, 2),
}


@dataclass
class VitSpec(TokenSpec):
    """timm `VisionTransformer`: patch embedding (patch x patch convolution, stride patch, bias), `n_prefix`
    prefix tokens prepended (`cls_token`; with 2, `dist_token` of a distilled DeiT behind it), pos_embed added, then `blocks` pre-norm
    blocks x += proj(MHSA(LN1 x)); x += fc2(GELU(fc1(LN2 x))), LayerNorm eps `ln_eps`, exact GELU, scale (dim / heads) ** -0.5.
    `hooks`: depth d (1..4) -> zero-based block d * blocks / 4 - 1 (2, 5, 8, 11 of 12 blocks; 5, 11, 17, 23 of 24), whose OUTPUT (the
    residual stream after it, all tokens, the prefix ones included) is the hooked feature.  A stack whose depth is not a multiple of 4
    (the 6-block test variants) keeps block 3d - 1 for the depths that exist."""
    arch: str
    img: int
    patch: int = 16
    in_chans: int = 3
    dim: int = 768
    heads: int = 12
    mlp: int = 3072
    blocks: int = 12
    ln_eps: float = 1e-6
    hooks: Dict[int, int] = field(default_factory=dict)
    video: bool = False
    n_prefix: int = 1

    def __post_init__(self):
        if self.n_prefix not in (1, 2):
            raise ValueError(f"{self.arch}: {self.n_prefix} prefix tokens (1: cls_token, or 2: cls_token and dist_token)")
        if not self.hooks:
            if self.blocks % 4 == 0:
                self.hooks = self.quarter_hooks()
            else:
                self.hooks = {d: 3 * d - 1 for d in (1, 2, 3, 4) if 3 * d - 1 < self.blocks}

    @property
    def tokens(self) -> int:
        return self.n_prefix + (self.img // self.patch) ** 2

    @property
    def prefix_keys(self) -> List[str]:
        """The state-dict keys of the prefix tokens, in sequence order."""
        return ["cls_token", "dist_token"][:self.n_prefix]

    def block_keys(self, i: int) -> List[str]:
        p = f"blocks.{i}."
        return [p + k for k in ("norm1.weight", "norm1.bias", "attn.qkv.weight", "attn.qkv.bias", "attn.proj.weight", "attn.proj.bias",
                                "norm2.weight", "norm2.bias", "mlp.fc1.weight", "mlp.fc1.bias", "mlp.fc2.weight", "mlp.fc2.bias")]

    def param_shapes(self) -> Dict[str, Tuple[int, ...]]:
        """timm `state_dict` key -> shape for every parameter up to the last block (`norm.*`, `head.*` and a distilled model's
        `head_dist.*` are not used below a hook)."""
        D, H = self.dim, self.mlp
        out = {"patch_embed.proj.weight": (D, self.in_chans, self.patch, self.patch), "patch_embed.proj.bias": (D,)}
        out.update({k: (1, 1, D) for k in self.prefix_keys})
        out["pos_embed"] = (1, self.tokens, D)
        for i in range(self.blocks):
            shapes = [(D,), (D,), (3 * D, D), (3 * D,), (D, D), (D,), (D,), (D,), (H, D), (H,), (D, H), (D,)]
            out.update(zip(self.block_keys(i), shapes))
        return out

    def native_arrays(self, sd, n_blocks: int) -> List["torch.Tensor"]:
        """The arrays `i2v_vit_create_ex` takes for the first `n_blocks` blocks, as float32 host tensors: patch weight, patch bias, the
        prefix tokens as one (n_prefix, dim) array (cls_token, then dist_token), pos_embed, then the blocks as they lie."""
        import torch
        f = lambda k: sd[k].detach().float().cpu()      # noqa: E731
        prefix = torch.cat([f(k).reshape(1, self.dim) for k in self.prefix_keys], 0)
        w = [f(k).contiguous() for k in ("patch_embed.proj.weight", "patch_embed.proj.bias")]
        w += [prefix.contiguous(), f("pos_embed").contiguous()]
        return w + [f(k).contiguous() for i in range(n_blocks) for k in self.block_keys(i)]

    def config_values(self):
        return (self.img, self.patch, self.in_chans, self.dim, self.heads, self.mlp, self.blocks, self.ln_eps)

    @property
    def create_extra(self):
        return (self.n_prefix,)

    def macs_per_frame(self) -> int:
        T, D, H = self.tokens, self.dim, self.mlp
        per_block = T * D * (3 * D + D + 2 * H) + 2 * T * T * D
        return (T - self.n_prefix) * D * self.in_chans * self.patch ** 2 + self.blocks * per_block

    def workspace_bytes(self, hook_blocks: Sequence[int], frames: int) -> int:
        """Device bytes `i2v_vit_create_ex` plans for these hooks and `frames` frames (the formula of csrc/i2v_vit.cpp: weights of the
        blocks run, six saved tensors per block, the shared scratch, one gradient view per hook)."""
        D, H, T, F, nb = self.dim, self.mlp, self.tokens, frames, max(hook_blocks) + 1
        KP, NP, FT = self.in_chans * self.patch ** 2, T - self.n_prefix, frames * T
        probs = F * self.heads * T * ((T + 3) // 4 * 4)
        weights = D * KP + D + self.n_prefix * D + T * D + nb * (4 * D * D + 2 * D * H + 9 * D + H)
        per_block = 5 * FT * D + probs + FT * H + 4 * FT
        shared = 6 * FT * D + FT * H + probs + F * NP * (KP + D)
        return 4 * (weights + nb * per_block + shared + len(hook_blocks) * FT * D)


def vit(in_hw=(224, 224)) -> VitSpec:
    """ViT-B/16 at 224 x 224 only: interpolating pos_embed to another size is not offered."""
    return vit_named(VIT_NAME, in_hw)


def is_vit_name(model_name: str) -> bool:
    """A name of timm's ViT / DeiT vocabulary, served (`VIT_MODELS`) or not: `graphs.build` routes these to `vit_named`, which
    refuses the ones that are not offered with a message that lists the served names."""
    return model_name in VIT_MODELS or model_name.startswith(("vit_", "deit_"))


def vit_named(model_name: str, in_hw=(224, 224)) -> VitSpec:
    """Any row of `VIT_MODELS`, at 224 x 224 only.  Refused, each with the reason: the 384 x 384 checkpoints and every other input
    size (pos_embed interpolation is not offered), the hybrid ResNet-ViT models, the `in21k` heads, and names outside the table."""
    served = "served: " + ", ".join(VIT_MODELS)
    if model_name not in VIT_MODELS:
        if "384" in model_name:
            why = "the 384 x 384 checkpoints are not offered (224 x 224 only: pos_embed is not interpolated)"
        elif "in21k" in model_name:
            why = "the in21k checkpoints (21843-class heads) are not offered"
        elif any(t in model_name for t in ("_r26_", "_r50_", "_r_", "resnet")):
            why = "the hybrid ResNet-ViT models are not offered"
        else:
            why = "not a model of this table"
        raise ValueError(f"ViT surrogate {model_name!r}: {why}; {served}")
    if tuple(in_hw) != (224, 224):
        raise ValueError(f"{model_name} takes 224 x 224 frames only (got {tuple(in_hw)[0]} x {tuple(in_hw)[1]}); "
                         "interpolating its pos_embed to another size is not supported")
    patch, dim, heads, mlp, blocks, n_prefix = VIT_MODELS[model_name]
    return VitSpec(model_name, 224, patch, 3, dim, heads, mlp, blocks, n_prefix=n_prefix)


# The test-size specs below are called "vit_tiny*" for their size.  They are NOT timm's `vit_tiny_patch16_224` (dim 192, 3 heads, 12
# blocks, a row of VIT_MODELS): the arch strings differ ("vit_tiny" against "vit_tiny_patch16_224"), and so do the checkpoint files.
def vit_tiny(in_hw=(64, 64), n_prefix: int = 1, patch: int = 16) -> VitSpec:
    """The same topology at test size: dim 64, 2 heads, 6 blocks (hooks d = 1, 2 -> blocks 2, 5), MLP ratio 4; square frames, a
    multiple of the patch.  `n_prefix = 2`: the distilled twin ("vit_tiny_distilled"); `patch = 32`: the patch-32-style twin
    ("vit_tiny_patch32": a 64 x 64 frame is 4 + 1 tokens)."""
    if in_hw[0] != in_hw[1] or in_hw[0] % patch:
        raise ValueError(f"the tiny ViT takes square frames of a multiple of {patch} pixels (got {tuple(in_hw)})")
    arch = "vit_tiny" + ("_distilled" if n_prefix == 2 else "") + ("_patch32" if patch == 32 else "")
    return VitSpec(arch, int(in_hw[0]), patch, 3, 64, 2, 256, 6, n_prefix=n_prefix)


#: Seeded stand-in for a trained ViT, drawn per key like the CNN initialiser: truncated-normal-like (clamped at 2 std) matrices of std
#: 0.02 as timm initialises them, except qkv at 0.05 so that the attention logits reach O(1) and the softmax is not uniform; LayerNorm
#: gains near 1; small biases.  The residual stream stays O(1) through the 12 blocks (the tests check the hooks).
VIT_SYNTHETIC = clamped_tail(ends("norm1.weight", "norm2.weight"), clamped(0.05))


def _vit_twin(model_name: str, in_hw):
    """One test-size twin per token layout: plain, distilled (2 prefix tokens), patch 32."""
    patch, _, _, _, _, n_prefix = VIT_MODELS[model_name]
    return vit_tiny(in_hw, n_prefix, patch)


VIT_FAMILY = Family("vit", VitSpec, VIT_MODELS, is_vit_name, vit_named, _vit_twin, "timm's plain ViT / DeiT names at 224 x 224", "blocks {}", True,
                VIT_SYNTHETIC)


# ---------------------------------------------------------------------------
# the Swin surrogates: hierarchical, windowed transformers, planned by a library entry of their own (include/i2v_swin.h)
# ---------------------------------------------------------------------------
#: timm 0.5.0's 224 x 224, ImageNet-1k Swin models (patch 4, window 7, MLP ratio 4, head width 32): name -> (C, depths, heads).
SWIN_MODELS: Dict[str, Tuple[int, Tuple[int, ...], Tuple[int, ...]]] = {
    "swin_tiny_patch4_window7_224": (96, (2, 2, 6, 2), (3, 6, 12, 24)),
    "swin_small_patch4_window7_224": (96, (2, 2, 18, 2), (3, 6, 12, 24)),
    "swin_base_patch4_window7_224": (128, (2, 2, 18, 2), (4, 8, 16, 32)),
    "swin_large_patch4_window7_224": (192, (2, 2, 18, 2), (6, 12, 24, 48)),
}


@dataclass
class SwinSpec(StagedSpec):
    """timm `SwinTransformer`: patch embedding (patch x patch convolution, stride patch, bias) and LayerNorm, no
    class token, no position embedding; stage i is `depths[i]` blocks at width dim * 2^i on a grid of (img / patch) / 2^i, with patch
    merging behind every stage but the last.  A block is x += proj(WMSA(LN1 x)); x += fc2(GELU(fc1(LN2 x))) with window attention
    (relative-position bias; odd blocks shifted by window // 2 with the region mask; window = grid and no shift where the grid is not
    larger than the window), LayerNorm eps `ln_eps`, exact GELU, MLP ratio 4.
    `hooks`: depth d (1..stages) -> zero-based stage d - 1, whose last block's OUTPUT, before that stage's patch merging, is the
    hooked feature: grid_i^2 * width_i floats per frame."""
    arch: str
    img: int
    patch: int = 4
    in_chans: int = 3
    dim: int = 96
    window: int = 7
    depths: Tuple[int, ...] = (2, 2, 6, 2)
    heads: Tuple[int, ...] = (3, 6, 12, 24)
    ln_eps: float = 1e-5
    hooks: Dict[int, int] = field(default_factory=dict)
    video: bool = False

    def __post_init__(self):
        self.depths, self.heads = tuple(self.depths), tuple(self.heads)
        if len(self.depths) != len(self.heads) or not 1 <= len(self.depths) <= 4:
            raise ValueError(f"{self.arch}: depths {self.depths} and heads {self.heads} must name the same 1..4 stages")
        for i in range(self.stages):
            if self.grid(i) * self.patch << i != self.img or self.grid(i) % self.window:
                raise ValueError(f"{self.arch}: a {self.img} x {self.img} frame does not give stage {i} a grid of whole "
                                 f"{self.window} x {self.window} windows")
            if self.width(i) % self.heads[i]:
                raise ValueError(f"{self.arch}: width {self.width(i)} of stage {i} is not a multiple of its {self.heads[i]} heads")
        if not self.hooks:
            self.hooks = {d: d - 1 for d in range(1, self.stages + 1)}

    @property
    def stages(self) -> int:
        return len(self.depths)

    def grid(self, i: int) -> int:
        return (self.img // self.patch) >> i

    def width(self, i: int) -> int:
        return self.dim << i

    def tokens(self, i: int) -> int:
        return self.grid(i) ** 2

    def hook_dim(self, i: int) -> int:
        """Floats per frame of the feature hooked at stage i."""
        return self.tokens(i) * self.width(i)

    def shift(self, i: int, j: int) -> int:
        """Cyclic shift of block j of stage i."""
        return self.window // 2 if j % 2 == 1 and self.grid(i) > self.window else 0

    @property
    def n_index(self) -> int:
        return (2 * self.window - 1) ** 2

    def block_keys(self, i: int, j: int) -> List[str]:
        p = f"layers.{i}.blocks.{j}."
        return [p + k for k in ("norm1.weight", "norm1.bias", "attn.qkv.weight", "attn.qkv.bias", "attn.relative_position_bias_table",
                                "attn.proj.weight", "attn.proj.bias", "norm2.weight", "norm2.bias", "mlp.fc1.weight", "mlp.fc1.bias",
                                "mlp.fc2.weight", "mlp.fc2.bias")]

    def merge_keys(self, i: int) -> List[str]:
        p = f"layers.{i}.downsample."
        return [p + "norm.weight", p + "norm.bias", p + "reduction.weight"]

    def embed_keys(self) -> List[str]:
        return ["patch_embed.proj.weight", "patch_embed.proj.bias", "patch_embed.norm.weight", "patch_embed.norm.bias"]

    def native_keys(self, n_stages: int) -> List[str]:
        """The keys in the order `i2v_swin_create` takes the arrays, for the first `n_stages` stages."""
        out = self.embed_keys()
        for i in range(n_stages):
            for j in range(self.depths[i]):
                out += self.block_keys(i, j)
            if i + 1 < n_stages:
                out += self.merge_keys(i)
        return out

    def native_arrays(self, sd, n_stages: int) -> List["torch.Tensor"]:
        """The arrays `i2v_swin_create` takes for the first `n_stages` stages, as they lie, as float32 host tensors (include/i2v_swin.h:
        the embedding, then per stage its blocks and the merging behind it)."""
        return [sd[k].detach().float().cpu().contiguous() for k in self.native_keys(n_stages)]

    def config_values(self):
        return (self.img, self.patch, self.in_chans, self.dim, self.window, self.stages, self.depths, self.heads, self.ln_eps)

    def param_shapes(self) -> Dict[str, Tuple[int, ...]]:
        """timm `state_dict` key -> shape for every parameter up to the last block (the merging behind the last stage does not exist;
        `norm.*` and `head.*` are not used below a hook; the `relative_position_index` / `attn_mask` buffers are computed)."""
        C = self.dim
        out = dict(zip(self.embed_keys(), [(C, self.in_chans, self.patch, self.patch), (C,), (C,), (C,)]))
        for i in range(self.stages):
            D, H = self.width(i), self.heads[i]
            for j in range(self.depths[i]):
                shapes = [(D,), (D,), (3 * D, D), (3 * D,), (self.n_index, H), (D, D), (D,), (D,), (D,), (4 * D, D), (4 * D,), (D, 4 * D), (D,)]
                out.update(zip(self.block_keys(i, j), shapes))
            if i + 1 < self.stages:
                out.update(zip(self.merge_keys(i), [(4 * D,), (4 * D,), (2 * D, 4 * D)]))
        return out

    def relative_position_index(self) -> "torch.Tensor":
        """(window^2, window^2) int64: idx[i, j] = (r_i - r_j + window - 1)(2 window - 1) + c_i - c_j + window - 1."""
        import torch
        w = self.window
        r, c = torch.arange(w * w) // w, torch.arange(w * w) % w
        return (r[:, None] - r[None, :] + w - 1) * (2 * w - 1) + (c[:, None] - c[None, :] + w - 1)

    def attn_mask(self, i: int) -> "torch.Tensor":
        """(windows, window^2, window^2) float32 mask of the shifted blocks of stage i, by the closed formula: 0 where the two tokens
        lie in the same region of the rolled grid, -100 elsewhere."""
        import torch
        g, w, sh = self.grid(i), self.window, self.window // 2
        y = torch.arange(g)
        reg1 = (y >= g - w).long() + (y >= g - sh).long()
        reg = (reg1[:, None] * 3 + reg1[None, :]).reshape(g // w, w, g // w, w).permute(0, 2, 1, 3).reshape(-1, w * w)
        return torch.where(reg[:, :, None] == reg[:, None, :], 0.0, -100.0).float()

    def macs_per_frame(self) -> int:
        total = self.tokens(0) * self.dim * self.in_chans * self.patch ** 2
        for i in range(self.stages):
            T, D = self.tokens(i), self.width(i)
            total += self.depths[i] * (T * D * 12 * D + 2 * T * min(self.window, self.grid(i)) ** 2 * D)
            if i + 1 < self.stages:
                total += (T // 4) * 8 * D * D
        return total

    def workspace_bytes(self, hook_stages: Sequence[int], frames: int) -> int:
        """Device bytes `i2v_swin_create` plans for these hooked stages and `frames` frames (the formula of csrc/i2v_swin.cpp: weights of
        the stages run; patches, embedding and its LayerNorm statistics; per block the input stream, qkv, the mid stream, the fc1
        pre-activation and four statistics per token; per stage its output stream; per merging the gathered rows and their statistics;
        the shared scratch; one gradient view per hook)."""
        F, ns = frames, max(hook_stages) + 1
        KP, T0, D0 = self.in_chans * self.patch ** 2, self.tokens(0), self.dim
        weights = D0 * KP + 3 * D0
        acts = F * T0 * (KP + D0 + 2)
        for i in range(ns):
            D, FT = self.width(i), F * self.tokens(i)
            weights += self.depths[i] * (12 * D * D + 13 * D + self.n_index * self.heads[i])
            acts += self.depths[i] * (9 * FT * D + 4 * FT) + FT * D
            if i + 1 < ns:
                weights += 8 * D + 8 * D * D
                acts += FT * D + 2 * (FT // 4)
        acts += 9 * F * T0 * D0
        acts += sum(F * self.hook_dim(s) for s in hook_stages)
        return 4 * (weights + acts)


def is_swin_name(model_name: str) -> bool:
    """A name of timm's Swin vocabulary, served (`SWIN_MODELS`) or not: `graphs.build` routes these to `swin_named`, which refuses the
    ones that are not offered with a message that lists the served names."""
    return model_name in SWIN_MODELS or model_name.startswith("swin_")


def swin_named(model_name: str, in_hw=(224, 224)) -> SwinSpec:
    """Any row of `SWIN_MODELS`, at 224 x 224 only.  Refused, each with the reason: the window-12 384 x 384 models and every other input
    size, the `in22k` checkpoints, and names outside the table."""
    served = "served: " + ", ".join(SWIN_MODELS)
    if model_name not in SWIN_MODELS:
        if "384" in model_name or "window12" in model_name:
            why = "the window-12 384 x 384 models are not offered (224 x 224 with window 7 only)"
        elif "in22k" in model_name:
            why = "the in22k checkpoints (21841-class heads) are not offered"
        else:
            why = "not a model of this table"
        raise ValueError(f"Swin surrogate {model_name!r}: {why}; {served}")
    if tuple(in_hw) != (224, 224):
        raise ValueError(f"{model_name} takes 224 x 224 frames only (got {tuple(in_hw)[0]} x {tuple(in_hw)[1]}): its window-7 stages need "
                         "the 56 / 28 / 14 / 7 grids")
    dim, depths, heads = SWIN_MODELS[model_name]
    return SwinSpec(model_name, 224, 4, 3, dim, 7, depths, heads)


def swin_tiny(in_hw=(64, 64)) -> SwinSpec:
    """The same topology at test size ("swin_test": not timm's `swin_tiny_patch4_window7_224`): patch 4, window 4, C = 16, depths (2, 2),
    heads (1, 2), head width 16.  A 64 x 64 frame is a 16 x 16 grid of 16 windows, then 8 x 8 with 4: both blocks of both stages are real,
    the shifted one included, and there is one patch merging.  Square frames of a multiple of 32 pixels."""
    if in_hw[0] != in_hw[1] or in_hw[0] % 32:
        raise ValueError(f"the test-size Swin takes square frames of a multiple of 32 pixels (got {tuple(in_hw)})")
    return SwinSpec("swin_test", int(in_hw[0]), 4, 3, 16, 4, (2, 2), (1, 2))


def check_swin_buffers(spec: SwinSpec, sd, where: str) -> None:
    """timm's Swin checkpoints carry the buffers `relative_position_index` and `attn_mask`; they are computed from the geometry here
    and never loaded, so one that differs describes another model: refused by key name."""
    import torch
    idx = spec.relative_position_index()
    for i in range(spec.stages):
        for j in range(spec.depths[i]):
            p = f"layers.{i}.blocks.{j}."
            k = p + "attn.relative_position_index"
            if k in sd and not (tuple(sd[k].shape) == tuple(idx.shape) and torch.equal(sd[k].long(), idx)):
                raise ValueError(f"{where}: buffer {k} differs from the index computed for window {spec.window}")
            k = p + "attn_mask"
            if k in sd and sd[k] is not None:
                if spec.shift(i, j) == 0:
                    raise ValueError(f"{where}: buffer {k} is a mask, but block {j} of stage {i} is not shifted")
                want = spec.attn_mask(i)
                if not (tuple(sd[k].shape) == tuple(want.shape) and torch.equal(sd[k].float(), want)):
                    raise ValueError(f"{where}: buffer {k} differs from the mask computed for a {spec.grid(i)} x {spec.grid(i)} grid, "
                                     f"window {spec.window}, shift {spec.shift(i, j)}")


#: Seeded stand-in for a trained Swin, drawn per key: matrices of std 0.02 clamped at 2 std as timm initialises them, except qkv at
#: width^-0.5, which puts the attention logits at O(1) at every stage's width (96 .. 1536), and the relative-position bias table at
#: std 0.5, so that the bias visibly shapes the softmax; LayerNorm gains near 1; small biases.  Each block then adds a few tenths to a
#: unit-variance stream, which stays O(1) through swin_small's 24 blocks (the tests check the hooks' spread).
SWIN_SYNTHETIC = [(ends("relative_position_bias_table"), clamped(0.5)),
                  *clamped_tail(ends("norm1.weight", "norm2.weight", "norm.weight"), lambda shp, g: clamped(shp[1] ** -0.5)(shp, g))]

SWIN_FAMILY = Family("swin", SwinSpec, SWIN_MODELS, is_swin_name, swin_named, lambda name, in_hw: swin_tiny(in_hw),
                "timm's Swin names at 224 x 224", "the last block of stages {}", True, SWIN_SYNTHETIC, check_swin_buffers)


# ---------------------------------------------------------------------------
# the ConvNeXt surrogates: convolutional, but planned on the transformer stack (include/i2v_convnext.h)
# ---------------------------------------------------------------------------
#: timm's 224 x 224, ImageNet-1k ConvNeXt models (stem 4 x 4 / 4, 7 x 7 depthwise blocks, MLP ratio 4): name -> (C, depths).
CONVNEXT_MODELS: Dict[str, Tuple[int, Tuple[int, ...]]] = {
    "convnext_tiny": (96, (3, 3, 9, 3)),
    "convnext_small": (96, (3, 3, 27, 3)),
    "convnext_base": (128, (3, 3, 27, 3)),
    "convnext_large": (192, (3, 3, 27, 3)),
}


@dataclass
class ConvNextSpec(StagedSpec):
    """timm `ConvNeXt`: the stem is a patch x patch convolution with stride patch and bias, then a LayerNorm over
    channels; stage i is `depths[i]` blocks at width dim * 2^i on a plane of (img / patch) / 2^i squared, with a downsample (LayerNorm
    over channels, then a 2 x 2 / 2 convolution with bias) in front of every stage but the first.  A block is
    x + gamma * fc2(GELU(fc1(LN(dwconv7x7(x))))) with LN, fc1, GELU and fc2 per position over channels, LayerNorm eps `ln_eps`, exact
    GELU, MLP ratio 4.  `hooks`: depth d (1..stages) -> zero-based stage d - 1, whose last block's OUTPUT, before the next stage's
    downsample, is the hooked feature: plane_i^2 * width_i floats per frame, handed over token-major (row, column, channel)."""
    arch: str
    img: int
    patch: int = 4
    in_chans: int = 3
    dim: int = 96
    depths: Tuple[int, ...] = (3, 3, 9, 3)
    ln_eps: float = 1e-6
    hooks: Dict[int, int] = field(default_factory=dict)
    video: bool = False

    def __post_init__(self):
        self.depths = tuple(self.depths)
        if not 1 <= len(self.depths) <= 4 or min(self.depths) < 1:
            raise ValueError(f"{self.arch}: depths {self.depths} must name 1..4 stages of at least one block")
        if self.dim % 4 or self.patch % 4:
            raise ValueError(f"{self.arch}: width {self.dim} and stem patch {self.patch} must be multiples of 4")
        if self.img % (self.patch << (self.stages - 1)):
            raise ValueError(f"{self.arch}: a {self.img} x {self.img} frame does not halve {self.stages - 1} times behind a "
                             f"{self.patch} x {self.patch} stem")
        if not self.hooks:
            self.hooks = {d: d - 1 for d in range(1, self.stages + 1)}

    @property
    def stages(self) -> int:
        return len(self.depths)

    def grid(self, i: int) -> int:
        return (self.img // self.patch) >> i

    def width(self, i: int) -> int:
        return self.dim << i

    def tokens(self, i: int) -> int:
        return self.grid(i) ** 2

    def hook_dim(self, i: int) -> int:
        """Floats per frame of the feature hooked at stage i."""
        return self.tokens(i) * self.width(i)

    def stem_keys(self) -> List[str]:
        return ["stem.0.weight", "stem.0.bias", "stem.1.weight", "stem.1.bias"]

    def downsample_keys(self, i: int) -> List[str]:
        p = f"stages.{i}.downsample."
        return [p + "0.weight", p + "0.bias", p + "1.weight", p + "1.bias"]

    def block_keys(self, i: int, j: int) -> List[str]:
        p = f"stages.{i}.blocks.{j}."
        return [p + k for k in ("conv_dw.weight", "conv_dw.bias", "norm.weight", "norm.bias", "mlp.fc1.weight", "mlp.fc1.bias",
                                "mlp.fc2.weight", "mlp.fc2.bias", "gamma")]

    def param_shapes(self) -> Dict[str, Tuple[int, ...]]:
        """timm `state_dict` key -> shape for every parameter up to the last block (`norm_pre.*`, `head.*` are not used below a hook)."""
        C = self.dim
        out = dict(zip(self.stem_keys(), [(C, self.in_chans, self.patch, self.patch), (C,), (C,), (C,)]))
        for i in range(self.stages):
            D = self.width(i)
            if i > 0:
                out.update(zip(self.downsample_keys(i), [(D // 2,), (D // 2,), (D, D // 2, 2, 2), (D,)]))
            for j in range(self.depths[i]):
                out.update(zip(self.block_keys(i, j), [(D, 1, 7, 7), (D,), (D,), (D,), (4 * D, D), (4 * D,), (D, 4 * D), (D,), (D,)]))
        return out

    @staticmethod
    def downsample_linear(w: "torch.Tensor") -> "torch.Tensor":
        """The (2C, C, 2, 2) weight of a downsample's 2 x 2 / 2 convolution as the Linear (2C, 4C) behind the 2 x 2 gather of the
        transformer stack, whose quarter q of a gathered row is the position at (row, column) offset (q & 1, q >> 1) of its cell:
        L[o][q * C + c] = w[o][c][q & 1][q >> 1], i.e. the axes (o, c, dy, dx) reordered to (o, dx, dy, c)."""
        return w.permute(0, 3, 2, 1).reshape(w.shape[0], -1).contiguous()

    def native_arrays(self, sd, n_stages: int) -> List["torch.Tensor"]:
        """The arrays `i2v_convnext_create` takes for the first `n_stages` stages, from a timm-layout state dict, as float32 host
        tensors: the depthwise filters transposed to (49, C), the downsample convolutions as Linears (`downsample_linear`), and `gamma`
        folded into fc2 -- fc2.weight[o, :] * gamma[o], fc2.bias[o] * gamma[o] --, so that the layer scale costs nothing at run time."""
        f = lambda k: sd[k].detach().float().cpu()      # noqa: E731
        out = [f(k).contiguous() for k in self.stem_keys()]
        for i in range(n_stages):
            if i > 0:
                k = self.downsample_keys(i)
                out += [f(k[0]).contiguous(), f(k[1]).contiguous(), self.downsample_linear(f(k[2])), f(k[3]).contiguous()]
            for j in range(self.depths[i]):
                k = self.block_keys(i, j)
                D, gamma = self.width(i), f(k[8])
                out += [f(k[0]).reshape(D, 49).t().contiguous()] + [f(x).contiguous() for x in k[1:6]]
                out += [(f(k[6]) * gamma[:, None]).contiguous(), (f(k[7]) * gamma).contiguous()]
        return out

    def config_values(self):
        return (self.img, self.patch, self.in_chans, self.dim, self.stages, self.depths, self.ln_eps)

    def macs_per_frame(self) -> int:
        total = self.tokens(0) * self.dim * self.in_chans * self.patch ** 2
        for i in range(self.stages):
            T, D = self.tokens(i), self.width(i)
            total += self.depths[i] * (T * D * 49 + T * D * 8 * D)
            if i > 0:
                total += T * D * 2 * D
        return total

    def workspace_bytes(self, hook_stages: Sequence[int], frames: int) -> int:
        """Device bytes `i2v_convnext_create` plans for these hooked stages and `frames` frames (the formula of csrc/i2v_convnext.cpp:
        weights of the stages run, each block's filter twice (the mirrored copy); patches, stem output and its LayerNorm statistics;
        per stage one stream; per block the depthwise output, the fc1 pre-activation and two statistics per position; per downsample
        two statistics per position of the stage before; the shared scratch; one gradient view per hook)."""
        F, ns = frames, max(hook_stages) + 1
        KP, T0, D0 = self.in_chans * self.patch ** 2, self.tokens(0), self.dim
        weights = D0 * KP + 3 * D0
        acts = F * T0 * (KP + D0 + 2)
        for i in range(ns):
            D, FT = self.width(i), F * self.tokens(i)
            if i > 0:
                weights += 2 * D + 2 * D * D
                acts += 8 * FT
            weights += self.depths[i] * (8 * D * D + 49 * D + 8 * D)
            acts += self.depths[i] * (49 * D + 5 * FT * D + 2 * FT) + FT * D
        acts += 7 * F * T0 * D0
        acts += sum(F * self.hook_dim(s) for s in hook_stages)
        return 4 * (weights + acts)


def is_convnext_name(model_name: str) -> bool:
    """A name of timm's ConvNeXt vocabulary, served (`CONVNEXT_MODELS`) or not: `graphs.build` routes these to `convnext_named`, which
    refuses the ones that are not offered with a message that lists the served names."""
    return model_name in CONVNEXT_MODELS or model_name.startswith("convnext")


def convnext_named(model_name: str, in_hw=(224, 224)) -> ConvNextSpec:
    """Any row of `CONVNEXT_MODELS`, at 224 x 224 only.  Refused, each with the reason where there is one: ConvNeXt-V2 (its blocks carry
    a global response normalisation), the 384 x 384 fine-tunes, the in22k / in22ft1k checkpoints, and names outside the table (xlarge,
    nano, atto, ...)."""
    served = "served: " + ", ".join(CONVNEXT_MODELS)
    if model_name not in CONVNEXT_MODELS:
        if model_name.startswith("convnextv2"):
            why = "ConvNeXt-V2 blocks carry a global response normalisation (GRN) that is not built"
        elif "384" in model_name:
            why = "the 384 x 384 fine-tunes are not offered (224 x 224 only)"
        elif "in22ft1k" in model_name:
            why = "the in22ft1k checkpoints are not offered (the ImageNet-1k models only)"
        elif "in22k" in model_name:
            why = "the in22k checkpoints (21841-class heads) are not offered"
        else:
            why = "not a model of this table"
        raise ValueError(f"ConvNeXt surrogate {model_name!r}: {why}; {served}")
    if tuple(in_hw) != (224, 224):
        raise ValueError(f"{model_name} takes 224 x 224 frames only (got {tuple(in_hw)[0]} x {tuple(in_hw)[1]})")
    dim, depths = CONVNEXT_MODELS[model_name]
    return ConvNextSpec(model_name, 224, 4, 3, dim, depths)


def convnext_tiny_twin(in_hw=(64, 64)) -> ConvNextSpec:
    """The same topology at test size ("convnext_test": not timm's `convnext_tiny`): widths 8 / 16 / 32 / 64, depths (2, 1, 2, 1).  A
    64 x 64 frame gives planes of 16, 8, 4 and 2 squared: the 7 x 7 filter is larger than the last two.  Square frames of a multiple of
    32 pixels."""
    if in_hw[0] != in_hw[1] or in_hw[0] % 32:
        raise ValueError(f"the test-size ConvNeXt takes square frames of a multiple of 32 pixels (got {tuple(in_hw)})")
    return ConvNextSpec("convnext_test", int(in_hw[0]), 4, 3, 8, (2, 1, 2, 1))


#: Seeded stand-in for a trained ConvNeXt, drawn per key: the stem and downsample convolutions at fan_in^-0.5 (a unit-variance stream
#: stays one), depthwise filters at 1 / 7 (49 taps of unit inputs give unit outputs), fc1 at fan_in^-0.5 and fc2 at 0.5 fan_in^-0.5,
#: LayerNorm gains near 1, small biases, and `gamma` spread over 0.1 .. 0.5 with random signs -- far from the ones a forgotten fold
#: would use.  Each block then adds a few tenths to its stream, which stays O(1) through 36 blocks.
CONVNEXT_SYNTHETIC = [(ends("gamma"), signed_uniform(0.1, 0.4)), (ends("conv_dw.weight"), normal_over(7.0)),
                      *fan_in_tail(ends("norm.weight", "stem.1.weight", "downsample.0.weight"), half=ends("fc2.weight"))]

CONVNEXT_FAMILY = Family("convnext", ConvNextSpec, CONVNEXT_MODELS, is_convnext_name, convnext_named, lambda name, in_hw: convnext_tiny_twin(in_hw),
                "timm's ConvNeXts at 224 x 224", "the last block of stages {}", True, CONVNEXT_SYNTHETIC)


# ---------------------------------------------------------------------------
# the all-MLP surrogates: MLP-Mixer and ResMLP, planned on the transformer stack (include/i2v_mixer.h)
# ---------------------------------------------------------------------------
#: timm 0.5.0's `MlpMixer` models at 224 x 224 with ImageNet-1k heads: name -> (kind, patch, dim, blocks).  The distilled ResMLPs are
#: the same graph as the plain ones: distinct names, distinct checkpoint files.
MIXER_MODELS: Dict[str, Tuple[str, int, int, int]] = {
    "mixer_s32_224": ("mixer", 32, 512, 8),
    "mixer_s16_224": ("mixer", 16, 512, 8),
    "mixer_b32_224": ("mixer", 32, 768, 12),
    "mixer_b16_224": ("mixer", 16, 768, 12),
    "mixer_l32_224": ("mixer", 32, 1024, 24),
    "mixer_l16_224": ("mixer", 16, 1024, 24),
    "resmlp_12_224": ("resmlp", 16, 384, 12),
    "resmlp_24_224": ("resmlp", 16, 384, 24),
    "resmlp_36_224": ("resmlp", 16, 384, 36),
    "resmlp_12_distilled_224": ("resmlp", 16, 384, 12),
    "resmlp_24_distilled_224": ("resmlp", 16, 384, 24),
    "resmlp_36_distilled_224": ("resmlp", 16, 384, 36),
}


@dataclass
class MixerSpec(TokenSpec):
    """timm 0.5.0 `MlpMixer`: the stem is a patch x patch convolution with stride patch and bias -- no norm, no
    prefix token, no pos_embed --, giving `tokens` = (img / patch)^2 tokens of `dim` channels; then `blocks` blocks.
      kind "mixer"  (`MixerBlock`)  x += mlp_tokens(LN1(x)^T)^T, fc1 (tokens_hidden, tokens), GELU, fc2 (tokens, tokens_hidden), down the
                                    token axis per channel; x += mlp_channels(LN2(x)), fc1 (mlp, dim), GELU, fc2; LayerNorm eps `ln_eps`
      kind "resmlp" (`ResBlock`)    x += ls1 * linear_tokens((alpha1 * x + beta1)^T)^T; x += ls2 * mlp_channels(alpha2 * x + beta2);
                                    `Affine` norms, tokens_hidden = 0
    Exact GELU.  `hooks`: depth d (1..4) -> zero-based block d * blocks / 4 - 1, whose OUTPUT (the residual stream after it, all tokens)
    is the hooked feature: tokens * dim floats per frame, token-major."""
    arch: str
    img: int
    patch: int = 16
    in_chans: int = 3
    dim: int = 768
    blocks: int = 12
    kind: str = "mixer"
    ln_eps: float = 1e-6
    hooks: Dict[int, int] = field(default_factory=dict)
    video: bool = False

    def __post_init__(self):
        if self.kind not in ("mixer", "resmlp"):
            raise ValueError(f"{self.arch}: kind {self.kind!r} (mixer or resmlp)")
        if self.img % self.patch or self.patch % 4 or self.dim % 4:
            raise ValueError(f"{self.arch}: a {self.img} x {self.img} frame, patch {self.patch}, width {self.dim}: the patch must divide "
                             "the frame, and patch and width must be multiples of 4")
        if self.blocks % 4:
            raise ValueError(f"{self.arch}: {self.blocks} blocks: depths 1..4 hook blocks d * blocks / 4 - 1")
        if not self.hooks:
            self.hooks = self.quarter_hooks()

    @property
    def tokens(self) -> int:
        return (self.img // self.patch) ** 2

    @property
    def tokens_hidden(self) -> int:
        """Width of the token MLP's hidden layer (timm's mlp_ratio[0] = 0.5 of dim); 0 for ResMLP, whose token mixing is one Linear."""
        return self.dim // 2 if self.kind == "mixer" else 0

    @property
    def mlp(self) -> int:
        return 4 * self.dim

    def hook_dim(self, i: int = 0) -> int:
        """Floats per frame of the feature hooked at block i (the same for every block)."""
        return self.tokens * self.dim

    def block_keys(self, i: int) -> List[str]:
        p = f"blocks.{i}."
        if self.kind == "mixer":
            names = ("norm1.weight", "norm1.bias", "mlp_tokens.fc1.weight", "mlp_tokens.fc1.bias", "mlp_tokens.fc2.weight",
                     "mlp_tokens.fc2.bias", "norm2.weight", "norm2.bias", "mlp_channels.fc1.weight", "mlp_channels.fc1.bias",
                     "mlp_channels.fc2.weight", "mlp_channels.fc2.bias")
        else:
            names = ("ls1", "ls2", "norm1.alpha", "norm1.beta", "linear_tokens.weight", "linear_tokens.bias", "norm2.alpha", "norm2.beta",
                     "mlp_channels.fc1.weight", "mlp_channels.fc1.bias", "mlp_channels.fc2.weight", "mlp_channels.fc2.bias")
        return [p + k for k in names]

    def param_shapes(self) -> Dict[str, Tuple[int, ...]]:
        """timm `state_dict` key -> shape for every parameter up to the last block, in timm's order (`norm.*` and `head.*` lie behind
        every hook and are not used)."""
        D, S, Sh, H = self.dim, self.tokens, self.tokens_hidden, self.mlp
        out = {"stem.proj.weight": (D, self.in_chans, self.patch, self.patch), "stem.proj.bias": (D,)}
        if self.kind == "mixer":
            shapes = [(D,), (D,), (Sh, S), (Sh,), (S, Sh), (S,), (D,), (D,), (H, D), (H,), (D, H), (D,)]
        else:
            shapes = [(D,), (D,), (1, 1, D), (1, 1, D), (S, S), (S,), (1, 1, D), (1, 1, D), (H, D), (H,), (D, H), (D,)]
        for i in range(self.blocks):
            out.update(zip(self.block_keys(i), shapes))
        return out

    def native_arrays(self, sd, n_blocks: int) -> List["torch.Tensor"]:
        """The arrays `i2v_mixer_create` takes for the first `n_blocks` blocks, from a timm-layout state dict, as float32 host tensors.
        MLP-Mixer: the stem and each block's twelve arrays as they lie.  ResMLP, nine per block: alpha1, beta1 and ls1 as (dim) arrays
        for the token launch, linear_tokens as it lies, then mlp_channels.fc1 with `norm2` folded in (column c times alpha2[c]; bias
        plus weight . beta2) and mlp_channels.fc2 with `ls2` folded in (row o and bias element o times ls2[o]): the affine and the layer
        scale of the channel half cost nothing at run time.  The folds are made in float64."""
        f = lambda k: sd[k].detach().float().cpu()      # noqa: E731
        out = [f("stem.proj.weight").contiguous(), f("stem.proj.bias").contiguous()]
        for i in range(n_blocks):
            k = self.block_keys(i)
            if self.kind == "mixer":
                out += [f(x).contiguous() for x in k]
                continue
            ls1, ls2, a1, b1, a2, b2 = (f(x).reshape(-1) for x in (k[0], k[1], k[2], k[3], k[6], k[7]))
            w1, c1, w2, c2 = (f(x).double() for x in k[8:12])
            out += [a1.contiguous(), b1.contiguous(), ls1.contiguous(), f(k[4]).contiguous(), f(k[5]).contiguous()]
            out += [(w1 * a2.double()[None, :]).float().contiguous(), (c1 + w1 @ b2.double()).float().contiguous()]
            out += [(w2 * ls2.double()[:, None]).float().contiguous(), (c2 * ls2.double()).float().contiguous()]
        return out

    def config_values(self):
        return (self.img, self.patch, self.in_chans, self.dim, self.blocks, self.tokens_hidden, self.mlp, 1 if self.kind == "resmlp" else 0, self.ln_eps)

    def macs_per_frame(self) -> int:
        S, D, Sh, H = self.tokens, self.dim, self.tokens_hidden, self.mlp
        token = 2 * S * Sh * D if Sh else S * S * D
        return S * D * self.in_chans * self.patch ** 2 + self.blocks * (token + 2 * S * D * H)

    def workspace_bytes(self, hook_blocks: Sequence[int], frames: int) -> int:
        """Device bytes `i2v_mixer_create` plans for these hooked blocks and `frames` frames (the formula of csrc/i2v_mixer.cpp).
        MLP-Mixer: the weights of the blocks run, each block's two token weights once more (the transposed copies); patches; per block
        its mid stream, its output, the fc1 pre-activation and four statistics per token; the first block's input; the shared scratch
        (two streams, one more for the running gradient, one MLP-wide); one gradient view per hook.  ResMLP: the folded weights, the
        token weight twice; patches; one stream; per block the fc1 pre-activation; scratch (one MLP-wide, the running gradient); per
        hook a copy of the stream and a gradient view."""
        D, S, Sh, H, nb = self.dim, self.tokens, self.tokens_hidden, self.mlp, max(hook_blocks) + 1
        KP, FT, nh = self.in_chans * self.patch ** 2, frames * self.tokens, len(hook_blocks)
        weights = D * KP + D
        if self.kind == "mixer":
            weights += nb * (4 * D + 2 * Sh * S + Sh + S + 2 * D * H + H + D + 2 * S * Sh)
            acts = FT * KP + nb * (2 * FT * D + FT * H + 4 * FT) + FT * D + (3 * FT * D + FT * H)
        else:
            weights += nb * (3 * D + S * S + S + 2 * D * H + H + D + S * S)
            acts = FT * KP + nb * FT * H + FT * D + (FT * H + FT * D) + nh * FT * D
        return 4 * (weights + acts + nh * FT * D)


def is_mixer_name(model_name: str) -> bool:
    """A name of timm's all-MLP vocabulary (`mlp_mixer.py`), served (`MIXER_MODELS`) or not: `graphs.build` routes these to
    `mixer_named`, which refuses the ones that are not offered with a message that lists the served names."""
    return model_name in MIXER_MODELS or model_name.startswith(("mixer_", "resmlp_", "gmixer_", "gmlp_"))


def mixer_named(model_name: str, in_hw=(224, 224)) -> MixerSpec:
    """Any row of `MIXER_MODELS`, at 224 x 224 only.  Refused, each with the reason: the in21k / in22ft1k / miil / dino checkpoints,
    `resmlp_big_24_*` (patch 8), the gated models (`gmixer_*`, `gmlp_*`), and names outside the table."""
    served = "served: " + ", ".join(MIXER_MODELS)
    if model_name not in MIXER_MODELS:
        if any(t in model_name for t in ("_in21k", "_in22ft1k", "_miil", "_dino")):
            why = ("the in21k / in22ft1k / miil / dino checkpoints carry other label sets or expect other pre-processing and are not "
                   "offered (the ImageNet-1k models only)")
        elif model_name.startswith("resmlp_big_24_"):
            why = "resmlp_big_24 cuts 8 x 8 patches (784 tokens): the token tile is not planned for it"
        elif model_name.startswith(("gmixer_", "gmlp_")):
            why = "the gated models (gMixer's SiLU-gated units, gMLP's spatial gating unit) are not built"
        else:
            why = "not a model of this table"
        raise ValueError(f"MLP-Mixer / ResMLP surrogate {model_name!r}: {why}; {served}")
    if tuple(in_hw) != (224, 224):
        raise ValueError(f"{model_name} takes 224 x 224 frames only (got {tuple(in_hw)[0]} x {tuple(in_hw)[1]}): its token-mixing weights "
                         "fix the number of tokens")
    kind, patch, dim, blocks = MIXER_MODELS[model_name]
    return MixerSpec(model_name, 224, patch, 3, dim, blocks, kind)


def mixer_tiny_twin(kind: str = "mixer", patch: int = 16, in_hw=(64, 64)) -> MixerSpec:
    """The same topology at test size: dim 32, 8 blocks, so depths 1..4 hook blocks 1, 3, 5, 7; square frames of a multiple of 32 pixels,
    whose size fixes the token count and with it the token weights.  At 64 x 64 -- "mixer_test": patch 16, 16 tokens, token hidden
    width 16; "mixer_test_patch32": 4 tokens; "resmlp_test": the ResMLP twin, patch 32, 4 tokens.  None of them is a row of
    `MIXER_MODELS`."""
    if in_hw[0] != in_hw[1] or in_hw[0] % 32:
        raise ValueError(f"the test-size MLP-Mixer / ResMLP take square frames of a multiple of 32 pixels (got {tuple(in_hw)})")
    arch = "resmlp_test" if kind == "resmlp" else "mixer_test" + ("_patch32" if patch == 32 else "")
    return MixerSpec(arch, int(in_hw[0]), patch, 3, 32, 8, kind)


#: Seeded stand-in for a trained MLP-Mixer / ResMLP, drawn per key: Linears (the stem as one) at fan_in^-0.5, the second Linear of an
#: MLP at 0.5 fan_in^-0.5, LayerNorm gains near 1, small biases.  ResMLP's `ls1` / `ls2` are spread over 0.1 .. 0.4 with random signs,
#: `alpha` over 0.5 .. 1.5 and `beta` ~ 0.3 N(0, 1): far from timm's initial 1e-4 / 1 / 0 and from the ones and zeros a forgotten fold
#: would use.
MIXER_SYNTHETIC = [(ends(".ls1", ".ls2"), signed_uniform(0.1, 0.3)), (ends(".alpha"), uniform(0.5)), (ends(".beta"), normal(0.3)),
                   *fan_in_tail(ends("norm1.weight", "norm2.weight"), half=ends("fc2.weight"))]


def _mixer_twin(model_name: str, in_hw):
    """One twin per kind: the Mixer one follows the name's patch, the ResMLP one has 4 tokens."""
    kind, patch, _, _ = MIXER_MODELS[model_name]
    return mixer_tiny_twin(kind, patch if kind == "mixer" else 32, in_hw)


MIXER_FAMILY = Family("mixer", MixerSpec, MIXER_MODELS, is_mixer_name, mixer_named, _mixer_twin, "timm's MLP-Mixers and ResMLPs at 224 x 224",
                "blocks {}", True, MIXER_SYNTHETIC)


# ---------------------------------------------------------------------------
# the CaiT surrogates: self-attention blocks with talking-heads attention and LayerScale, planned on the transformer stack
# (include/i2v_cait.h)
# ---------------------------------------------------------------------------
#: timm 0.5.0's `Cait` models at 224 x 224 (patch 16, MLP ratio 4, head width 48): name -> (dim, self-attention blocks, heads).
CAIT_MODELS: Dict[str, Tuple[int, int, int]] = {
    "cait_xxs24_224": (192, 24, 4),
    "cait_xxs36_224": (192, 36, 4),
    "cait_s24_224": (384, 24, 8),
}


@dataclass
class CaitSpec(TokenSpec):
    """timm 0.5.0 `Cait` up to its last self-attention block: patch embedding (patch x patch convolution, stride
    patch, bias), pos_embed (tokens, dim) added, NO prefix token -- `cls_token` joins only in the two class-attention blocks, which lie
    behind the last hookable block and never run --, then `blocks` pre-norm blocks
      x += gamma_1 * proj(THA(LN1 x));  x += gamma_2 * fc2(GELU(fc1(LN2 x)))
    LayerNorm eps `ln_eps`, exact GELU, THA talking-heads attention: S_h = (scale q_h) k_h^T, S'_g = sum_h proj_l[g][h] S_h + bias,
    P = softmax over keys, P'_g = sum_h proj_w[g][h] P_h + bias, out_g = P'_g v_g, scale (dim / heads) ** -0.5.
    `hooks`: depth d (1..4) -> zero-based block d * blocks / 4 - 1 (5, 11, 17, 23 of 24; 8, 17, 26, 35 of 36), whose OUTPUT (the residual
    stream after it, all tokens) is the hooked feature: tokens * dim floats per frame, token-major."""
    arch: str
    img: int
    patch: int = 16
    in_chans: int = 3
    dim: int = 384
    heads: int = 8
    blocks: int = 24
    ln_eps: float = 1e-6
    hooks: Dict[int, int] = field(default_factory=dict)
    video: bool = False

    def __post_init__(self):
        if self.img % self.patch or self.patch % 4 or self.dim % self.heads or (self.dim // self.heads) % 4:
            raise ValueError(f"{self.arch}: a {self.img} x {self.img} frame, patch {self.patch}, width {self.dim}, {self.heads} heads: the "
                             "patch must divide the frame, and patch and head width must be multiples of 4")
        if self.blocks % 4:
            raise ValueError(f"{self.arch}: {self.blocks} blocks: depths 1..4 hook blocks d * blocks / 4 - 1")
        if not self.hooks:
            self.hooks = self.quarter_hooks()

    @property
    def tokens(self) -> int:
        return (self.img // self.patch) ** 2

    @property
    def mlp(self) -> int:
        return 4 * self.dim

    def hook_dim(self, i: int = 0) -> int:
        """Floats per frame of the feature hooked at block i (the same for every block)."""
        return self.tokens * self.dim

    def block_keys(self, i: int) -> List[str]:
        """timm's order: the block's own parameters (the LayerScale vectors) ahead of its children's."""
        p = f"blocks.{i}."
        return [p + k for k in ("gamma_1", "gamma_2", "norm1.weight", "norm1.bias", "attn.qkv.weight", "attn.qkv.bias", "attn.proj.weight",
                                "attn.proj.bias", "attn.proj_l.weight", "attn.proj_l.bias", "attn.proj_w.weight", "attn.proj_w.bias",
                                "norm2.weight", "norm2.bias", "mlp.fc1.weight", "mlp.fc1.bias", "mlp.fc2.weight", "mlp.fc2.bias")]

    def param_shapes(self) -> Dict[str, Tuple[int, ...]]:
        """timm `state_dict` key -> shape for every parameter up to the last self-attention block, in timm's order (`cls_token`,
        `blocks_token_only.*`, `norm.*` and `head.*` lie behind every hook and are not used)."""
        D, H, M = self.dim, self.heads, self.mlp
        out = {"pos_embed": (1, self.tokens, D), "patch_embed.proj.weight": (D, self.in_chans, self.patch, self.patch),
               "patch_embed.proj.bias": (D,)}
        shapes = [(D,), (D,), (D,), (D,), (3 * D, D), (3 * D,), (D, D), (D,), (H, H), (H,), (H, H), (H,), (D,), (D,), (M, D), (M,), (D, M), (D,)]
        for i in range(self.blocks):
            out.update(zip(self.block_keys(i), shapes))
        return out

    def native_arrays(self, sd, n_blocks: int) -> List["torch.Tensor"]:
        """The arrays `i2v_cait_create` takes for the first `n_blocks` blocks, from a timm-layout state dict, as float32 host tensors: the
        patch weight and bias, pos_embed as (tokens, dim), then 16 per block -- norm1, qkv, proj_l, proj_w as they lie, `attn.proj` with
        `gamma_1` folded in (row o of the weight and element o of the bias times gamma_1[o]), norm2, fc1, and `mlp.fc2` with `gamma_2`
        folded in the same way: LayerScale costs nothing at run time.  The folds are made in float64."""
        f = lambda k: sd[k].detach().float().cpu()      # noqa: E731
        out = [f("patch_embed.proj.weight").contiguous(), f("patch_embed.proj.bias").contiguous(),
               f("pos_embed").reshape(self.tokens, self.dim).contiguous()]
        for i in range(n_blocks):
            p = f"blocks.{i}."
            g1, g2 = f(p + "gamma_1").double(), f(p + "gamma_2").double()
            out += [f(p + k).contiguous() for k in ("norm1.weight", "norm1.bias", "attn.qkv.weight", "attn.qkv.bias", "attn.proj_l.weight",
                                                    "attn.proj_l.bias", "attn.proj_w.weight", "attn.proj_w.bias")]
            out += [(f(p + "attn.proj.weight").double() * g1[:, None]).float().contiguous(), (f(p + "attn.proj.bias").double() * g1).float().contiguous()]
            out += [f(p + k).contiguous() for k in ("norm2.weight", "norm2.bias", "mlp.fc1.weight", "mlp.fc1.bias")]
            out += [(f(p + "mlp.fc2.weight").double() * g2[:, None]).float().contiguous(), (f(p + "mlp.fc2.bias").double() * g2).float().contiguous()]
        return out

    def config_values(self):
        return (self.img, self.patch, self.in_chans, self.dim, self.heads, self.mlp, self.blocks, self.ln_eps)

    def macs_per_frame(self) -> int:
        T, D, M, H = self.tokens, self.dim, self.mlp, self.heads
        per_block = T * D * (3 * D + D + 2 * M) + 2 * T * T * D + 2 * T * T * H * H
        return T * D * self.in_chans * self.patch ** 2 + self.blocks * per_block

    def workspace_bytes(self, hook_blocks: Sequence[int], frames: int) -> int:
        """Device bytes `i2v_cait_create` plans for these hooks and `frames` frames (the formula of csrc/i2v_cait.cpp: the weights of the
        blocks run; per block its input, qkv, the probabilities, the mid stream, the fc1 pre-activation and four statistics per token;
        the shared scratch -- the last stream, two streams, one MLP-wide, TWO arrays of the probabilities' size, the qkv gradient, the
        patch rows; one gradient view per hook)."""
        D, M, T, H, nb = self.dim, self.mlp, self.tokens, self.heads, max(hook_blocks) + 1
        KP, FT = self.in_chans * self.patch ** 2, frames * T
        probs = frames * H * T * ((T + 3) // 4 * 4)
        weights = D * KP + D + T * D + nb * (4 * D * D + 2 * D * M + 9 * D + M + 2 * H * H + 2 * H)
        per_block = 5 * FT * D + probs + FT * M + 4 * FT
        shared = 6 * FT * D + FT * M + 2 * probs + FT * KP
        return 4 * (weights + nb * per_block + shared + len(hook_blocks) * FT * D)


def is_cait_name(model_name: str) -> bool:
    """A name of timm's CaiT vocabulary (`cait.py`), served (`CAIT_MODELS`) or not: `graphs.build` routes these to `cait_named`, which
    refuses the ones that are not offered with a message that lists the served names."""
    return model_name in CAIT_MODELS or model_name.startswith("cait")


def cait_named(model_name: str, in_hw=(224, 224)) -> CaitSpec:
    """Any row of `CAIT_MODELS`, at 224 x 224 only.  Refused, each with the reason: the 384 x 384 and 448 x 448 checkpoints
    (`cait_xxs24_384` ... `cait_m48_448`), and names outside the table."""
    served = "served: " + ", ".join(CAIT_MODELS)
    if model_name not in CAIT_MODELS:
        if model_name.endswith(("_384", "_448")):
            why = ("the 384 x 384 and 448 x 448 checkpoints are not offered (224 x 224 only: pos_embed is not interpolated, and 576 or "
                   "784 keys do not fit the attention tile)")
        else:
            why = "not a model of this table"
        raise ValueError(f"CaiT surrogate {model_name!r}: {why}; {served}")
    if tuple(in_hw) != (224, 224):
        raise ValueError(f"{model_name} takes 224 x 224 frames only (got {tuple(in_hw)[0]} x {tuple(in_hw)[1]}); "
                         "interpolating its pos_embed to another size is not supported")
    dim, blocks, heads = CAIT_MODELS[model_name]
    return CaitSpec(model_name, 224, 16, 3, dim, heads, blocks)


def cait_tiny_twin(in_hw=(64, 64)) -> CaitSpec:
    """The same topology at test size ("cait_test"): dim 32, 4 heads of width 8, 8 blocks, so depths 1..4 hook blocks 1, 3, 5, 7; square
    frames of a multiple of 16 pixels -- 16 tokens at 64 x 64, exactly one attention tile; 80 x 80 gives 25, a tile and a tail.  Not a
    row of `CAIT_MODELS`."""
    if in_hw[0] != in_hw[1] or in_hw[0] % 16:
        raise ValueError(f"the test-size CaiT takes square frames of a multiple of 16 pixels (got {tuple(in_hw)})")
    return CaitSpec("cait_test", int(in_hw[0]), 16, 3, 32, 4, 8)


def _mix_draw(shp, g):
    """A talking-heads mix: the identity plus 0.25 N(0, 1) per entry."""
    import torch
    return torch.eye(shp[0]) + 0.25 * torch.randn(*shp, generator=g)


#: Seeded stand-in for a trained CaiT, drawn per key so that every piece of the block's arithmetic shows in the hooks: Linears (the
#: patch embedding as one) ~ fan_in^-0.5 N(0, 1), which keeps a unit-variance stream and puts the attention logits at O(1); `attn.proj`
#: and `mlp.fc2` at half that; LayerNorm gains 1 + 0.1 N(0, 1); biases 0.02 N(0, 1); pos_embed 0.5 N(0, 1).  The LayerScale vectors
#: `gamma_1` / `gamma_2` are uniform on [0.5, 1] with random signs -- timm initialises them at 1e-5 or 1e-6, which would make every
#: block an identity and the tests blind to the kernel.  The talking-heads mixes `attn.proj_l.weight` / `attn.proj_w.weight` are the
#: identity plus 0.25 N(0, 1) per entry, with `proj_l.bias` ~ 0.5 N(0, 1) and `proj_w.bias` ~ 0.02 N(0, 1): far from the identity and
#: the zeros a skipped mix would compute.
CAIT_SYNTHETIC = [(ends(".gamma_1", ".gamma_2"), signed_uniform(0.5, 0.5)), (ends("proj_l.weight", "proj_w.weight"), _mix_draw),
                  (ends("proj_l.bias"), normal(0.5)), (keys("pos_embed"), normal(0.5)), *fan_in_tail(ends("norm1.weight", "norm2.weight"))]

CAIT_FAMILY = Family("cait", CaitSpec, CAIT_MODELS, is_cait_name, cait_named, lambda name, in_hw: cait_tiny_twin(in_hw),
                "timm's CaiTs at 224 x 224", "blocks {}", True, CAIT_SYNTHETIC)


# ---------------------------------------------------------------------------
# the ConViT surrogates: gated positional self-attention blocks, then plain blocks behind a class token that joins in mid-stream,
# planned on the transformer stack (include/i2v_convit.h)
# ---------------------------------------------------------------------------
#: timm 0.5.0's `ConViT` models at 224 x 224 (patch 16, 12 blocks of which the first 10 are GPSA, MLP ratio 4, head width 48, no qkv
#: bias): name -> (dim, heads).
CONVIT_MODELS: Dict[str, Tuple[int, int]] = {
    "convit_tiny": (192, 4),
    "convit_small": (432, 9),
    "convit_base": (768, 16),
}


@dataclass
class ConvitSpec(TokenSpec):
    """timm 0.5.0 `ConViT` up to its last block: patch embedding (patch x patch convolution, stride patch, bias),
    pos_embed (tokens, dim) added, then `blocks` pre-norm blocks  x += proj(attn(LN1 x));  x += fc2(GELU(fc1(LN2 x))),  LayerNorm eps
    `ln_eps`, exact GELU, no qkv bias.  Blocks 0 .. local_blocks - 1 run on the patch tokens with gated positional self-attention:
      P_h = (1 - sigma(g_h)) softmax(scale q_h k_h^T) + sigma(g_h) softmax_j(pos_proj_h . r_ij);  P_h /= sum_j P_h;  out_h = P_h v_h
    with r_ij = (jx - ix, jy - iy, squared distance) on the token grid.  Before block `local_blocks` the stream becomes [cls_token; x]
    (tokens + 1), and the remaining blocks use plain attention.
    `hooks`: depth d (1..4) -> zero-based block d * blocks / 4 - 1 (2, 5, 8, 11 of 12), whose OUTPUT (the residual stream after it, all
    tokens) is the hooked feature: tokens * dim floats per frame before the join, (tokens + 1) * dim behind it, token-major."""
    arch: str
    img: int
    patch: int = 16
    in_chans: int = 3
    dim: int = 192
    heads: int = 4
    blocks: int = 12
    local_blocks: int = 10
    ln_eps: float = 1e-6
    hooks: Dict[int, int] = field(default_factory=dict)
    video: bool = False

    def __post_init__(self):
        if self.img % self.patch or self.patch % 4 or self.dim % self.heads or (self.dim // self.heads) % 4:
            raise ValueError(f"{self.arch}: a {self.img} x {self.img} frame, patch {self.patch}, width {self.dim}, {self.heads} heads: the "
                             "patch must divide the frame, and patch and head width must be multiples of 4")
        if self.blocks % 4 or not 1 <= self.local_blocks <= self.blocks:
            raise ValueError(f"{self.arch}: {self.blocks} blocks, {self.local_blocks} of them local: depths 1..4 hook blocks d * blocks / 4 "
                             "- 1, and the class token joins before a block 1 .. blocks")
        if not self.hooks:
            self.hooks = self.quarter_hooks()

    @property
    def grid(self) -> int:
        return self.img // self.patch

    @property
    def tokens(self) -> int:
        """Patch tokens: what the stream holds before the class token joins."""
        return self.grid ** 2

    @property
    def mlp(self) -> int:
        return 4 * self.dim

    def tokens_at(self, i: int) -> int:
        """Tokens block i runs on, and the stream after it holds."""
        return self.tokens + (1 if i >= self.local_blocks else 0)

    def hook_shape(self, i: int):
        return (self.tokens_at(i), self.dim)

    def hook_dim(self, i: int = 0) -> int:
        """Floats per frame of the feature hooked at block i."""
        return self.tokens_at(i) * self.dim

    def block_keys(self, i: int) -> List[str]:
        """timm's order: norm1, the attention (`GPSA`: its own parameter gating_param first, as a state dict lists a module's own
        parameters ahead of its children's, then qk, v, proj, pos_proj as the constructor makes them; `MHSA`: qkv, proj), norm2, mlp."""
        p = f"blocks.{i}."
        attn = (("attn.gating_param", "attn.qk.weight", "attn.v.weight", "attn.proj.weight", "attn.proj.bias", "attn.pos_proj.weight",
                 "attn.pos_proj.bias") if i < self.local_blocks else ("attn.qkv.weight", "attn.proj.weight", "attn.proj.bias"))
        return [p + k for k in ("norm1.weight", "norm1.bias") + attn + ("norm2.weight", "norm2.bias", "mlp.fc1.weight", "mlp.fc1.bias",
                                                                       "mlp.fc2.weight", "mlp.fc2.bias")]

    def param_shapes(self) -> Dict[str, Tuple[int, ...]]:
        """timm `state_dict` key -> shape for every parameter up to the last block, in timm's order (`norm.*` and `head.*` lie behind
        every hook and are not used)."""
        D, H, M = self.dim, self.heads, self.mlp
        out = {"cls_token": (1, 1, D), "pos_embed": (1, self.tokens, D), "patch_embed.proj.weight": (D, self.in_chans, self.patch, self.patch),
               "patch_embed.proj.bias": (D,)}
        tail = [(D,), (D,), (M, D), (M,), (D, M), (D,)]
        for i in range(self.blocks):
            attn = [(H,), (2 * D, D), (D, D), (D, D), (D,), (H, 3), (H,)] if i < self.local_blocks else [(3 * D, D), (D, D), (D,)]
            out.update(zip(self.block_keys(i), [(D,), (D,)] + attn + tail))
        return out

    def rel_indices(self) -> "torch.Tensor":
        """r_ij (tokens, tokens, 3) in float64: (jx - ix, jy - iy, (jx - ix)^2 + (jy - iy)^2) for token = y * grid + x."""
        import torch
        t = torch.arange(self.tokens)
        x, y = (t % self.grid).double(), (t // self.grid).double()
        dx, dy = x[None, :] - x[:, None], y[None, :] - y[:, None]
        return torch.stack([dx, dy, dx * dx + dy * dy], -1)

    def gate_table(self, sd, i: int):
        """(c (heads), A (heads, tokens, ld)) of GPSA block i in float32, computed in float64: A_h = sigma(g_h) softmax_j(w_h . r_ij) with
        rows zero-padded to ld = tokens rounded up to 4, c_h = 1 - sigma(g_h).  `pos_proj.bias` is constant along j and cancels inside
        the softmax, so it is not read."""
        import torch
        p = f"blocks.{i}.attn."
        sig = torch.sigmoid(sd[p + "gating_param"].detach().double().cpu())
        pos = torch.einsum("ijk,hk->hij", self.rel_indices(), sd[p + "pos_proj.weight"].detach().double().cpu()).softmax(-1)
        T, ld = self.tokens, (self.tokens + 3) // 4 * 4
        A = torch.zeros(self.heads, T, ld, dtype=torch.float64)
        A[:, :, :T] = sig[:, None, None] * pos
        return (1.0 - sig).float().contiguous(), A.float().contiguous()

    def native_arrays(self, sd, n_blocks: int) -> List["torch.Tensor"]:
        """The arrays `i2v_convit_create` takes for the first `n_blocks` blocks, from a timm-layout state dict, as float32 host tensors:
        the patch weight and bias, pos_embed as (tokens, dim), cls_token as (dim); per GPSA block 14 -- norm1, `attn.qk.weight` and
        `attn.v.weight` stacked into one (3 dim, dim) array (q of head h at row h dh, k at dim + h dh, v at 2 dim + h dh: the layout of
        a plain qkv), a zero (3 dim) bias, `gate_table`'s c and A, proj, norm2, fc1, fc2 --; per plain block 12 -- the same with
        `attn.qkv.weight` as it lies and without c and A."""
        import torch
        f = lambda k: sd[k].detach().float().cpu()      # noqa: E731
        out = [f("patch_embed.proj.weight").contiguous(), f("patch_embed.proj.bias").contiguous(),
               f("pos_embed").reshape(self.tokens, self.dim).contiguous(), f("cls_token").reshape(self.dim).contiguous()]
        tail = ("attn.proj.weight", "attn.proj.bias", "norm2.weight", "norm2.bias", "mlp.fc1.weight", "mlp.fc1.bias", "mlp.fc2.weight",
                "mlp.fc2.bias")
        for i in range(n_blocks):
            p = f"blocks.{i}."
            out += [f(p + "norm1.weight").contiguous(), f(p + "norm1.bias").contiguous()]
            if i < self.local_blocks:
                out += [torch.cat([f(p + "attn.qk.weight"), f(p + "attn.v.weight")], 0).contiguous(), torch.zeros(3 * self.dim)]
                out += list(self.gate_table(sd, i))
            else:
                out += [f(p + "attn.qkv.weight").contiguous(), torch.zeros(3 * self.dim)]
            out += [f(p + k).contiguous() for k in tail]
        return out

    def config_values(self):
        return (self.img, self.patch, self.in_chans, self.dim, self.heads, self.mlp, self.blocks, self.local_blocks, self.ln_eps)

    def macs_per_frame(self) -> int:
        D, M = self.dim, self.mlp
        total = self.tokens * D * self.in_chans * self.patch ** 2
        for i in range(self.blocks):
            T = self.tokens_at(i)
            total += T * D * (3 * D + D + 2 * M) + 2 * T * T * D
        return total

    def workspace_bytes(self, hook_blocks: Sequence[int], frames: int) -> int:
        """Device bytes `i2v_convit_create` plans for these hooks and `frames` frames (the formula of csrc/i2v_convit.cpp).  With T_b
        the tokens of block b, ld_b = T_b rounded up to 4 and T_m those of the deepest block run: the weights of the blocks run (a GPSA
        block adds heads + heads * tokens * ld floats); per block its input, qkv, the probabilities, the mid stream, the fc1
        pre-activation and four statistics per token, at T_b; the shared scratch at T_m -- the last stream, two streams, one MLP-wide,
        ONE array of the probabilities' size, the qkv gradient --, the patch rows, and two streams of patch tokens where blocks follow
        the join; one gradient view per hook at its own token count."""
        D, M, T, H, nb = self.dim, self.mlp, self.tokens, self.heads, max(hook_blocks) + 1
        KP, ld = self.in_chans * self.patch ** 2, (T + 3) // 4 * 4
        nl = min(nb, self.local_blocks)
        weights = D * KP + D + T * D + D + nb * (4 * D * D + 2 * D * M + 9 * D + M) + nl * (H + H * T * ld)
        saves = 0
        for b in range(nb):
            Tb = self.tokens_at(b)
            saves += frames * (Tb * (5 * D + M + 4) + H * Tb * ((Tb + 3) // 4 * 4))
        Tm = self.tokens_at(nb - 1)
        shared = frames * (Tm * (6 * D + M) + H * Tm * ((Tm + 3) // 4 * 4) + T * KP + (2 * T * D if nb > nl else 0))
        hooks = sum(frames * self.tokens_at(b) * D for b in hook_blocks)
        return 4 * (weights + saves + shared + hooks)


def is_convit_name(model_name: str) -> bool:
    """A name of timm's ConViT vocabulary (`convit.py`), served (`CONVIT_MODELS`) or not: `graphs.build` routes these to `convit_named`,
    which refuses the ones that are not offered with a message that lists the served names."""
    return model_name in CONVIT_MODELS or model_name.startswith("convit")


def convit_named(model_name: str, in_hw=(224, 224)) -> ConvitSpec:
    """Any row of `CONVIT_MODELS`, at 224 x 224 only; names outside the table are refused with the reason."""
    if model_name not in CONVIT_MODELS:
        raise ValueError(f"ConViT surrogate {model_name!r}: not a model of this table; served: " + ", ".join(CONVIT_MODELS))
    if tuple(in_hw) != (224, 224):
        raise ValueError(f"{model_name} takes 224 x 224 frames only (got {tuple(in_hw)[0]} x {tuple(in_hw)[1]}); its positional "
                         "attention and pos_embed are tied to the 14 x 14 token grid; served: " + ", ".join(CONVIT_MODELS))
    dim, heads = CONVIT_MODELS[model_name]
    return ConvitSpec(model_name, 224, 16, 3, dim, heads, 12, 10)


def convit_tiny_twin(in_hw=(64, 64)) -> ConvitSpec:
    """The same topology at test size ("convit_test"): dim 32, 4 heads of width 8, 8 blocks of which the first 6 are GPSA, so depths
    1..4 hook blocks 1, 3, 5, 7 and depth 4 crosses the join; square frames of a multiple of 16 pixels -- 16 tokens at 64 x 64, exactly
    one attention tile, and 25 at 80 x 80, a tile and a tail; 17 / 26 behind the join.  Not a row of `CONVIT_MODELS`."""
    if in_hw[0] != in_hw[1] or in_hw[0] % 16:
        raise ValueError(f"the test-size ConViT takes square frames of a multiple of 16 pixels (got {tuple(in_hw)})")
    return ConvitSpec("convit_test", int(in_hw[0]), 16, 3, 32, 4, 8, 6)


def _pos_proj_draw(shp, g):
    """timm's local initialisation of `attn.pos_proj.weight` plus seeded noise (see `CONVIT_SYNTHETIC`)."""
    import torch
    H = shp[0]
    ks = int(H ** 0.5)
    centre = (ks - 1) / 2 if ks % 2 == 0 else ks // 2
    w = torch.zeros(H, 3)
    for h1 in range(ks):
        for h2 in range(ks):
            w[h1 + ks * h2] = torch.tensor([2.0 * (h2 - centre), 2.0 * (h1 - centre), -1.0])
    return w + torch.randn(H, 3, generator=g) * torch.tensor([0.3, 0.3, 0.1])


#: Seeded stand-in for a trained ConViT, drawn per key as CaiT's is: Linears ~ fan_in^-0.5 N(0, 1) (`attn.proj` and `mlp.fc2` at half
#: that), LayerNorm gains 1 + 0.1 N(0, 1), biases 0.02 N(0, 1), pos_embed and cls_token 0.5 N(0, 1).  `attn.v` is an ordinary Linear
#: draw, not timm's identity.  `attn.pos_proj.weight` is timm's local initialisation -- column 2 = -1, and columns 0 / 1 on the head's
#: offset in a floor(sqrt(heads)) grid: head p = h1 + k h2 gets column 1 = 2 (h1 - centre) and column 0 = 2 (h2 - centre) -- plus seeded
#: noise, 0.3 N(0, 1) on the two offset columns and 0.1 N(0, 1) on the distance column, so that the x and y columns of every head
#: differ and a transposed grid convention shows.  `attn.gating_param` ~ N(0, 1), so sigma(g) spans the range (timm starts it at 1);
#: `attn.pos_proj.bias` ~ 0.5 N(0, 1), far from the zero a dropped bias would equal.
CONVIT_SYNTHETIC = [(ends("pos_proj.weight"), _pos_proj_draw), (ends("gating_param"), normal()), (ends("pos_proj.bias"), normal(0.5)),
                    (keys("pos_embed", "cls_token"), normal(0.5)), *fan_in_tail(ends("norm1.weight", "norm2.weight"))]

CONVIT_FAMILY = Family("convit", ConvitSpec, CONVIT_MODELS, is_convit_name, convit_named, lambda name, in_hw: convit_tiny_twin(in_hw),
                "timm's ConViTs at 224 x 224", "blocks {}", True, CONVIT_SYNTHETIC)


# ---------------------------------------------------------------------------
# the XCiT surrogates: cross-covariance attention (channels attend to channels), a convolutional stem and a depthwise "local patch
# interaction" per block, planned on the transformer stack (include/i2v_xcit.h)
# ---------------------------------------------------------------------------
_XCIT_BASE: Dict[str, Tuple[int, int, int]] = {
    "xcit_nano_12_p16_224": (128, 12, 4),
    "xcit_tiny_12_p16_224": (192, 12, 4),
    "xcit_tiny_24_p16_224": (192, 24, 4),
    "xcit_small_12_p16_224": (384, 12, 8),
    "xcit_small_24_p16_224": (384, 24, 8),
    "xcit_medium_24_p16_224": (512, 24, 8),
    "xcit_large_24_p16_224": (768, 24, 16),
}
#: timm 0.5.0's `XCiT` models at 224 x 224 with patch 16 (MLP ratio 4, qkv bias, LayerScale): name -> (dim, blocks, heads).  Each name has
#: a `_dist` twin: the same architecture (no distillation token), its own checkpoint file.
XCIT_MODELS: Dict[str, Tuple[int, int, int]] = {**_XCIT_BASE, **{k + "_dist": v for k, v in _XCIT_BASE.items()}}

BN2D_EPS = 1e-5      # torch's BatchNorm2d default: the stem's and the local patch interaction's


@dataclass
class XcitSpec(TokenSpec):
    """timm 0.5.0 `XCiT` up to its last cross-covariance block.  Stem: four 3 x 3 / stride 2 / pad 1 convolutions
    without bias (widths dim / 8, dim / 4, dim / 2, dim), each followed by an eval-mode BatchNorm2d, the first three by the exact GELU;
    then + the Fourier position features of the token grid through a 1 x 1 convolution.  Then `blocks` blocks, LayerNorm eps `ln_eps`:
      x += gamma1 proj(XCA(norm1 x));  x += gamma3 LPI(norm3 x);  x += gamma2 fc2(gelu(fc1(norm2 x)))
    XCA: per head the (dh, dh) softmax of temperature * (q / ||q||)^T (k / ||k||), the norms taken per column over the tokens, applied to
    v's columns.  LPI on the grid: depthwise 3 x 3 with bias, GELU, eval-mode BatchNorm2d, depthwise 3 x 3 with bias.
    `hooks`: depth d (1..4) -> zero-based block d * blocks / 4 - 1, whose OUTPUT (the residual stream after it) is the hooked feature:
    tokens * dim floats per frame, token-major.  The class-attention blocks, `cls_token`, `norm.*` and `head.*` lie behind every hook."""
    arch: str
    img: int
    in_chans: int = 3
    dim: int = 192
    heads: int = 4
    blocks: int = 12
    ln_eps: float = 1e-6
    hooks: Dict[int, int] = field(default_factory=dict)
    video: bool = False

    def __post_init__(self):
        if self.img % 16 or self.dim % 8 or self.dim % self.heads or (self.dim // self.heads) % 4 or self.dim // self.heads > 64:
            raise ValueError(f"{self.arch}: a {self.img} x {self.img} frame, width {self.dim}, {self.heads} heads: the frame must be a multiple "
                             "of 16 pixels, the width of 8, and the head width a multiple of 4 up to 64")
        if self.blocks % 4:
            raise ValueError(f"{self.arch}: {self.blocks} blocks: depths 1..4 hook blocks d * blocks / 4 - 1")
        if not self.hooks:
            self.hooks = self.quarter_hooks()

    patch = 16

    @property
    def grid(self) -> int:
        return self.img // 16

    @property
    def tokens(self) -> int:
        return self.grid ** 2

    @property
    def mlp(self) -> int:
        return 4 * self.dim

    @property
    def stem_widths(self) -> List[int]:
        return [self.in_chans, self.dim // 8, self.dim // 4, self.dim // 2, self.dim]

    def hook_dim(self, i: int = 0) -> int:
        return self.tokens * self.dim

    def block_keys(self, i: int) -> List[str]:
        """timm's order: the block's own parameters gamma1, gamma3, gamma2 first, then norm1, attn (its own `temperature` first), norm3,
        local_mp, norm2, mlp.  `local_mp.bn.num_batches_tracked` is not read."""
        p = f"blocks.{i}."
        return [p + k for k in ("gamma1", "gamma3", "gamma2", "norm1.weight", "norm1.bias", "attn.temperature", "attn.qkv.weight",
                                "attn.qkv.bias", "attn.proj.weight", "attn.proj.bias", "norm3.weight", "norm3.bias", "local_mp.conv1.weight",
                                "local_mp.conv1.bias", "local_mp.bn.weight", "local_mp.bn.bias", "local_mp.bn.running_mean",
                                "local_mp.bn.running_var", "local_mp.conv2.weight", "local_mp.conv2.bias", "norm2.weight", "norm2.bias",
                                "mlp.fc1.weight", "mlp.fc1.bias", "mlp.fc2.weight", "mlp.fc2.bias")]

    def param_shapes(self) -> Dict[str, Tuple[int, ...]]:
        """timm `state_dict` key -> shape for every parameter and BatchNorm statistic up to the last block, in timm's order."""
        D, H, M, cs = self.dim, self.heads, self.mlp, self.stem_widths
        out = {}
        for k in range(4):
            p = f"patch_embed.proj.{2 * k}."
            out[p + "0.weight"] = (cs[k + 1], cs[k], 3, 3)
            out.update({p + "1." + n: (cs[k + 1],) for n in ("weight", "bias", "running_mean", "running_var")})
        out["pos_embeder.token_projection.weight"] = (D, 64, 1, 1)
        out["pos_embeder.token_projection.bias"] = (D,)
        shapes = [(D,), (D,), (D,), (D,), (D,), (H, 1, 1), (3 * D, D), (3 * D,), (D, D), (D,), (D,), (D,), (D, 1, 3, 3), (D,), (D,), (D,), (D,),
                  (D,), (D, 1, 3, 3), (D,), (D,), (D,), (M, D), (M,), (D, M), (D,)]
        for i in range(self.blocks):
            out.update(zip(self.block_keys(i), shapes))
        return out

    def fourier_features(self) -> "torch.Tensor":
        """(tokens, 64) in float64: timm's `PositionalEncodingFourier` before its 1 x 1 convolution -- hidden 32 per axis, temperature
        10000, scale 2 pi, coordinates 1 .. grid divided by (grid + 1e-6); sin on even feature indices and cos on odd; y features first."""
        import math
        import torch
        g = self.grid
        coord = torch.arange(1, g + 1, dtype=torch.float64) / (g + 1e-6) * (2 * math.pi)
        i = torch.arange(32, dtype=torch.float64)
        dim_t = 10000.0 ** (2 * torch.div(i, 2, rounding_mode="floor") / 32)
        arg = coord[:, None] / dim_t[None, :]                                   # (g, 32)
        feat = torch.where((torch.arange(32) % 2 == 0)[None, :], arg.sin(), arg.cos())
        fy = feat[:, None, :].expand(g, g, 32)                                  # token (y, x): y features, then x features
        fx = feat[None, :, :].expand(g, g, 32)
        return torch.cat([fy, fx], -1).reshape(g * g, 64)

    def native_arrays(self, sd, n_blocks: int) -> List["torch.Tensor"]:
        """The arrays `i2v_xcit_create` takes for the first `n_blocks` blocks, from a timm-layout state dict, as float32 host tensors,
        folded in float64: per stem convolution the BatchNorm-folded weight as (C_out, 9 C_in) with column (3 ky + kx) C_in + c and the
        bias; the position table (tokens, dim); per block 21 -- norm1, qkv, temperature (heads), gamma1-folded proj, norm2, fc1,
        gamma2-folded fc2, norm3, conv1 as (9, dim) and its bias, the LPI BatchNorm as (a, s), gamma3-folded conv2 as (9, dim) and bias.
        The LPI BatchNorm cannot go into conv2: conv2 pads the BatchNorm's OUTPUT with zeros, so a tap outside the plane adds 0, not s."""
        import torch
        d = lambda k: sd[k].detach().double().cpu()      # noqa: E731
        f32 = lambda t: t.float().contiguous()           # noqa: E731
        out = []
        for k in range(4):
            p = f"patch_embed.proj.{2 * k}."
            s = d(p + "1.weight") / torch.sqrt(d(p + "1.running_var") + BN2D_EPS)
            w = d(p + "0.weight") * s[:, None, None, None]
            out += [f32(w.permute(0, 2, 3, 1).reshape(w.shape[0], -1)), f32(d(p + "1.bias") - d(p + "1.running_mean") * s)]
        wp = d("pos_embeder.token_projection.weight").reshape(self.dim, 64)
        out.append(f32(self.fourier_features() @ wp.t() + d("pos_embeder.token_projection.bias")))
        D = self.dim
        for i in range(n_blocks):
            p = f"blocks.{i}."
            g1, g2, g3 = d(p + "gamma1"), d(p + "gamma2"), d(p + "gamma3")
            a = d(p + "local_mp.bn.weight") / torch.sqrt(d(p + "local_mp.bn.running_var") + BN2D_EPS)
            out += [f32(d(p + "norm1.weight")), f32(d(p + "norm1.bias")), f32(d(p + "attn.qkv.weight")), f32(d(p + "attn.qkv.bias")),
                    f32(d(p + "attn.temperature").reshape(self.heads)),
                    f32(d(p + "attn.proj.weight") * g1[:, None]), f32(d(p + "attn.proj.bias") * g1),
                    f32(d(p + "norm2.weight")), f32(d(p + "norm2.bias")), f32(d(p + "mlp.fc1.weight")), f32(d(p + "mlp.fc1.bias")),
                    f32(d(p + "mlp.fc2.weight") * g2[:, None]), f32(d(p + "mlp.fc2.bias") * g2),
                    f32(d(p + "norm3.weight")), f32(d(p + "norm3.bias")),
                    f32(d(p + "local_mp.conv1.weight").reshape(D, 9).t()), f32(d(p + "local_mp.conv1.bias")),
                    f32(a), f32(d(p + "local_mp.bn.bias") - d(p + "local_mp.bn.running_mean") * a),
                    f32((d(p + "local_mp.conv2.weight").reshape(D, 9) * g3[:, None]).t()), f32(d(p + "local_mp.conv2.bias") * g3)]
        return out

    def config_values(self):
        return (self.img, self.in_chans, self.dim, self.heads, self.mlp, self.blocks, self.ln_eps)

    def macs_per_frame(self) -> int:
        D, M, T, cs = self.dim, self.mlp, self.tokens, self.stem_widths
        total = sum((self.img >> (k + 1)) ** 2 * 9 * cs[k] * cs[k + 1] for k in range(4))
        return total + self.blocks * (T * D * (3 * D + D + 2 * M) + 2 * T * D * (D // self.heads) + 18 * T * D)

    def workspace_bytes(self, hook_blocks: Sequence[int], frames: int) -> int:
        """Device bytes `i2v_xcit_create` plans for these hooks and `frames` frames (the formula of csrc/i2v_xcit.cpp): the folded stem
        weights and the position table; per block run its 21 arrays and the two mirrored (9, dim) filters; the stem's gathered rows (the
        largest of the four stages) and the pre-activation and GELU planes of its first three stages; per block its input, qkv, the
        normalised Gram with two rows of norms, the probabilities, the two mid streams, the LPI pre-activation, the fc1 pre-activation
        and six statistics per token; the shared scratch -- the last stream, two streams, one MLP-wide, one qkv-wide --; one gradient
        view per hook."""
        D, M, T, H, nb, cs = self.dim, self.mlp, self.tokens, self.heads, max(hook_blocks) + 1, self.stem_widths
        dh = D // H
        planes = [(self.img >> (k + 1)) ** 2 for k in range(4)]
        weights = sum(cs[k + 1] * 9 * cs[k] + cs[k + 1] for k in range(4)) + T * D + nb * (12 * D * D + 37 * D + H + 18 * D)
        stem = frames * (max(planes[k] * 9 * cs[k] for k in range(4)) + 2 * sum(planes[k] * cs[k + 1] for k in range(3)))
        saves = nb * frames * (T * (11 * D + 6) + H * dh * (2 * dh + 2))
        shared = frames * T * (6 * D + M)
        return 4 * (weights + stem + saves + shared + len(hook_blocks) * frames * T * D)


def is_xcit_name(model_name: str) -> bool:
    """A name of timm's XCiT vocabulary (`xcit.py`), served (`XCIT_MODELS`) or not: `graphs.build` routes these to `xcit_named`, which
    refuses the ones that are not offered with a message that lists the served names."""
    return model_name.startswith("xcit")


def xcit_named(model_name: str, in_hw=(224, 224)) -> XcitSpec:
    """Any row of `XCIT_MODELS`, at 224 x 224 only; names outside the table are refused with the reason."""
    served = "; served: " + ", ".join(XCIT_MODELS)
    if model_name not in XCIT_MODELS:
        why = "not a model of this table"
        if "_p8_" in model_name:
            why += " (patch 8: a three-convolution stem and 784 tokens, not planned)"
        elif "_384" in model_name:
            why += " (384 x 384 frames: only the 224 x 224 models are served)"
        raise ValueError(f"XCiT surrogate {model_name!r}: {why}" + served)
    if tuple(in_hw) != (224, 224):
        raise ValueError(f"{model_name} takes 224 x 224 frames only (got {tuple(in_hw)[0]} x {tuple(in_hw)[1]}); its checkpoint is the "
                         "224 x 224 model's" + served)
    dim, blocks, heads = XCIT_MODELS[model_name]
    return XcitSpec(model_name, 224, 3, dim, heads, blocks)


def xcit_tiny_twin(in_hw=(64, 64)) -> XcitSpec:
    """The same topology at test size, 8 blocks (depths 1..4 hook blocks 1, 3, 5, 7): "xcit_test" on square frames of a multiple of 16
    pixels -- at 64 x 64 4 x 4 = 16 tokens, dim 32, 4 heads of 8 -- and "xcit_test_80" at 80 x 80 -- 5 x 5 = 25 tokens (an odd plane, no
    multiple of 4 or 16), dim 48, 4 heads of 12, stem rows of 27 / 54 / 108 / 216.  Not rows of `XCIT_MODELS`."""
    if in_hw[0] != in_hw[1] or in_hw[0] % 16:
        raise ValueError(f"the test-size XCiT takes square frames of a multiple of 16 pixels (got {tuple(in_hw)})")
    if int(in_hw[0]) == 80:
        return XcitSpec("xcit_test_80", 80, 3, 48, 4, 8)
    return XcitSpec("xcit_test", int(in_hw[0]), 3, 32, 4, 8)


#: timm renamed XCiT's `pos_embeder` to `pos_embed` after 0.5.0: the later spelling of the same two arrays is accepted
XCIT_KEY_ALIASES = {"pos_embed.token_projection.weight": "pos_embeder.token_projection.weight",
                    "pos_embed.token_projection.bias": "pos_embeder.token_projection.bias"}

#: Seeded stand-in for a trained XCiT, drawn per key as CaiT's is: Linears and convolutions ~ fan_in^-0.5 N(0, 1) (`attn.proj` and
#: `mlp.fc2` at half that), LayerNorm gains 1 + 0.1 N(0, 1), biases 0.02 N(0, 1) -- the depthwise convolutions' 0.1 N(0, 1), so that a
#: dropped bias shows --, BatchNorm gains uniform on (0.5, 1.5), shifts and running means 0.1 N(0, 1), running variances uniform on
#: (0.5, 1.5).  The LayerScales gamma1 / gamma2 / gamma3 are uniform on (0.5, 1.5) -- timm starts them at 1 (or 1e-5 for the 24-block
#: models) and they train away from it --, each drawn on its own so that exchanging two of them shows; `attn.temperature` is uniform on
#: (0.5, 4), so that the softmax over channels is neither flat nor one-hot.
XCIT_SYNTHETIC = [
    (lambda k: k.endswith(("gamma1", "gamma2", "gamma3", "running_var")) or ".bn.weight" in k
     or (k.startswith("patch_embed") and k.endswith("1.weight")), uniform(0.5)),
    (ends("temperature"), uniform(0.5, 3.5)),
    (lambda k: k.endswith("running_mean") or ".bn.bias" in k or (k.startswith("patch_embed") and k.endswith("1.bias")), normal(0.1)),
    (ends("conv1.bias", "conv2.bias"), normal(0.1)),
    *fan_in_tail(ends("norm1.weight", "norm2.weight", "norm3.weight"))]

XCIT_FAMILY = Family("xcit", XcitSpec, XCIT_MODELS, is_xcit_name, xcit_named, lambda name, in_hw: xcit_tiny_twin(in_hw),
                "timm's XCiTs at 224 x 224 with patch 16", "blocks {}", True, XCIT_SYNTHETIC, key_aliases=XCIT_KEY_ALIASES)


# ---------------------------------------------------------------------------
# the Twins surrogates: a four-stage pyramid whose global attention takes its keys from a sub-sampled plane (rectangular attention),
# with a depthwise conditional position encoding per stage, planned on the transformer stack (include/i2v_twins.h)
# ---------------------------------------------------------------------------
#: timm 0.5.0's `Twins` models at 224 x 224 (patch sizes 4, 2, 2, 2; sr_ratios 8, 4, 2, 1): name -> (dims, heads, MLP ratios, depths,
#: window).  Window 0 (PCPVT): every block is global sub-sampled attention; window 7 (SVT): block j of a stage is locally-grouped
#: attention for even j and global sub-sampled attention for odd j.
TWINS_MODELS: Dict[str, Tuple[Tuple[int, ...], Tuple[int, ...], Tuple[int, ...], Tuple[int, ...], int]] = {
    "twins_pcpvt_small": ((64, 128, 320, 512), (1, 2, 5, 8), (8, 8, 4, 4), (3, 4, 6, 3), 0),
    "twins_pcpvt_base": ((64, 128, 320, 512), (1, 2, 5, 8), (8, 8, 4, 4), (3, 4, 18, 3), 0),
    "twins_pcpvt_large": ((64, 128, 320, 512), (1, 2, 5, 8), (8, 8, 4, 4), (3, 8, 27, 3), 0),
    "twins_svt_small": ((64, 128, 256, 512), (2, 4, 8, 16), (4, 4, 4, 4), (2, 2, 10, 4), 7),
    "twins_svt_base": ((96, 192, 384, 768), (3, 6, 12, 24), (4, 4, 4, 4), (2, 2, 18, 2), 7),
    "twins_svt_large": ((128, 256, 512, 1024), (4, 8, 16, 32), (4, 4, 4, 4), (2, 2, 18, 2), 7),
}


@dataclass
class TwinsSpec(StagedSpec):
    """timm 0.5.0 `Twins` up to its last block.  Stage k: `patch_embeds.k`, a convolution with kernel = stride =
    patch (4 for stage 0, 2 after) and LayerNorm eps `pe_eps`; then `depths[k]` pre-norm blocks at width `dims[k]` (norms eps `ln_eps`,
    exact GELU, MLP ratio `mlp_ratios[k]`); `pos_block.k` after block 0: x += dwconv3x3(x) + bias on the grid.
    Block j's attention is global sub-sampled attention (GSA) where `window` is 0 or j is odd: `attn.q`, and `attn.kv` applied to the
    plane after `attn.sr` (a convolution with kernel = stride = sr_ratios[k]) and `attn.norm` (eps `pe_eps`) where sr > 1 -- grid^2
    queries against (grid / sr)^2 keys --; else locally-grouped attention (LSA): `attn.qkv` inside window x window windows, no shift
    and no bias table.
    `hooks`: depth d (1..4) -> zero-based stage d - 1, whose last block's OUTPUT, before the next patch embedding, is the hooked
    feature: grid_k^2 * dims[k] floats per frame, token-major.  `norm.*` and `head.*` lie behind every hook."""
    arch: str
    img: int
    dims: Tuple[int, ...] = (64, 128, 320, 512)
    heads: Tuple[int, ...] = (1, 2, 5, 8)
    mlp_ratios: Tuple[int, ...] = (8, 8, 4, 4)
    depths: Tuple[int, ...] = (3, 4, 6, 3)
    window: int = 0
    sr_ratios: Tuple[int, ...] = (8, 4, 2, 1)
    in_chans: int = 3
    patch: int = 4
    ln_eps: float = 1e-6
    pe_eps: float = 1e-5
    hooks: Dict[int, int] = field(default_factory=dict)
    video: bool = False

    def __post_init__(self):
        self.dims, self.heads, self.mlp_ratios = tuple(self.dims), tuple(self.heads), tuple(self.mlp_ratios)
        self.depths, self.sr_ratios = tuple(self.depths), tuple(self.sr_ratios)
        if not (len(self.dims) == len(self.heads) == len(self.mlp_ratios) == len(self.depths) == len(self.sr_ratios) == 4):
            raise ValueError(f"{self.arch}: dims, heads, MLP ratios, depths and sr_ratios must name the same 4 stages")
        for k in range(4):
            g, sr, dh = self.grid(k), self.sr_ratios[k], self.dims[k] // self.heads[k]
            if g * (self.patch << k) != self.img or g % sr or (g // sr) ** 2 > 64:
                raise ValueError(f"{self.arch}: a {self.img} x {self.img} frame does not give stage {k} a grid of whole {sr} x {sr} "
                                 "blocks with at most 64 of them")
            if self.dims[k] % self.heads[k] or dh % 4 or dh > 64:
                raise ValueError(f"{self.arch}: width {self.dims[k]} of stage {k} under {self.heads[k]} heads: the head width must be "
                                 "a multiple of 4 up to 64")
            if self.window and (g % self.window or (self.window, dh) not in ((7, 32), (4, 16))):
                raise ValueError(f"{self.arch}: stage {k} (grid {g}, head width {dh}) under window {self.window}: whole windows of 7 "
                                 "at head width 32 or of 4 at head width 16")
        if not self.hooks:
            self.hooks = {d: d - 1 for d in (1, 2, 3, 4)}

    stages = 4

    def grid(self, k: int) -> int:
        return (self.img // self.patch) >> k

    def width(self, k: int) -> int:
        return self.dims[k]

    def tokens(self, k: int) -> int:
        return self.grid(k) ** 2

    def keys_per_frame(self, k: int) -> int:
        """Keys (and values) a query of stage k's global sub-sampled attention attends to."""
        return (self.grid(k) // self.sr_ratios[k]) ** 2

    def mlp(self, k: int) -> int:
        return self.mlp_ratios[k] * self.dims[k]

    def is_lsa(self, k: int, j: int) -> bool:
        """Block j of stage k is locally-grouped (window) attention."""
        return bool(self.window) and j % 2 == 0

    def hook_dim(self, k: int) -> int:
        """Floats per frame of the feature hooked at stage k."""
        return self.tokens(k) * self.dims[k]

    def embed_keys(self, k: int) -> List[str]:
        p = f"patch_embeds.{k}."
        return [p + "proj.weight", p + "proj.bias", p + "norm.weight", p + "norm.bias"]

    def block_keys(self, k: int, j: int) -> List[str]:
        """timm's order: norm1, attn (GSA: q, kv, proj, then sr and norm where sr > 1; LSA: qkv, proj), norm2, mlp."""
        if self.is_lsa(k, j):
            attn = ["attn.qkv.weight", "attn.qkv.bias", "attn.proj.weight", "attn.proj.bias"]
        else:
            attn = ["attn.q.weight", "attn.q.bias", "attn.kv.weight", "attn.kv.bias", "attn.proj.weight", "attn.proj.bias"]
            if self.sr_ratios[k] > 1:
                attn += ["attn.sr.weight", "attn.sr.bias", "attn.norm.weight", "attn.norm.bias"]
        p = f"blocks.{k}.{j}."
        return [p + n for n in ["norm1.weight", "norm1.bias"] + attn + ["norm2.weight", "norm2.bias", "mlp.fc1.weight", "mlp.fc1.bias",
                                                                       "mlp.fc2.weight", "mlp.fc2.bias"]]

    def peg_keys(self, k: int) -> List[str]:
        return [f"pos_block.{k}.proj.0.weight", f"pos_block.{k}.proj.0.bias"]

    def native_block_keys(self, k: int, j: int) -> List[str]:
        """The block's keys in the order `i2v_twins_create` takes them: as timm's, but `attn.sr` and `attn.norm` in front of
        `attn.proj`, where the forward runs them."""
        keys = self.block_keys(k, j)
        sub = [key for key in keys if ".attn.sr." in key or ".attn.norm." in key]
        rest = [key for key in keys if key not in sub]
        at = next(i for i, key in enumerate(rest) if key.endswith("attn.proj.weight"))
        return rest[:at] + sub + rest[at:]

    def param_shapes(self) -> Dict[str, Tuple[int, ...]]:
        """timm `state_dict` key -> shape for every parameter up to the last block, in timm's order: all patch embeddings, all blocks,
        all position encodings."""
        out = {}
        for k in range(4):
            D, Cin, P = self.dims[k], self.dims[k - 1] if k else self.in_chans, 2 if k else self.patch
            out.update(zip(self.embed_keys(k), [(D, Cin, P, P), (D,), (D,), (D,)]))
        for k in range(4):
            D, M, sr = self.dims[k], self.mlp(k), self.sr_ratios[k]
            tail = {"norm2.weight": (D,), "norm2.bias": (D,), "mlp.fc1.weight": (M, D), "mlp.fc1.bias": (M,), "mlp.fc2.weight": (D, M),
                    "mlp.fc2.bias": (D,), "norm1.weight": (D,), "norm1.bias": (D,), "attn.qkv.weight": (3 * D, D), "attn.qkv.bias": (3 * D,),
                    "attn.q.weight": (D, D), "attn.q.bias": (D,), "attn.kv.weight": (2 * D, D), "attn.kv.bias": (2 * D,),
                    "attn.proj.weight": (D, D), "attn.proj.bias": (D,), "attn.sr.weight": (D, D, sr, sr), "attn.sr.bias": (D,),
                    "attn.norm.weight": (D,), "attn.norm.bias": (D,)}
            for j in range(self.depths[k]):
                for key in self.block_keys(k, j):
                    out[key] = tail[key.split(".", 3)[3]]
        for k in range(4):
            out.update(zip(self.peg_keys(k), [(self.dims[k], 1, 3, 3), (self.dims[k],)]))
        return out

    def native_arrays(self, sd, n_stages: int) -> List["torch.Tensor"]:
        """The arrays `i2v_twins_create` takes for the first `n_stages` stages, from a timm-layout state dict, as float32 host tensors.
        Repacked to the gathers' column orders: `patch_embeds.0.proj` flattened as it stands (column (c patch + dy) patch + dx); the later
        embeddings (D, C, 2, 2) -> (D, 4 C) with column (dy + 2 dx) C + c, the 2 x 2 merge gather's order; `attn.sr` (D, D, s, s) ->
        (D, s s D) with column (dy s + dx) D + c, the block gather's order; `pos_block` (D, 1, 3, 3) -> (9, D).  Behind block 0's arrays
        of each stage come its position encoding's filter and bias."""
        f32 = lambda k: sd[k].detach().float().cpu().contiguous()      # noqa: E731
        out = []
        for k in range(n_stages):
            w = f32(f"patch_embeds.{k}.proj.weight")
            out.append(w.reshape(w.shape[0], -1) if k == 0 else w.permute(0, 3, 2, 1).reshape(w.shape[0], -1).contiguous())
            out += [f32(key) for key in self.embed_keys(k)[1:]]
            for j in range(self.depths[k]):
                for key in self.native_block_keys(k, j):
                    t = f32(key)
                    out.append(t.permute(0, 2, 3, 1).reshape(t.shape[0], -1).contiguous() if key.endswith("attn.sr.weight") else t)
                if j == 0:
                    out += [f32(self.peg_keys(k)[0]).reshape(self.dims[k], 9).t().contiguous(), f32(self.peg_keys(k)[1])]
        return out

    def config_lists(self):
        """(dims, heads, MLP widths, depths, sr) as `i2v_twins_config` takes them."""
        return list(self.dims), list(self.heads), [self.mlp(k) for k in range(4)], list(self.depths), list(self.sr_ratios)

    def config_values(self):
        return (self.img, self.in_chans, self.patch, self.stages, self.window, *self.config_lists(), self.ln_eps, self.pe_eps)

    def macs_per_frame(self) -> int:
        total = 0
        for k in range(4):
            T, Tk, D, M, sr = self.tokens(k), self.keys_per_frame(k), self.dims[k], self.mlp(k), self.sr_ratios[k]
            total += T * D * (self.dims[k - 1] * 4 if k else self.in_chans * self.patch ** 2) + 9 * T * D
            for j in range(self.depths[k]):
                if self.is_lsa(k, j):
                    total += T * D * 4 * D + 2 * T * self.window ** 2 * D
                else:
                    total += T * D * 2 * D + Tk * D * 2 * D + 2 * T * Tk * D + (Tk * sr * sr * D * D if sr > 1 else 0)
                total += 2 * T * D * M
        return total

    def workspace_bytes(self, hook_stages: Sequence[int], frames: int, composed: Optional[bool] = None) -> int:
        """Device bytes `i2v_twins_create` plans for these hooked stages and `frames` frames (the formula of csrc/i2v_twins.cpp).
        `composed`: the plan of the shared-launch route of the GSA core (`I2V_TWINS_ATTN=0`; None reads the environment as the planner
        does), which keeps per GSA block the probabilities -- queries x keys rounded up to 4, per head and frame -- and one such array
        of scratch.  Otherwise: the
        weights of the stages run, with one tap-reversed copy of each position-encoding filter; per stage the embedding before its
        LayerNorm with two statistics per token, and its output stream; per block its input, the mid stream, the fc1 pre-activation and
        four statistics per token, and qkv (LSA) or q, kv and -- where sr > 1 -- the sub-sampled plane before its LayerNorm with two
        statistics per key (GSA); the shared scratch -- the patch rows, four streams of the largest stage, one MLP-wide, the attention
        gradient (three streams with windows, one without), four key-side planes -- and the zero table the window launch takes; one
        gradient view per hook."""
        import os
        if composed is None:
            composed = os.environ.get("I2V_TWINS_ATTN") == "0"
        F, ns = frames, max(hook_stages) + 1
        KP = self.in_chans * self.patch ** 2
        weights = acts = m_ftd = m_ftm = m_kv = m_p = 0
        for k in range(ns):
            D, M, sr, T, Tk = self.dims[k], self.mlp(k), self.sr_ratios[k], self.tokens(k), self.keys_per_frame(k)
            weights += D * (4 * self.dims[k - 1] if k else KP) + 3 * D + 2 * 9 * D + D
            acts += F * T * (D + 2) + F * T * D
            for j in range(self.depths[k]):
                weights += 2 * D + D * D + D + 2 * D + 2 * M * D + M + D
                if self.is_lsa(k, j):
                    weights += 3 * D * D + 3 * D
                    acts += 3 * F * T * D
                else:
                    weights += 3 * D * D + 3 * D + (sr * sr * D * D + 3 * D if sr > 1 else 0)
                    acts += F * T * D + 2 * F * Tk * D + (F * Tk * (D + 2) if sr > 1 else 0)
                    if composed:
                        probs = F * T * self.heads[k] * ((Tk + 3) // 4 * 4)
                        acts, m_p = acts + probs, max(m_p, probs)
                acts += F * T * (2 * D + M + 4)
            m_ftd, m_ftm, m_kv = max(m_ftd, F * T * D), max(m_ftm, F * T * M), max(m_kv, 2 * F * Tk * D)
        ni = (2 * self.window - 1) ** 2 * max(self.heads[:ns]) if self.window else 0
        acts += F * self.tokens(0) * KP + (7 if self.window else 5) * m_ftd + m_ftm + 2 * m_kv + ni + m_p
        acts += sum(F * self.hook_dim(s) for s in hook_stages)
        return 4 * (weights + acts)


def is_twins_name(model_name: str) -> bool:
    """A name of timm's Twins vocabulary (`twins.py`), served (`TWINS_MODELS`) or not: `graphs.build` routes these to `twins_named`,
    which refuses the ones that are not offered with a message that lists the served names."""
    return model_name.startswith("twins_")


def twins_named(model_name: str, in_hw=(224, 224)) -> TwinsSpec:
    """Any row of `TWINS_MODELS`, at 224 x 224 only; names outside the table are refused with the reason."""
    served = "; served: " + ", ".join(TWINS_MODELS)
    if model_name not in TWINS_MODELS:
        raise ValueError(f"Twins surrogate {model_name!r}: not a model of this table" + served)
    if tuple(in_hw) != (224, 224):
        raise ValueError(f"{model_name} takes 224 x 224 frames only (got {tuple(in_hw)[0]} x {tuple(in_hw)[1]}): its sub-sampling and "
                         "window-7 stages need the 56 / 28 / 14 / 7 grids" + served)
    dims, heads, ratios, depths, window = TWINS_MODELS[model_name]
    return TwinsSpec(model_name, 224, dims, heads, ratios, depths, window)


def twins_tiny_twin(model_name: str = "twins_pcpvt_small", in_hw=(64, 64)) -> TwinsSpec:
    """The same topology at test size, four stages of two blocks each, so that both block kinds, the position encoding and every sr in
    (8, 4, 2, 1) are real and depths 1..4 hook different stages.  Not rows of `TWINS_MODELS`.
      PCPVT names, square frames of a multiple of 32 pixels: "twins_pcpvt_test" -- at 64 x 64 grids 16 / 8 / 4 / 2, 4 keys; widths 16,
        32, 40, 64 under 1, 2, 5, 8 heads (head widths 16, 16, 8, 8), MLP ratios 4, 4, 2, 2
      PCPVT names at 96 x 96: "twins_pcpvt_test_96" -- grids 24 / 12 / 6 / 3 (an odd last plane), 9 keys (odd, no multiple of 4), 576 /
        144 / 36 / 9 queries; widths 24, 48, 60, 96 under 2, 4, 5, 8 heads of width 12, MLP ratio 2
      SVT names, square frames of a multiple of 128 pixels: "twins_svt_test" -- window 4 and head width 16, Swin's other served window
        shape; at 128 x 128 grids 32 / 16 / 8 / 4, 16 keys; widths 16, 32, 64, 128 under 1, 2, 4, 8 heads, MLP ratio 2
      SVT names at 224 x 224 (the size the attack classes probe a builder with): "twins_svt_test_224" -- window 7 and head width 32 on
        the 56 / 28 / 14 / 7 grids, widths 32, 64, 128, 256, MLP ratio 2"""
    side = int(in_hw[0])
    if in_hw[0] != in_hw[1]:
        raise ValueError(f"the test-size Twins take square frames (got {tuple(in_hw)})")
    if "svt" in model_name:
        if side == 224:
            return TwinsSpec("twins_svt_test_224", 224, (32, 64, 128, 256), (1, 2, 4, 8), (2, 2, 2, 2), (2, 2, 2, 2), 7)
        if side % 128:
            raise ValueError(f"the test-size Twins-SVT takes square frames of a multiple of 128 pixels, or 224 x 224 (got {tuple(in_hw)})")
        return TwinsSpec("twins_svt_test", side, (16, 32, 64, 128), (1, 2, 4, 8), (2, 2, 2, 2), (2, 2, 2, 2), 4)
    if side == 96:
        return TwinsSpec("twins_pcpvt_test_96", 96, (24, 48, 60, 96), (2, 4, 5, 8), (2, 2, 2, 2), (2, 2, 2, 2), 0)
    if side % 32:
        raise ValueError(f"the test-size Twins-PCPVT takes square frames of a multiple of 32 pixels (got {tuple(in_hw)})")
    return TwinsSpec("twins_pcpvt_test", side, (16, 32, 40, 64), (1, 2, 5, 8), (4, 4, 2, 2), (2, 2, 2, 2), 0)


#: Seeded stand-in for a trained Twins, drawn per key as XCiT's is: Linears and the patch and sub-sampling convolutions ~ fan_in^-0.5
#: N(0, 1) (`attn.proj` and `mlp.fc2` at half that), the blocks' LayerNorm gains 1 + 0.1 N(0, 1), biases 0.02 N(0, 1).  What is new
#: shows: `attn.norm` and the patch embeddings' norms have gains uniform on (0.5, 1.5) and shifts 0.1 N(0, 1), so that a sub-sampled
#: plane that skipped its LayerNorm is seen; `attn.sr.bias` is 0.1 N(0, 1); the position encoding's depthwise filter is N(0, 1) / 3
#: with a bias of 0.1 N(0, 1), so that its term is of the size of the stream it is added to.
TWINS_SYNTHETIC = [
    (lambda k: k.endswith("attn.norm.weight") or (k.startswith("patch_embeds") and k.endswith("norm.weight")), uniform(0.5)),
    (lambda k: k.endswith("attn.norm.bias") or (k.startswith("patch_embeds") and k.endswith("norm.bias")) or k.endswith("attn.sr.bias")
     or (k.startswith("pos_block") and k.endswith("bias")), normal(0.1)),
    (starts("pos_block"), normal_over(3.0)),
    *fan_in_tail(ends("norm1.weight", "norm2.weight"))]

TWINS_FAMILY = Family("twins", TwinsSpec, TWINS_MODELS, is_twins_name, twins_named, twins_tiny_twin, "timm's Twins (PCPVT and SVT) at 224 x 224",
                "the last block of stages {}", True, TWINS_SYNTHETIC)


# ---------------------------------------------------------------------------
# the BEiT surrogates: a ViT-shaped stack without a position embedding, whose every block adds a learned relative position bias to its
# attention scores and scales its two branches by LayerScale vectors, planned on the transformer stack (include/i2v_beit.h)
# ---------------------------------------------------------------------------
#: timm 0.5.0's `Beit` models at 224 x 224 (head width 64): name -> (patch, dim, heads, mlp, blocks)
BEIT_MODELS: Dict[str, Tuple[int, int, int, int, int]] = {
    "beit_base_patch16_224": (16, 768, 12, 3072, 12),
    "beit_large_patch16_224": (16, 1024, 16, 4096, 24),
}


@dataclass
class BeitSpec(TokenSpec):
    """timm 0.5.0 `Beit` up to its last block: `patch_embed.proj`, a patch x patch convolution at stride patch
    with bias; one `cls_token` prepended; NO `pos_embed` and no shared `rel_pos_bias`; then `blocks` pre-norm blocks (LayerNorm eps
    `ln_eps`, exact GELU)  x += gamma_1 * proj(attn(norm1 x));  x += gamma_2 * fc2(gelu(fc1(norm2 x))).
    attn: qkv = F.linear(x, qkv.weight, cat(q_bias, 0, v_bias)); q * dh ** -0.5; the scores get
    `relative_position_bias_table[relative_position_index]`, permuted to (heads, T, T), added; softmax over the keys; the product with
    v; proj.  The table has (2 g - 1)^2 + 3 rows for a grid of g a side.
    `hooks`: depth d (1..4) -> zero-based block d * blocks / 4 - 1 (ViT's rule: 2, 5, 8, 11 of 12 blocks; 5, 11, 17, 23 of 24), whose
    OUTPUT (the residual stream after it, all tokens, the class token included) is the hooked feature: tokens * dim floats per frame.
    `norm` / `fc_norm` and `head` lie behind every hook."""
    arch: str
    img: int
    patch: int = 16
    in_chans: int = 3
    dim: int = 768
    heads: int = 12
    mlp: int = 3072
    blocks: int = 12
    ln_eps: float = 1e-6
    hooks: Dict[int, int] = field(default_factory=dict)
    video: bool = False

    def __post_init__(self):
        dh = self.dim // self.heads
        if self.img % self.patch or self.tokens > 208:
            raise ValueError(f"{self.arch}: a {self.img} x {self.img} frame under patch {self.patch} must be whole patches and at most "
                             "208 tokens with the class token")
        if self.dim % self.heads or dh % 4 or dh > 64:
            raise ValueError(f"{self.arch}: width {self.dim} under {self.heads} heads: the head width must be a multiple of 4 up to 64")
        if self.blocks % 4:
            raise ValueError(f"{self.arch}: {self.blocks} blocks: the hooks sit at every quarter of the stack")
        if not self.hooks:
            self.hooks = self.quarter_hooks()

    @property
    def grid(self) -> int:
        return self.img // self.patch

    @property
    def tokens(self) -> int:
        return 1 + self.grid ** 2

    @property
    def table_rows(self) -> int:
        return (2 * self.grid - 1) ** 2 + 3

    @property
    def hook_dim(self) -> int:
        """Floats per frame of a hooked feature."""
        return self.tokens * self.dim

    def block_keys(self, i: int) -> List[str]:
        """The block's PARAMETERS in timm's state-dict order (the buffer `attn.relative_position_index` sits behind the table there:
        `index_key`)."""
        p = f"blocks.{i}."
        return [p + k for k in ("gamma_1", "gamma_2", "norm1.weight", "norm1.bias", "attn.q_bias", "attn.v_bias",
                                "attn.relative_position_bias_table", "attn.qkv.weight", "attn.proj.weight", "attn.proj.bias", "norm2.weight",
                                "norm2.bias", "mlp.fc1.weight", "mlp.fc1.bias", "mlp.fc2.weight", "mlp.fc2.bias")]

    def index_key(self, i: int) -> str:
        return f"blocks.{i}.attn.relative_position_index"

    def param_shapes(self) -> Dict[str, Tuple[int, ...]]:
        """timm `state_dict` key -> shape for every parameter up to the last block, in timm's order.  The int64 buffers
        `attn.relative_position_index` (tokens, tokens) are not parameters: they are computed (`relative_position_index`), never loaded."""
        D, M = self.dim, self.mlp
        out = {"cls_token": (1, 1, D), "patch_embed.proj.weight": (D, self.in_chans, self.patch, self.patch), "patch_embed.proj.bias": (D,)}
        shapes = [(D,), (D,), (D,), (D,), (D,), (D,), (self.table_rows, self.heads), (3 * D, D), (D, D), (D,), (D,), (D,), (M, D), (M,),
                  (D, M), (D,)]
        for i in range(self.blocks):
            out.update(zip(self.block_keys(i), shapes))
        return out

    def relative_position_index(self) -> "torch.Tensor":
        """The (tokens, tokens) int64 index into a block's bias table, as `beit.py` defines it, from coordinate differences: the pair of
        patches (yi, xi), (yj, xj) -> (yi - yj + g - 1) (2 g - 1) + (xi - xj + g - 1); the class token's row -> n - 3, its column ->
        n - 2, its own element -> n - 1, for a table of n rows."""
        import torch
        g, n = self.grid, self.table_rows
        y = torch.arange(g).repeat_interleave(g)
        x = torch.arange(g).repeat(g)
        idx = torch.empty(self.tokens, self.tokens, dtype=torch.int64)
        idx[1:, 1:] = (y[:, None] - y[None, :] + g - 1) * (2 * g - 1) + (x[:, None] - x[None, :] + g - 1)
        idx[0, :] = n - 3
        idx[:, 0] = n - 2
        idx[0, 0] = n - 1
        return idx

    def native_arrays(self, sd, n_blocks: int) -> List["torch.Tensor"]:
        """The arrays `i2v_beit_create` takes for the first `n_blocks` blocks, from a timm-layout state dict, as float32 host tensors:
        the patch weight flattened as it stands, its bias, `cls_token` as (dim); per block 13 arrays -- the qkv bias built as
        [q_bias | 0 | v_bias], the table expanded through the index to a dense (heads, T, T) array, `gamma_1` folded into `attn.proj`
        and `gamma_2` into `mlp.fc2` (weight rows and bias; products in float64, rounded once)."""
        import torch
        f32 = lambda k: sd[k].detach().float().cpu().contiguous()      # noqa: E731
        f64 = lambda k: sd[k].detach().double().cpu()                  # noqa: E731
        T, idx = self.tokens, self.relative_position_index().reshape(-1)
        out = [f32("patch_embed.proj.weight").reshape(self.dim, -1), f32("patch_embed.proj.bias"), f32("cls_token").reshape(self.dim)]
        for i in range(n_blocks):
            p = f"blocks.{i}."
            g1, g2 = f64(p + "gamma_1"), f64(p + "gamma_2")
            dense = f32(p + "attn.relative_position_bias_table")[idx].reshape(T, T, self.heads).permute(2, 0, 1).contiguous()
            out += [f32(p + "norm1.weight"), f32(p + "norm1.bias"), f32(p + "attn.qkv.weight"),
                    torch.cat([f32(p + "attn.q_bias"), torch.zeros(self.dim), f32(p + "attn.v_bias")]), dense,
                    (g1[:, None] * f64(p + "attn.proj.weight")).float().contiguous(), (g1 * f64(p + "attn.proj.bias")).float().contiguous(),
                    f32(p + "norm2.weight"), f32(p + "norm2.bias"), f32(p + "mlp.fc1.weight"), f32(p + "mlp.fc1.bias"),
                    (g2[:, None] * f64(p + "mlp.fc2.weight")).float().contiguous(), (g2 * f64(p + "mlp.fc2.bias")).float().contiguous()]
        return out

    def config_values(self):
        return (self.img, self.patch, self.in_chans, self.dim, self.heads, self.mlp, self.blocks, self.ln_eps)

    def macs_per_frame(self) -> int:
        T, D, M = self.tokens, self.dim, self.mlp
        per_block = T * D * (3 * D + D + 2 * M) + 2 * T * T * D
        return (T - 1) * D * self.in_chans * self.patch ** 2 + self.blocks * per_block

    def workspace_bytes(self, hook_blocks: Sequence[int], frames: int, composed: Optional[bool] = None) -> int:
        """Device bytes `i2v_beit_create` plans for these hooks and `frames` frames (the formula of csrc/i2v_beit.cpp): the weights of
        the blocks run, the dense bias of each among them; per block its input, qkv, the mid stream, the fc1 pre-activation and four
        statistics per token; the shared scratch -- the top stream, two streams, one MLP-wide, the qkv gradient, the patch rows and
        their embedding, and the table of zeros the assemble launch takes --; one gradient view per hook.  `composed`: the plan of the
        shared-launch route of the attention core (`I2V_BEIT_ATTN=0`; None reads the environment as the planner does), which keeps per
        block the probabilities -- tokens x tokens rounded up to 4, per head and frame -- and the bias padded to that row stride, and
        one array of scratch the size of a block's probabilities."""
        import os
        if composed is None:
            composed = os.environ.get("I2V_BEIT_ATTN") == "0"
        D, M, T, H, F, nb = self.dim, self.mlp, self.tokens, self.heads, frames, max(hook_blocks) + 1
        KP, NP, FT, ld = self.in_chans * self.patch ** 2, T - 1, frames * T, (T + 3) // 4 * 4
        probs, padded = (F * H * T * ld, H * T * ld) if composed else (0, 0)
        weights = D * KP + 2 * D + nb * (4 * D * D + 2 * D * M + 9 * D + M + H * T * T)
        per_block = 5 * FT * D + FT * M + 4 * FT + probs + padded
        shared = 6 * FT * D + FT * M + F * NP * (KP + D) + T * D + probs
        return 4 * (weights + nb * per_block + shared + len(hook_blocks) * FT * D)


def is_beit_name(model_name: str) -> bool:
    """A name of timm's BEiT vocabulary (`beit.py`), served (`BEIT_MODELS`) or not: `graphs.build` routes these to `beit_named`, which
    refuses the ones that are not offered with a message that lists the served names."""
    return model_name.startswith("beit_")


def beit_named(model_name: str, in_hw=(224, 224)) -> BeitSpec:
    """Any row of `BEIT_MODELS`, at 224 x 224 only.  Refused, each with the reason: the 384 x 384 and 512 x 512 checkpoints (other
    bias-table sizes), the `_in22k` names (ViT's rule for `in21k`), names outside the table, and every other input size."""
    served = "; served: " + ", ".join(BEIT_MODELS)
    if model_name not in BEIT_MODELS:
        if "384" in model_name or "512" in model_name:
            why = "the 384 x 384 and 512 x 512 checkpoints carry bias tables of other sizes and are not offered (224 x 224 only)"
        elif "in22k" in model_name:
            why = "the in22k checkpoints (21841-class heads) are not offered"
        else:
            why = "not a model of this table"
        raise ValueError(f"BEiT surrogate {model_name!r}: {why}" + served)
    if tuple(in_hw) != (224, 224):
        raise ValueError(f"{model_name} takes 224 x 224 frames only (got {tuple(in_hw)[0]} x {tuple(in_hw)[1]}): its relative position "
                         "bias tables are those of the 14 x 14 grid" + served)
    patch, dim, heads, mlp, blocks = BEIT_MODELS[model_name]
    return BeitSpec(model_name, 224, patch, 3, dim, heads, mlp, blocks)


def beit_tiny_twin(model_name: str = "beit_base_patch16_224", in_hw=(64, 64)) -> BeitSpec:
    """The same topology at test size, by frame size (every served name maps to the same twins).  Not rows of `BEIT_MODELS`.
      64 x 64: "beit_test" -- grid 4, 17 tokens, a table of 52 rows; dim 64 under 2 heads of width 32, MLP 256, 8 blocks, so that depths
        1..4 hook blocks 1, 3, 5, 7
      96 x 96: "beit_test_96" -- grid 6, 37 tokens (a multiple of neither 4 nor 16), 124 table rows; dim 48 under 4 heads of width 12 (no
        multiple of 16), MLP 96, 8 blocks
      224 x 224 (the size the attack classes probe a builder with): "beit_test_224" -- 197 tokens, dim 64 under 1 head of width 64, MLP
        128, 4 blocks"""
    if in_hw[0] != in_hw[1] or int(in_hw[0]) not in (64, 96, 224):
        raise ValueError(f"the test-size BEiTs take 64 x 64, 96 x 96 or 224 x 224 frames (got {tuple(in_hw)})")
    side = int(in_hw[0])
    if side == 64:
        return BeitSpec("beit_test", 64, 16, 3, 64, 2, 256, 8)
    if side == 96:
        return BeitSpec("beit_test_96", 96, 16, 3, 48, 4, 96, 8)
    return BeitSpec("beit_test_224", 224, 16, 3, 64, 1, 128, 4)


def check_beit_buffers(spec: BeitSpec, sd, where: str) -> None:
    """timm's BEiT checkpoints carry the buffer `attn.relative_position_index` per block; it is computed from the geometry here and
    never loaded, so one that differs describes another model: refused by key name.  An absent one is fine."""
    import torch
    idx = spec.relative_position_index()
    for i in range(spec.blocks):
        k = spec.index_key(i)
        if k in sd and not (tuple(sd[k].shape) == tuple(idx.shape) and torch.equal(sd[k].long(), idx)):
            raise ValueError(f"{where}: buffer {k} differs from the index computed for a {spec.grid} x {spec.grid} grid")


#: Seeded stand-in for a trained BEiT, drawn per key as Twins' is: Linears and the patch convolution ~ fan_in^-0.5 N(0, 1) (`attn.proj`
#: and `mlp.fc2` at half that), LayerNorm gains 1 + 0.1 N(0, 1), biases 0.02 N(0, 1), `cls_token` 0.02 N(0, 1).  timm's initial values
#: would blind the tests -- a zero bias table makes the bias a no-op, a LayerScale of 0.1 or 1e-5 silences the blocks -- so what is new
#: shows: `relative_position_bias_table` is N(0, 1), `gamma_1` / `gamma_2` are uniform on (0.5, 1.5), and `q_bias` / `v_bias` are 0.1
#: N(0, 1).  The index buffers are not emitted: they are computed from the geometry.
BEIT_SYNTHETIC = [(ends("gamma_1", "gamma_2"), uniform(0.5)), (ends("relative_position_bias_table"), normal()),
                  (ends("q_bias", "v_bias"), normal(0.1)),
                  *fan_in_tail(ends("norm1.weight", "norm2.weight"), bias=lambda k: k.endswith("bias") or k == "cls_token")]

BEIT_FAMILY = Family("beit", BeitSpec, BEIT_MODELS, is_beit_name, beit_named, beit_tiny_twin, "timm's BEiTs at 224 x 224 with patch 16",
                "blocks {}", True, BEIT_SYNTHETIC, check_beit_buffers)


# ---------------------------------------------------------------------------
# the PiT surrogates: a ViT whose token grid is pooled between three stages like a CNN's, with an overlapping patch embedding and a
# spatial position table, planned on the transformer stack (include/i2v_pit.h)
# ---------------------------------------------------------------------------
#: timm 0.5.0's `PoolingVisionTransformer` models at 224 x 224: name -> (patch, stride, base dim, heads per stage, depth per stage);
#: every name has a `_distilled_224` twin with two prefix tokens (`pit_named`)
PIT_MODELS: Dict[str, Tuple[int, int, int, Tuple[int, int, int], Tuple[int, int, int]]] = {
    "pit_ti_224": (16, 8, 32, (2, 4, 8), (2, 6, 4)),
    "pit_xs_224": (16, 8, 48, (2, 4, 8), (2, 6, 4)),
    "pit_s_224": (16, 8, 48, (3, 6, 12), (2, 6, 4)),
    "pit_b_224": (14, 7, 64, (4, 8, 16), (3, 6, 4)),
}
PIT_MODELS.update({k.replace("_224", "_distilled_224"): v for k, v in list(PIT_MODELS.items())})


@dataclass
class PitSpec(TokenSpec):
    """timm 0.5.0 `PoolingVisionTransformer` up to its last block (restated, UNCHECKED against timm):
    `patch_embed.conv`, a patch x patch convolution at stride `stride` < patch, padding 0, with bias, onto a grid of
    (img - patch) / stride + 1 a side; `pos_embed` (1, C, g, g) added to the grid tokens only; `cls_token` (1, prefix, C) prepended
    (prefix = 2 for a distilled net); three stages `transformers.{s}` of pre-norm ViT blocks (LayerNorm eps `ln_eps`, exact GELU, MLP
    ratio 4, qkv bias, head width = base dim); behind stages 0 and 1 `transformers.{s}.pool`: `pool.conv`, a Conv2d(C, 2 C, 3, stride 2,
    padding 1, groups = C) on the grid tokens (grid -> (g - 1) / 2 + 1), and `pool.fc`, a Linear(C, 2 C) on the prefix tokens.
    `hooks`: depth d (1..4) -> zero-based FLAT block index whose OUTPUT (the residual stream after it, all tokens, the prefix tokens
    included, before any pooling) is the hooked feature: the last block of stage 0, block depth[1] / 2 - 1 of stage 1, the last block of
    stage 1, the last block of stage 2.  `norm`, `head` and `head_dist` lie behind every hook."""
    arch: str
    img: int
    patch: int = 16
    stride: int = 8
    base_dim: int = 48
    heads: Tuple[int, int, int] = (3, 6, 12)
    depths: Tuple[int, int, int] = (2, 6, 4)
    prefix: int = 1
    in_chans: int = 3
    ln_eps: float = 1e-6
    hooks: Dict[int, int] = field(default_factory=dict)
    video: bool = False

    def __post_init__(self):
        if self.patch > self.img or (self.img - self.patch) % self.stride or self.stride > self.patch:
            raise ValueError(f"{self.arch}: patches of {self.patch} at stride {self.stride} do not tile a {self.img} x {self.img} frame")
        if self.base_dim % 4 or self.base_dim > 64 or self.prefix not in (1, 2) or len(self.heads) != 3 or len(self.depths) != 3:
            raise ValueError(f"{self.arch}: head width {self.base_dim} (a multiple of 4 up to 64), {self.prefix} prefix tokens (1 or 2), three stages")
        if not self.hooks:
            d = self.depths
            self.hooks = {1: d[0] - 1, 2: d[0] + d[1] // 2 - 1, 3: d[0] + d[1] - 1, 4: d[0] + d[1] + d[2] - 1}

    @property
    def grids(self) -> Tuple[int, int, int]:
        g0 = (self.img - self.patch) // self.stride + 1
        g1 = (g0 - 1) // 2 + 1
        return (g0, g1, (g1 - 1) // 2 + 1)

    @property
    def widths(self) -> Tuple[int, int, int]:
        return tuple(self.base_dim * h for h in self.heads)

    @property
    def blocks(self) -> int:
        return sum(self.depths)

    def stage_of(self, block: int) -> int:
        """The stage of a flat block index."""
        d = self.depths
        return 0 if block < d[0] else 1 if block < d[0] + d[1] else 2

    def tokens(self, stage: int) -> int:
        return self.prefix + self.grids[stage] ** 2

    def hook_shape(self, block: int) -> Tuple[int, int]:
        st = self.stage_of(block)
        return (self.tokens(st), self.widths[st])

    def block_key(self, block: int) -> str:
        """timm's prefix of a flat block index: `transformers.{s}.blocks.{j}.`"""
        st = self.stage_of(block)
        return f"transformers.{st}.blocks.{block - sum(self.depths[:st])}."

    def param_shapes(self) -> Dict[str, Tuple[int, ...]]:
        """timm `state_dict` key -> shape for every parameter up to the last block, in timm's order."""
        g0, W = self.grids[0], self.widths
        out = {"pos_embed": (1, W[0], g0, g0), "cls_token": (1, self.prefix, W[0]),
               "patch_embed.conv.weight": (W[0], self.in_chans, self.patch, self.patch), "patch_embed.conv.bias": (W[0],)}
        b = 0
        for st in range(3):
            D = W[st]
            for _ in range(self.depths[st]):
                p = self.block_key(b)
                out.update({p + "norm1.weight": (D,), p + "norm1.bias": (D,), p + "attn.qkv.weight": (3 * D, D), p + "attn.qkv.bias": (3 * D,),
                            p + "attn.proj.weight": (D, D), p + "attn.proj.bias": (D,), p + "norm2.weight": (D,), p + "norm2.bias": (D,),
                            p + "mlp.fc1.weight": (4 * D, D), p + "mlp.fc1.bias": (4 * D,), p + "mlp.fc2.weight": (D, 4 * D),
                            p + "mlp.fc2.bias": (D,)})
                b += 1
            if st < 2:
                p = f"transformers.{st}.pool."
                out.update({p + "conv.weight": (2 * D, 1, 3, 3), p + "conv.bias": (2 * D,), p + "fc.weight": (2 * D, D), p + "fc.bias": (2 * D,)})
        return out

    def native_arrays(self, sd, n_blocks: int) -> List["torch.Tensor"]:
        """The arrays `i2v_pit_create` takes for the first `n_blocks` flat blocks, from a timm-layout state dict, as float32 host
        tensors: the patch weight flattened as it stands, its bias, `pos_embed` transposed to token-major with `prefix` rows of zeros in
        front, `cls_token` as (prefix, C); per block its 12 arrays; behind a stage whose successor runs a block, its pool's 4 arrays
        (the filter as (2 C, 9))."""
        import torch
        f32 = lambda k: sd[k].detach().float().cpu().contiguous()      # noqa: E731
        W, g0 = self.widths, self.grids[0]
        pos = f32("pos_embed").reshape(W[0], g0 * g0).t()
        out = [f32("patch_embed.conv.weight").reshape(W[0], -1), f32("patch_embed.conv.bias"),
               torch.cat([torch.zeros(self.prefix, W[0]), pos]).contiguous(), f32("cls_token").reshape(self.prefix, W[0])]
        for b in range(n_blocks):
            st, p = self.stage_of(b), self.block_key(b)
            if b and st != self.stage_of(b - 1):
                q = f"transformers.{st - 1}.pool."
                out += [f32(q + "conv.weight").reshape(W[st], 9), f32(q + "conv.bias"), f32(q + "fc.weight"), f32(q + "fc.bias")]
            out += [f32(p + k) for k in ("norm1.weight", "norm1.bias", "attn.qkv.weight", "attn.qkv.bias", "attn.proj.weight", "attn.proj.bias",
                                         "norm2.weight", "norm2.bias", "mlp.fc1.weight", "mlp.fc1.bias", "mlp.fc2.weight", "mlp.fc2.bias")]
        return out

    def config_values(self):
        return (self.img, self.patch, self.stride, self.in_chans, self.prefix, self.widths, self.heads, self.depths, self.ln_eps)

    def macs_per_frame(self) -> int:
        total = self.grids[0] ** 2 * self.widths[0] * self.in_chans * self.patch ** 2
        for st in range(3):
            T, D = self.tokens(st), self.widths[st]
            total += self.depths[st] * (T * D * 12 * D + 2 * T * T * D)
        return total

    def workspace_bytes(self, hook_blocks: Sequence[int], frames: int, composed: Optional[bool] = None) -> int:
        """Device bytes `i2v_pit_create` plans for these hooks and `frames` frames (the formula of csrc/i2v_pit.cpp): the weights of the
        blocks run and of the pools between the stages run; per block its input, qkv, the mid stream, the fc1 pre-activation, four
        statistics per token, and the attention output with its log-sum-exp; per stage the stream behind it; the shared scratch -- three
        streams, one MLP-wide, the qkv gradient (all at the widest stage's size), the patch rows and their embedding, delta --; one
        gradient view per hook.  `composed`: the plan of the shared-launch route (`I2V_PIT_ATTN=0`; None reads the environment as the
        planner does), which keeps per block the probabilities -- tokens x tokens rounded up to 4, per head and frame -- instead of the
        output and the log-sum-exp, and one array of scratch the size of the largest block's probabilities instead of delta."""
        import os
        if composed is None:
            composed = os.environ.get("I2V_PIT_ATTN") == "0"
        F, nb, W = frames, max(hook_blocks) + 1, self.widths
        KP, NP = self.in_chans * self.patch ** 2, self.grids[0] ** 2
        total = W[0] * KP + W[0] + (self.prefix + NP) * W[0] + self.prefix * W[0]
        mFTD = mStat = mP = first = 0
        for st in range(3):
            if first >= nb:
                break
            D, T, H = W[st], self.tokens(st), self.heads[st]
            count, FT = min(self.depths[st], nb - first), F * T
            probs = F * H * T * ((T + 3) // 4 * 4) if composed else 0
            core = probs if composed else FT * D + F * H * T
            total += count * (12 * D * D + 13 * D + 9 * FT * D + 4 * FT + core) + FT * D
            first += self.depths[st]
            if first < nb:
                total += 2 * D * 9 + 2 * D + 2 * D * D + 2 * D
            mFTD, mStat, mP = max(mFTD, FT * D), max(mStat, F * H * T), max(mP, probs)
        total += 10 * mFTD + F * NP * (KP + W[0]) + (mP if composed else mStat)
        total += sum(F * self.hook_shape(b)[0] * self.hook_shape(b)[1] for b in hook_blocks)
        return 4 * total


def is_pit_name(model_name: str) -> bool:
    """A name of timm's PiT vocabulary (`pit.py`), served (`PIT_MODELS`) or not: `graphs.build_surrogate` routes these to `pit_named`, which
    refuses the ones that are not offered with a message that lists the served names."""
    return model_name.startswith("pit_")


def pit_named(model_name: str, in_hw=(224, 224)) -> PitSpec:
    """Any row of `PIT_MODELS`, at 224 x 224 only.  Refused, each with the reason: names outside the table and every other input size."""
    served = "; served: " + ", ".join(PIT_MODELS)
    if model_name not in PIT_MODELS:
        raise ValueError(f"PiT surrogate {model_name!r}: not a model of this table (224 x 224 checkpoints only)" + served)
    if tuple(in_hw) != (224, 224):
        raise ValueError(f"{model_name} takes 224 x 224 frames only (got {tuple(in_hw)[0]} x {tuple(in_hw)[1]}): its position table is "
                         "that of its own grid" + served)
    patch, stride, base, heads, depths = PIT_MODELS[model_name]
    return PitSpec(model_name, 224, patch, stride, base, heads, depths, 2 if "_distilled_" in model_name else 1)


def pit_tiny_twin(model_name: str = "pit_s_224", in_hw=(64, 64)) -> PitSpec:
    """The same topology at test size, by frame size (every served name maps to the same twins).  Not rows of `PIT_MODELS`.
      64 x 64: "pit_test" -- patch 16 / stride 8, grids 7 -> 4 -> 2, one prefix token, base dim 16, heads 2 / 4 / 8, depths 2 / 2 / 2
      70 x 70: "pit_test_70" -- patch 14 / stride 7, grids 9 -> 5 -> 3, TWO prefix tokens, base dim 12 (ragged against the MFMA's chunk
        of 16), heads 2 / 4 / 8, depths 3 / 2 / 2
      224 x 224 (the size the attack classes probe a builder with): "pit_test_224" -- 730 tokens in stage 0, base dim 32, heads
        1 / 2 / 4, depths 1 / 2 / 1"""
    if in_hw[0] != in_hw[1] or int(in_hw[0]) not in (64, 70, 224):
        raise ValueError(f"the test-size PiTs take 64 x 64, 70 x 70 or 224 x 224 frames (got {tuple(in_hw)})")
    side = int(in_hw[0])
    if side == 64:
        return PitSpec("pit_test", 64, 16, 8, 16, (2, 4, 8), (2, 2, 2), 1)
    if side == 70:
        return PitSpec("pit_test_70", 70, 14, 7, 12, (2, 4, 8), (3, 2, 2), 2)
    return PitSpec("pit_test_224", 224, 16, 8, 32, (1, 2, 4), (1, 2, 1), 1)


#: Seeded stand-in for a trained PiT, drawn per key as BEiT's is: Linears and the patch convolution ~ fan_in^-0.5 N(0, 1) (`attn.proj`
#: and `mlp.fc2` at half that), LayerNorm gains 1 + 0.1 N(0, 1), biases 0.02 N(0, 1).  What is new must show in the tests: `pos_embed`
#: and `cls_token` are N(0, 1) (timm's 0.02 would leave the position table and the prefix tokens below the tests' bounds), and the pool
#: filter `pool.conv.weight` is N(0, 1) / 3 over its 9 taps, so that a pooled token is of the size of its inputs.
PIT_SYNTHETIC = [(keys("pos_embed", "cls_token"), normal()), (ends("pool.conv.weight"), normal_over(3.0)),
                 *fan_in_tail(ends("norm1.weight", "norm2.weight"))]

PIT_FAMILY = Family("pit", PitSpec, PIT_MODELS, is_pit_name, pit_named, pit_tiny_twin, "timm's PiTs at 224 x 224",
                "blocks {}, numbered across the stages", False, PIT_SYNTHETIC)


# ---------------------------------------------------------------------------
# the CoaT-Lite surrogates: four stages of serial blocks whose attention is FACTORIZED -- a softmax down the token axis of K, a dh x dh
# product per head -- with a convolutional position encoding, planned on the transformer stack (include/i2v_coat.h)
# ---------------------------------------------------------------------------
#: timm 0.5.0's serial `CoaT` models at 224 x 224: name -> (width per stage, depth per stage, MLP ratio per stage); 8 heads, crpe
#: windows 3 / 5 / 7 on 2 / 3 / 3 heads
COAT_MODELS: Dict[str, Tuple[Tuple[int, int, int, int], Tuple[int, int, int, int], Tuple[int, int, int, int]]] = {
    "coat_lite_tiny": ((64, 128, 256, 320), (2, 2, 2, 2), (8, 8, 4, 4)),
    "coat_lite_mini": ((64, 128, 320, 512), (2, 2, 2, 2), (8, 8, 4, 4)),
    "coat_lite_small": ((64, 128, 320, 512), (3, 4, 6, 3), (8, 8, 4, 4)),
}
#: timm's CoaT names with parallel blocks: refused with that reason
COAT_PARALLEL = ("coat_tiny", "coat_mini")


@dataclass
class CoatSpec(StagedSpec):
    """timm 0.5.0 `CoaT` with serial blocks only, up to its last block (restated from memory of coat.py, UNCHECKED
    against timm): `patch_embed1`, a Conv2d(3, C, 4, stride 4) and a LayerNorm; `patch_embed{2,3,4}`, a Conv2d(C', C, 2, stride 2) and
    a LayerNorm on the previous stage's grid tokens, the class token dropped; `cls_token{k}` (1, 1, C) in front of every stage, no
    position table; `serial_blocks{k}.{j}`: x = cpe(x); x = x + proj(FA(LN1 x)); x = x + fc2(gelu(fc1(LN2 x))) with LayerNorm eps
    `ln_eps`, a qkv bias and the exact GELU.  `cpe{k}.proj` is a depthwise 3 x 3 with a residual on the grid tokens.  FA takes the
    softmax of k over the TOKENS per channel, G = softmax(k)^T v per head, out = dh^-0.5 q G + q o E, E = `crpe{k}` of v as an image (0 on
    the class row): `conv_list.0 / 1 / 2`, depthwise 3 x 3 / 5 x 5 / 7 x 7 on the first `windows[0]`, the next `windows[1]` and the last
    `windows[2]` heads.  `hooks`: depth d (1..4) -> zero-based stage whose output (the residual stream after its last block, all tokens
    with the class token, before the next patch embedding) is the hooked feature.  `norm*`, `head` and `aggregate` lie behind every hook."""
    arch: str
    img: int
    widths: Tuple[int, int, int, int] = (64, 128, 256, 320)
    depths: Tuple[int, int, int, int] = (2, 2, 2, 2)
    mlp_ratios: Tuple[int, int, int, int] = (8, 8, 4, 4)
    heads: int = 8
    windows: Tuple[int, int, int] = (2, 3, 3)
    in_chans: int = 3
    ln_eps: float = 1e-6
    hooks: Dict[int, int] = field(default_factory=dict)
    video: bool = False

    def __post_init__(self):
        if self.img % 32:
            raise ValueError(f"{self.arch}: a {self.img} x {self.img} frame is not tiled by the 4 x 4 patches and three 2 x 2 embeddings")
        if sum(self.windows) != self.heads or min(self.windows) < 1 or any(w % self.heads or (w // self.heads) % 4 or w // self.heads > 64
                                                                            for w in self.widths):
            raise ValueError(f"{self.arch}: widths {self.widths} over {self.heads} heads (head widths: multiples of 4 up to 64), "
                             f"windows {self.windows} (positive, summing to the heads)")
        if not self.hooks:
            self.hooks = {1: 0, 2: 1, 3: 2, 4: 3}

    stages = 4

    @property
    def grids(self) -> Tuple[int, int, int, int]:
        return tuple(self.img // 4 // 2 ** k for k in range(4))

    @property
    def head_widths(self) -> Tuple[int, int, int, int]:
        return tuple(w // self.heads for w in self.widths)

    def tokens(self, stage: int) -> int:
        return 1 + self.grids[stage] ** 2

    def width(self, stage: int) -> int:
        return self.widths[stage]

    def window_channels(self, stage: int) -> Tuple[int, int, int]:
        """Channels of stage `stage` that pass crpe's 3 x 3, 5 x 5 and 7 x 7."""
        return tuple(w * self.head_widths[stage] for w in self.windows)

    def param_shapes(self) -> Dict[str, Tuple[int, ...]]:
        """timm `state_dict` key -> shape for every parameter up to the last block, the shared cpe / crpe under their stage-level keys."""
        out = {}
        for k in range(4):
            D, Cin, p, s = self.widths[k], self.widths[k - 1] if k else self.in_chans, 2 if k else 4, k + 1
            out.update({f"patch_embed{s}.proj.weight": (D, Cin, p, p), f"patch_embed{s}.proj.bias": (D,), f"patch_embed{s}.norm.weight": (D,),
                        f"patch_embed{s}.norm.bias": (D,), f"cls_token{s}": (1, 1, D), f"cpe{s}.proj.weight": (D, 1, 3, 3),
                        f"cpe{s}.proj.bias": (D,)})
            for i, (K, n) in enumerate(zip((3, 5, 7), self.window_channels(k))):
                out.update({f"crpe{s}.conv_list.{i}.weight": (n, 1, K, K), f"crpe{s}.conv_list.{i}.bias": (n,)})
            M = self.mlp_ratios[k] * D
            for j in range(self.depths[k]):
                q = f"serial_blocks{s}.{j}."
                out.update({q + "norm1.weight": (D,), q + "norm1.bias": (D,), q + "factoratt_crpe.qkv.weight": (3 * D, D),
                            q + "factoratt_crpe.qkv.bias": (3 * D,), q + "factoratt_crpe.proj.weight": (D, D), q + "factoratt_crpe.proj.bias": (D,),
                            q + "norm2.weight": (D,), q + "norm2.bias": (D,), q + "mlp.fc1.weight": (M, D), q + "mlp.fc1.bias": (M,),
                            q + "mlp.fc2.weight": (D, M), q + "mlp.fc2.bias": (D,)})
        return out

    def shared_duplicates(self) -> Dict[str, str]:
        """The keys under which a timm checkpoint carries the shared modules AGAIN inside every block -> their stage-level key."""
        out = {}
        for k in range(4):
            s = k + 1
            for j in range(self.depths[k]):
                q = f"serial_blocks{s}.{j}."
                for t in ("weight", "bias"):
                    out[q + f"cpe.proj.{t}"] = f"cpe{s}.proj.{t}"
                    for i in range(3):
                        out[q + f"factoratt_crpe.crpe.conv_list.{i}.{t}"] = f"crpe{s}.conv_list.{i}.{t}"
        return out

    def native_arrays(self, sd, n_stages: int) -> List["torch.Tensor"]:
        """The arrays `i2v_coat_create` takes for the first `n_stages` stages, from a timm-layout state dict, as float32 host tensors.
        Per stage 12: the patch weight as a Linear (stage 0 flattened as it stands, later stages with column (dy 2 + dx) C' + c, the cell
        gather's order), its bias, the LayerNorm pair, `cls_token` as (C), a table of zeros (1 + g^2, C), `cpe.proj.weight` tap-major as
        (9, C), its bias, crpe's filters tap-major as (9, n3), (25, n5), (49, n7) and its biases concatenated; then 12 per block."""
        import torch
        f32 = lambda k: sd[k].detach().float().cpu().contiguous()      # noqa: E731
        out = []
        for k in range(n_stages):
            D, s = self.widths[k], k + 1
            w = f32(f"patch_embed{s}.proj.weight")
            out += [(w.permute(0, 2, 3, 1) if k else w).reshape(D, -1).contiguous(), f32(f"patch_embed{s}.proj.bias"),
                    f32(f"patch_embed{s}.norm.weight"), f32(f"patch_embed{s}.norm.bias"), f32(f"cls_token{s}").reshape(D),
                    torch.zeros(self.tokens(k), D), f32(f"cpe{s}.proj.weight").reshape(D, 9).t().contiguous(), f32(f"cpe{s}.proj.bias")]
            out += [f32(f"crpe{s}.conv_list.{i}.weight").reshape(-1, K * K).t().contiguous() for i, K in enumerate((3, 5, 7))]
            out += [torch.cat([f32(f"crpe{s}.conv_list.{i}.bias") for i in range(3)]).contiguous()]
            for j in range(self.depths[k]):
                q = f"serial_blocks{s}.{j}."
                out += [f32(q + t) for t in ("norm1.weight", "norm1.bias", "factoratt_crpe.qkv.weight", "factoratt_crpe.qkv.bias",
                                             "factoratt_crpe.proj.weight", "factoratt_crpe.proj.bias", "norm2.weight", "norm2.bias",
                                             "mlp.fc1.weight", "mlp.fc1.bias", "mlp.fc2.weight", "mlp.fc2.bias")]
        return out

    def config_values(self):
        return (self.img, self.in_chans, self.widths, self.heads, self.depths, self.mlp_ratios, *self.windows, self.ln_eps)

    def macs_per_frame(self) -> int:
        total = 0
        for k in range(4):
            T, D, np_, dh = self.tokens(k), self.widths[k], self.grids[k] ** 2, self.head_widths[k]
            total += np_ * D * (4 * self.widths[k - 1] if k else 16 * self.in_chans)
            total += self.depths[k] * (T * D * (4 * D + 2 * self.mlp_ratios[k] * D) + 2 * T * D * dh + np_ * D * (9 + 30))
        return total

    def workspace_bytes(self, hook_stages: Sequence[int], frames: int) -> int:
        """Device bytes `i2v_coat_create` plans for these hooks and `frames` frames (the formula of csrc/i2v_coat.cpp): per stage run its
        12 arrays, the embedding before its LayerNorm with two statistics per grid token and the stream behind it; per block its 12 arrays,
        its input, qkv, the mid stream, the fc1 pre-activation, four statistics per token, E, G (frames, heads, dh, dh) and the column
        statistics (frames, heads, 2, dh); the shared scratch -- five streams and the qkv gradient at the widest stage's size, one
        MLP-wide, the patch rows, dG --; one gradient view per hook."""
        F, ns = frames, max(hook_stages) + 1
        total = mFTD = mMlp = mRows = mGram = 0
        for k in range(ns):
            D, T, np_, dh, M = self.widths[k], self.tokens(k), self.grids[k] ** 2, self.head_widths[k], self.mlp_ratios[k] * self.widths[k]
            kp, FT = (4 * self.widths[k - 1] if k else 16 * self.in_chans), F * T
            n3, n5, n7 = self.window_channels(k)
            total += D * kp + 4 * D + T * D + 9 * D + D + 9 * n3 + 25 * n5 + 49 * n7 + D
            total += self.depths[k] * (4 * D * D + 2 * M * D + 9 * D + M + 6 * FT * D + FT * M + 4 * FT + F * D * dh + 2 * F * D)
            total += F * np_ * D + 2 * F * np_ + FT * D
            mFTD, mMlp, mRows, mGram = max(mFTD, FT * D), max(mMlp, FT * M), max(mRows, F * np_ * kp), max(mGram, F * D * dh)
        total += 8 * mFTD + mMlp + mRows + mGram
        total += sum(F * self.tokens(k) * self.widths[k] for k in hook_stages)
        return 4 * total


def is_coat_name(model_name: str) -> bool:
    """A name of timm's CoaT vocabulary (`coat.py`), served (`COAT_MODELS`) or not: `graphs.build_surrogate` routes these to `coat_named`,
    which refuses the ones that are not offered with a message that lists the served names."""
    return model_name.startswith("coat")


def coat_named(model_name: str, in_hw=(224, 224)) -> CoatSpec:
    """Any row of `COAT_MODELS`, at 224 x 224 only.  Refused, each with the reason: `coat_tiny` and `coat_mini` (parallel blocks with
    bilinear cross-scale resampling), names outside the table and every other input size."""
    served = "; served: " + ", ".join(COAT_MODELS)
    if model_name in COAT_PARALLEL:
        raise ValueError(f"CoaT surrogate {model_name!r}: its parallel blocks need bilinear cross-scale resampling, which is not built "
                         "(the serial CoaT-Lite models are)" + served)
    if model_name not in COAT_MODELS:
        raise ValueError(f"CoaT surrogate {model_name!r}: not a model of this table (serial 224 x 224 models only)" + served)
    if tuple(in_hw) != (224, 224):
        raise ValueError(f"{model_name} takes 224 x 224 frames only (got {tuple(in_hw)[0]} x {tuple(in_hw)[1]})" + served)
    widths, depths, ratios = COAT_MODELS[model_name]
    return CoatSpec(model_name, 224, widths, depths, ratios)


def coat_tiny_twin(model_name: str = "coat_lite_tiny", in_hw=(64, 64)) -> CoatSpec:
    """The same topology at test size, by frame size (every served name maps to the same twins).  Not rows of `COAT_MODELS`.
      64 x 64: "coat_test" -- grids 16 -> 8 -> 4 -> 2 (the 7 x 7 window on a 2 x 2 plane), 8 heads, windows 2 / 3 / 3, widths
        32 / 32 / 64 / 96 (head widths 4 / 4 / 8 / 12), depths 2 / 1 / 2 / 1
      96 x 96: "coat_test_96" -- grids 24 -> 12 -> 6 -> 3 (an odd last grid), 4 heads, windows 1 / 2 / 1, widths 48 / 48 / 80 / 160 (no
        doublings; head widths 12 / 12 / 20 / 40, ragged against the MFMA's chunk of 16), depths 1 / 2 / 1 / 2
      224 x 224 (the size the attack classes probe a builder with): "coat_test_224" -- 3137 tokens in stage 0, widths 32 / 64 / 64 / 96,
        depths 1 / 1 / 1 / 1"""
    if in_hw[0] != in_hw[1] or int(in_hw[0]) not in (64, 96, 224):
        raise ValueError(f"the test-size CoaTs take 64 x 64, 96 x 96 or 224 x 224 frames (got {tuple(in_hw)})")
    side = int(in_hw[0])
    if side == 64:
        return CoatSpec("coat_test", 64, (32, 32, 64, 96), (2, 1, 2, 1), (8, 8, 4, 4), 8, (2, 3, 3))
    if side == 96:
        return CoatSpec("coat_test_96", 96, (48, 48, 80, 160), (1, 2, 1, 2), (8, 8, 4, 4), 4, (1, 2, 1))
    return CoatSpec("coat_test_224", 224, (32, 64, 64, 96), (1, 1, 1, 1), (8, 8, 4, 4), 8, (2, 3, 3))


def check_coat_duplicates(spec: CoatSpec, sd, where: str) -> None:
    """timm registers a stage's shared `cpe` and `crpe` again inside every serial block, so its checkpoints carry them under block-level
    keys too.  The stage-level keys are the ones loaded; a block-level duplicate that differs describes another model: refused by key
    name.  An absent one is fine."""
    import torch
    for dup, key in spec.shared_duplicates().items():
        if dup in sd and not (tuple(sd[dup].shape) == tuple(sd[key].shape) and torch.equal(sd[dup].float(), sd[key].float())):
            raise ValueError(f"{where}: {dup} differs from the stage's shared {key}")


def _window_filter_draw(shp, g):
    """A depthwise filter of `cpe` / `crpe`: N(0, 1) / window over its window^2 taps."""
    import torch
    return torch.randn(*shp, generator=g) / shp[-1]


#: Seeded stand-in for a trained CoaT-Lite, drawn per key as PiT's is: Linears and the patch convolutions ~ fan_in^-0.5 N(0, 1)
#: (`factoratt_crpe.proj` and `mlp.fc2` at half that), LayerNorm gains 1 + 0.1 N(0, 1), biases 0.02 N(0, 1).  What is new must show in
#: the tests: the class tokens are N(0, 1) and the filters of `cpe` and `crpe` N(0, 1) / window over their window^2 taps, so that each
#: window moves the features.
COAT_SYNTHETIC = [(starts("cls_token"), normal()), (lambda k: k.startswith(("cpe", "crpe")) and k.endswith("weight"), _window_filter_draw),
                  *fan_in_tail(ends("norm1.weight", "norm2.weight", "norm.weight"), half=ends("fc2.weight", "factoratt_crpe.proj.weight"))]

COAT_FAMILY = Family("coat", CoatSpec, COAT_MODELS, is_coat_name, coat_named, coat_tiny_twin, "timm's serial CoaT-Lites at 224 x 224",
                "the last block of stages {}", False, COAT_SYNTHETIC, check_coat_duplicates)


# ---------------------------------------------------------------------------
# the TNT surrogates (Transformer in Transformer): an inner transformer over the 16 pixel tokens of every patch feeding an outer ViT
# over the patches, planned on the transformer stack (include/i2v_tnt.h)
# ---------------------------------------------------------------------------
#: timm 0.5.0's `TNT` models at 224 x 224 with patch 16: name -> (dim, in_dim, blocks, heads, in_heads); MLP ratio 4 on both levels
TNT_MODELS: Dict[str, Tuple[int, int, int, int, int]] = {
    "tnt_s_patch16_224": (384, 24, 12, 6, 4),
    "tnt_b_patch16_224": (640, 40, 12, 10, 4),
}


@dataclass
class TntSpec(TokenSpec):
    """timm 0.5.0 `TNT` up to its last block (restated from memory of tnt.py, UNCHECKED against timm).
    `pixel_embed.proj`, a Conv2d(3, in_dim, 7, stride 4, padding 3), gives img / 4 positions a side; the 4 x 4 cell of patch
    n = g py + px is its 16 pixel tokens, p = 4 i + j at conv output (4 py + i, 4 px + j); `pixel_pos` (1, in_dim, 4, 4) is added per
    (c, i, j): the inner stream (frames g^2, 16, in_dim).  patch = norm2_proj(proj(norm1_proj(inner as (frames, g^2, 16 in_dim)))), the
    columns ordered p in_dim + c; `cls_token` in front, `patch_pos` (1, 1 + g^2, dim) added.  Block: inner += attn_in(norm_in inner);
    inner += mlp_in(norm_mlp_in inner); outer[:, 1:] += proj(norm1_proj(inner) as (frames, g^2, 16 in_dim)), norm1_proj over in_dim;
    outer += attn_out(norm_out outer); outer += mlp(norm_mlp outer).  An attention is `qk` = Linear(dim, 2 dim) without bias, columns
    [q of head 0.. | k of head 0..], `v` = Linear(dim, dim) without bias, scale head_dim ** -0.5, `proj` with bias; LayerNorm eps
    `ln_eps`, exact GELU.  `hooks`: depth d (1..4) -> zero-based block d * blocks / 4 - 1 (2, 5, 8, 11 of 12), whose OUTER stream behind
    it, all tokens with the class token, is the hooked feature: tokens * dim floats per frame.  `norm` and `head` lie behind every hook."""
    arch: str
    img: int
    dim: int = 384
    in_dim: int = 24
    blocks: int = 12
    heads: int = 6
    in_heads: int = 4
    mlp_ratio: int = 4
    in_chans: int = 3
    ln_eps: float = 1e-5
    hooks: Dict[int, int] = field(default_factory=dict)
    video: bool = False

    def __post_init__(self):
        if self.img % 16 or self.tokens > 208:
            raise ValueError(f"{self.arch}: a {self.img} x {self.img} frame must be whole 16 x 16 patches and at most 208 tokens with the class token")
        if self.in_dim % self.in_heads or self.in_dim % 4 or self.in_dim // self.in_heads > 16 or self.in_heads > 8:
            raise ValueError(f"{self.arch}: inner width {self.in_dim} under {self.in_heads} heads: a multiple of 4, up to 8 heads up to 16 wide")
        if self.dim % self.heads or (self.dim // self.heads) % 4 or self.dim // self.heads > 64:
            raise ValueError(f"{self.arch}: width {self.dim} under {self.heads} heads: the head width must be a multiple of 4 up to 64")
        if self.blocks % 4:
            raise ValueError(f"{self.arch}: {self.blocks} blocks: the hooks sit at every quarter of the stack")
        if not self.hooks:
            self.hooks = self.quarter_hooks()

    @property
    def grid(self) -> int:
        return self.img // 16

    @property
    def tokens(self) -> int:
        return 1 + self.grid ** 2

    @property
    def pixel_cols(self) -> int:
        """Columns of a row of the pixel gather: in_chans * 49 rounded up to a multiple of 4."""
        return (self.in_chans * 49 + 3) // 4 * 4

    @property
    def hook_dim(self) -> int:
        """Floats per frame of a hooked feature."""
        return self.tokens * self.dim

    def param_shapes(self) -> Dict[str, Tuple[int, ...]]:
        """timm `state_dict` key -> shape for every parameter up to the last block."""
        D, d, T, r = self.dim, self.in_dim, self.tokens, self.mlp_ratio
        out = {"cls_token": (1, 1, D), "patch_pos": (1, T, D), "pixel_pos": (1, d, 4, 4), "pixel_embed.proj.weight": (d, self.in_chans, 7, 7),
               "pixel_embed.proj.bias": (d,), "norm1_proj.weight": (16 * d,), "norm1_proj.bias": (16 * d,), "proj.weight": (D, 16 * d),
               "proj.bias": (D,), "norm2_proj.weight": (D,), "norm2_proj.bias": (D,)}
        for i in range(self.blocks):
            p = f"blocks.{i}."
            for outer, (w, nrm, att, nm, mlp) in enumerate(((d, "norm_in", "attn_in", "norm_mlp_in", "mlp_in"), (D, "norm_out", "attn_out", "norm_mlp", "mlp"))):
                if outer:
                    out.update({p + "norm1_proj.weight": (d,), p + "norm1_proj.bias": (d,), p + "proj.weight": (D, 16 * d), p + "proj.bias": (D,)})
                out.update({p + nrm + ".weight": (w,), p + nrm + ".bias": (w,), p + att + ".qk.weight": (2 * w, w), p + att + ".v.weight": (w, w),
                            p + att + ".proj.weight": (w, w), p + att + ".proj.bias": (w,), p + nm + ".weight": (w,), p + nm + ".bias": (w,),
                            p + mlp + ".fc1.weight": (r * w, w), p + mlp + ".fc1.bias": (r * w,), p + mlp + ".fc2.weight": (w, r * w),
                            p + mlp + ".fc2.bias": (w,)})
        return out

    def native_arrays(self, sd, n_blocks: int) -> List["torch.Tensor"]:
        """The arrays `i2v_tnt_create` takes for the first `n_blocks` blocks, from a timm-layout state dict, as float32 host tensors:
        11 in front -- the pixel filter as (in_dim, in_chans 49) rows padded with zeros to `pixel_cols`, its bias, `pixel_pos` as
        (16, in_dim) with row 4 i + j, the patch embedding's norm1_proj, proj and norm2_proj, `cls_token` as (dim), `patch_pos` as
        (tokens, dim) -- then 28 per block: the inner half as the shared block's 12 (qk.weight stacked on v.weight as the qkv weight,
        a qkv bias of zeros), the step's norm1_proj and proj, the outer half's 12."""
        import torch
        f32 = lambda k: sd[k].detach().float().cpu().contiguous()      # noqa: E731
        d, D = self.in_dim, self.dim
        pw = torch.zeros(d, self.pixel_cols)
        pw[:, :self.in_chans * 49] = f32("pixel_embed.proj.weight").reshape(d, -1)
        out = [pw, f32("pixel_embed.proj.bias"), f32("pixel_pos").reshape(d, 16).t().contiguous(), f32("norm1_proj.weight"),
               f32("norm1_proj.bias"), f32("proj.weight"), f32("proj.bias"), f32("norm2_proj.weight"), f32("norm2_proj.bias"),
               f32("cls_token").reshape(D), f32("patch_pos").reshape(self.tokens, D)]
        for i in range(n_blocks):
            p = f"blocks.{i}."
            for outer, (w, nrm, att, nm, mlp) in enumerate(((d, "norm_in", "attn_in", "norm_mlp_in", "mlp_in"), (D, "norm_out", "attn_out", "norm_mlp", "mlp"))):
                if outer:
                    out += [f32(p + "norm1_proj.weight"), f32(p + "norm1_proj.bias"), f32(p + "proj.weight"), f32(p + "proj.bias")]
                out += [f32(p + nrm + ".weight"), f32(p + nrm + ".bias"), torch.cat([f32(p + att + ".qk.weight"), f32(p + att + ".v.weight")]).contiguous(),
                        torch.zeros(3 * w), f32(p + att + ".proj.weight"), f32(p + att + ".proj.bias"), f32(p + nm + ".weight"), f32(p + nm + ".bias"),
                        f32(p + mlp + ".fc1.weight"), f32(p + mlp + ".fc1.bias"), f32(p + mlp + ".fc2.weight"), f32(p + mlp + ".fc2.bias")]
        return out

    def config_values(self):
        return (self.img, self.in_chans, self.dim, self.in_dim, self.heads, self.in_heads, self.mlp_ratio, self.blocks, self.ln_eps)

    def macs_per_frame(self) -> int:
        d, D, np_, T, r = self.in_dim, self.dim, self.grid ** 2, self.tokens, self.mlp_ratio
        inner = np_ * 16 * (d * (4 * d + 2 * r * d) + 2 * 16 * d)
        outer = T * D * (4 * D + 2 * r * D) + 2 * T * T * D
        return np_ * 16 * d * self.in_chans * 49 + np_ * 16 * d * D + self.blocks * (inner + np_ * 16 * d * D + outer)

    def workspace_bytes(self, hook_blocks: Sequence[int], frames: int) -> int:
        """Device bytes `i2v_tnt_create` plans for these hooks and `frames` frames (the formula of csrc/i2v_tnt.cpp), with R the pixel
        tokens: the 11 arrays in front and 28 per block run; per block both halves' input, qkv, mid stream, fc1 pre-activation and four
        statistics per token, and two statistics per pixel token for the step; the two top streams, the patch embedding before its
        LayerNorm with four statistics per patch; the shared scratch -- one stream, one MLP-wide and the qkv gradient at the larger of
        the two levels, the two running gradients, the pixel rows --; per hook one gradient view, and for a hook that is not the deepest
        a copy of its stream.  Nothing of either attention's score matrix."""
        F, nb, d, D, r = frames, max(hook_blocks) + 1, self.in_dim, self.dim, self.mlp_ratio
        np_, T, Kp = self.grid ** 2, self.tokens, self.pixel_cols
        R, FT, FP, Mi, M = F * np_ * 16, F * T, F * np_, r * d, r * D
        weights = d * Kp + d + 16 * d + 32 * d + D * 16 * d + 4 * D + T * D
        weights += nb * (4 * d * d + 2 * Mi * d + 9 * d + Mi + 2 * d + D * 16 * d + D + 4 * D * D + 2 * M * D + 9 * D + M)
        per_block = 5 * R * d + R * Mi + 4 * R + 2 * R + 5 * FT * D + FT * M + 4 * FT
        mS, mM = max(R * d, FT * D), max(R * Mi, FT * M)
        shared = R * d + FT * D + FP * D + 4 * FP + 4 * mS + mM + FT * D + R * d + R * Kp
        hooks = sum(FT * D * (2 if b != nb - 1 else 1) for b in hook_blocks)
        return 4 * (weights + nb * per_block + shared + hooks)


def is_tnt_name(model_name: str) -> bool:
    """A name of timm's TNT vocabulary (`tnt.py`), served (`TNT_MODELS`) or not: `graphs.build_surrogate` routes these to `tnt_named`,
    which refuses the ones that are not offered with a message that lists the served names."""
    return model_name.startswith("tnt")


def tnt_named(model_name: str, in_hw=(224, 224)) -> TntSpec:
    """Any row of `TNT_MODELS`, at 224 x 224 only.  Refused, each with the reason: names outside the table and every other input size."""
    served = "; served: " + ", ".join(TNT_MODELS)
    if model_name not in TNT_MODELS:
        raise ValueError(f"TNT surrogate {model_name!r}: not a model of this table (timm 0.5.0's 224 x 224 models with patch 16 only)" + served)
    if tuple(in_hw) != (224, 224):
        raise ValueError(f"{model_name} takes 224 x 224 frames only (got {tuple(in_hw)[0]} x {tuple(in_hw)[1]}): its position tables are "
                         "those of the 14 x 14 grid" + served)
    dim, in_dim, blocks, heads, in_heads = TNT_MODELS[model_name]
    return TntSpec(model_name, 224, dim, in_dim, blocks, heads, in_heads)


def tnt_tiny_twin(model_name: str = "tnt_s_patch16_224", in_hw=(64, 64)) -> TntSpec:
    """The same topology at test size, by frame size (every served name maps to the same twins).  Not rows of `TNT_MODELS`.  All have 4
    blocks, so that depths 1..4 hook every block.
      64 x 64: "tnt_test" -- grid 4, 17 outer tokens, 256 inner sequences a frame; in_dim 24 under 4 heads of width 6 (tnt_s's inner
        shape), dim 32 under 2 heads of width 16
      48 x 48: "tnt_test_48" -- grid 3 (odd), 10 outer tokens; in_dim 40 under 4 heads of width 10 (tnt_b's inner shape), dim 48 under
        4 heads of width 12
      224 x 224 (the size the attack classes probe a builder with): "tnt_test_224" -- 197 outer tokens, in_dim 24, dim 32 under 1 head"""
    if in_hw[0] != in_hw[1] or int(in_hw[0]) not in (64, 48, 224):
        raise ValueError(f"the test-size TNTs take 64 x 64, 48 x 48 or 224 x 224 frames (got {tuple(in_hw)})")
    side = int(in_hw[0])
    if side == 64:
        return TntSpec("tnt_test", 64, 32, 24, 4, 2, 4)
    if side == 48:
        return TntSpec("tnt_test_48", 48, 48, 40, 4, 4, 4)
    return TntSpec("tnt_test_224", 224, 32, 24, 4, 1, 4)


#: Seeded stand-in for a trained TNT, drawn per key as CoaT-Lite's is: Linears and the pixel convolution ~ fan_in^-0.5 N(0, 1) (every
#: attention's `proj`, the step's `proj` and every `fc2` at half that), LayerNorm gains 1 + 0.1 N(0, 1), biases 0.02 N(0, 1).  What is
#: new must show in the tests: `cls_token` is N(0, 1) and the two position tables 0.5 N(0, 1), so that the pixel order inside a patch
#: moves the features.
TNT_SYNTHETIC = [(keys("cls_token"), normal()), (keys("patch_pos", "pixel_pos"), normal(0.5)),
                 *fan_in_tail(lambda k: "norm" in k and k.endswith("weight"),
                              half=lambda k: k.endswith(("fc2.weight", "proj.weight")) and not k.startswith("pixel_embed"))]

TNT_FAMILY = Family("tnt", TntSpec, TNT_MODELS, is_tnt_name, tnt_named, tnt_tiny_twin, "timm's TNTs at 224 x 224",
                "the outer stream after blocks {}", False, TNT_SYNTHETIC)


# ---------------------------------------------------------------------------
# the transformer surrogate families as one table (`family.Family`)
# ---------------------------------------------------------------------------
#: the rows, in the order the resolvers and the command line ask them
FAMILIES = (VIT_FAMILY, SWIN_FAMILY, CONVNEXT_FAMILY, MIXER_FAMILY, CAIT_FAMILY, CONVIT_FAMILY, XCIT_FAMILY,
            TWINS_FAMILY, BEIT_FAMILY, PIT_FAMILY, COAT_FAMILY, TNT_FAMILY)
#: spec class -> its row
FAMILY_OF = {f.spec: f for f in FAMILIES}


# ---------------------------------------------------------------------------
# name -> graph, following the reference's `get_model` vocabulary
# ---------------------------------------------------------------------------
def build(model_name: str, in_hw=(224, 224)) -> Graph:
    """`model_name` uses the reference's names (`image_attacks.py:85-87`):
    'resnet' is ResNet-101 there (`:94-95`); 'resnet50' is added because
    BASELINE.json quotes its metric on ResNet-50."""
    if model_name == "resnet":
        return resnet((3, 4, 23, 3), 64, in_hw, "resnet101")
    if model_name == "resnet50":
        return resnet((3, 4, 6, 3), 64, in_hw, "resnet50")
    if model_name in RESNET_FAMILY:     # extension: the other torchvision ResNets, Wide ResNet and ResNeXt (grouped conv2)
        block, layers, groups, wpg = RESNET_FAMILY[model_name]
        return resnet(layers, 64, in_hw, model_name, block, groups, wpg)
    if is_seresnet_name(model_name):    # extension: timm's SE-ResNet / SE-ResNeXt family (the squeeze-and-excitation node)
        return seresnet_named(model_name, in_hw)
    if is_mnasnet_name(model_name):     # extension: torchvision's MNASNet family (depthwise 3x3 / 5x5 convolutions)
        return mnasnet_named(model_name, in_hw)
    for prefix, why in MOBILE_NOT_SERVED:
        if model_name.startswith(prefix):
            raise ValueError(f"{model_name!r} is not served: {why}; the mobile-class names served: " + ", ".join(MNASNET_MODELS))
    if model_name == "vgg":
        return vgg(VGG16_CFG, in_hw, "vgg16")
    if model_name == "alexnet":
        return alexnet(1, in_hw)
    if model_name == "squeezenet":
        return squeezenet(1, in_hw)
    if model_name == "densenet121":     # extension (BASELINE.json configs[2] names it); see `densenet`
        return densenet(32, (6, 12, 24, 16), 64, 4, in_hw, "densenet121")
    if model_name == "densenet161":
        return densenet(48, (6, 12, 36, 24), 96, 4, in_hw, "densenet161")
    for fam in FAMILIES:                # extension: the transformer surrogate of `get_vits()` (TPAMI_attack.py:88-98) and timm's families
        if fam.in_build and fam.is_name(model_name):
            return fam.named(model_name, in_hw)
    if model_name == "densenet":
        # The reference constructs densenet161 (`image_attacks.py:96-97`) but no attack class
        # has a densenet branch in `_find_target_layer` (`:260-271`): the hook lookup returns
        # None and `None.register_forward_hook` raises AttributeError.  Mirror that error.
        raise AttributeError("'NoneType' object has no attribute 'register_forward_hook'")
    # the reference leaves `model` unbound for unknown names (`image_attacks.py:103`)
    raise UnboundLocalError("local variable 'model' referenced before assignment")


def build_surrogate(model_name: str, in_hw=(224, 224)):
    """The name resolver of the image-guided attack classes and the command line: `build`, with the families in front that `build` does
    not know (`Family.in_build`: PiT, CoaT-Lite, TNT).  `build` itself keeps its vocabulary as it stands -- there a `pit_*` name is an
    unknown name, as in the reference -- so a family is added here without changing what `build` answers."""
    for fam in FAMILIES:
        if not fam.in_build and fam.is_name(model_name):
            return fam.named(model_name, in_hw)
    return build(model_name, in_hw)


#: tiny variants used by parity tests / golden fixtures (same topology, fewer channels/blocks)
def build_tiny(model_name: str, in_hw=(64, 64)) -> Graph:
    if model_name in ("resnet", "resnet50"):
        return resnet((2, 1, 2, 1), 8, in_hw, "resnet_tiny")
    if model_name == "resnext_tiny":        # groups 4, conv2 widths 16 / 32 / 64 / 128: group widths 4, 8, 16, 32; both strides; a 2 x 2 plane
        return resnet((2, 1, 2, 1), 8, in_hw, "resnext_tiny", "bottleneck", 4, 32)
    if model_name == "resnet_basic_tiny":
        return resnet((2, 1, 2, 1), 8, in_hw, "resnet_basic_tiny", "basic")
    if model_name == "seresnet_tiny":       # resnet_tiny with an SE node per block: C 32 .. 256, rd 8 / 16; planes 16 x 16 .. 2 x 2
        return resnet((2, 1, 2, 1), 8, in_hw, "seresnet_tiny", se=True)
    if model_name == "seresnext_tiny":      # resnext_tiny with an SE node per block
        return resnet((2, 1, 2, 1), 8, in_hw, "seresnext_tiny", "bottleneck", 4, 32, se=True)
    if model_name == "mnasnet_tiny":        # both filter sizes, both strides, identity blocks, 5x5 filters on 4x4 and 2x2 planes; a last plane of 2 x 2
        return mnasnet(1.0, in_hw, "mnasnet_tiny", depths=(8, 8, 8, 8, 16, 16, 16, 24),
                       stacks=((3, 2, 3, 2), (5, 2, 3, 2), (5, 2, 6, 1), (3, 1, 6, 2), (5, 2, 6, 2), (3, 1, 6, 1)))
    if model_name == "vgg":
        cfg = (8, 8, "M", 16, 16, "M", 16, 16, 16, "M", 32, 32, 32, "M", 32, 32, 32, "M")
        return vgg(cfg, in_hw, "vgg_tiny")
    if model_name == "alexnet":
        return alexnet(8, in_hw, "alexnet_tiny")
    if model_name == "squeezenet":
        return squeezenet(4, in_hw, "squeezenet_tiny")
    if model_name in ("densenet121", "densenet161"):
        return densenet(8, (2, 3, 2, 2), 16, 2, in_hw, "densenet_tiny")
    for fam in FAMILIES:
        if fam.is_name(model_name):
            if model_name not in fam.models:
                fam.named(model_name)           # (a name outside the table is refused with the served names)
            return fam.tiny_twin(model_name, in_hw)
    return build(model_name, in_hw)
