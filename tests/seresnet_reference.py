"""TEST INFRASTRUCTURE: timm's SE-ResNet / SE-ResNeXt family restated on plain torch functions over the graph IR, in float64 or float32 on
the CPU.  The interpreter is the one of tests/resnet_family_reference.py (`F.conv2d(..., groups=)`, eval-mode BatchNorm, max-pool,
residual addends, ReLU) plus the squeeze-and-excitation op of timm 0.5.0's `SEModule` (mean over the plane, fc1 + ReLU, fc2 + sigmoid,
scale) with the shortcut add and ReLU the node carries; the input gradient is autograd's.  `SeRef` also has the interface of
`oracle.restate.OracleNet` that `oracle.restate.run_attack` drives (`.dtype`, `.hooks`, `.forward`, `.backward`), as
tests/vit_reference.py's `VitReference` has.  `const_gate` replaces every gate by a constant: what a dead gate would compute."""
import torch
import torch.nn.functional as F

from tests.resnet_family_reference import BN_EPS, case_inputs, rel_l2  # noqa: F401


def node_alone_graph(C, rd, plane, residual, relu):
    """3-channel 3x3 stem (BN, ReLU) -> 1x1 convolution (BN, linear) -> SE node, the stem output as residual when asked -> hook 1."""
    from i2v_amd import graphs
    g = graphs.Graph("se_case", (plane, plane))
    x = g.new_tensor(3, plane, plane, False, "input")
    g.input = x
    a = g.conv(x, C, 3, 1, 1, "stem.weight", bn="stem_bn", relu=True, name="stem")
    b = g.conv(a, C, 1, 1, 0, "lin.weight", bn="lin_bn", relu=False, name="lin")
    y = g.se(b, rd, "se", relu=relu, residual=a if residual else None, name="out")
    g.hooks[1] = y
    return g


#: the node alone: (C, rd, plane, residual, relu, frames)
NODE_CASES = [(16, 8, 7, True, True, 3),         # HW = 49, odd: gate words straddle frames
              (32, 8, 9, False, True, 3),        # no residual
              (64, 8, 14, True, False, 3),       # identity output, no gate rows
              (64, 8, 1, True, True, 3),         # a 1 x 1 plane
              (256, 16, 56, True, True, 2),      # layer1's shape, 16-byte path
              (2048, 128, 7, True, True, 3)]     # layer4's shape


def case_id(case):
    return "C%d_rd%d_p%d_r%d_a%d" % (case[0], case[1], case[2], int(case[3]), int(case[4]))


def n_se(graph, hooks):
    return sum(1 for nd in graph.truncated(list(hooks)).nodes if nd.op == "se")


class SeRef:
    def __init__(self, graph, sd, hook_tensors, dtype=torch.float64, const_gate=None):
        self.g, self.hooks, self.dtype = graph.truncated(list(hook_tensors)), list(hook_tensors), dtype
        self.sd = {k: v.to(dtype) for k, v in sd.items()}
        self.const_gate = const_gate
        self.gates = []                    # the s of every SE node of the last `features` call, (N, C) each
        self._x = self._feats = None

    def features(self, x):
        """The hooked features of frames `x` (differentiable)."""
        g, sd = self.g, self.sd
        val = {g.input: x}
        self.gates = []
        for nd in g.nodes:
            src = val[nd.src]
            if nd.op == "conv":
                y = F.conv2d(src, sd[nd.weight], sd[nd.bias] if nd.bias else None, nd.stride, nd.pad, 1, nd.groups)
                if nd.bn:
                    y = F.batch_norm(y, sd[nd.bn + ".running_mean"], sd[nd.bn + ".running_var"], sd[nd.bn + ".weight"], sd[nd.bn + ".bias"],
                                     False, 0.0, BN_EPS)
                if nd.residual is not None:
                    y = y + val[nd.residual]
                if nd.relu:
                    y = F.relu(y)
            elif nd.op == "se":
                m = src.mean((2, 3), keepdim=True)
                h = F.relu(F.conv2d(m, sd[nd.fc1 + ".weight"], sd[nd.fc1 + ".bias"]))
                s = torch.sigmoid(F.conv2d(h, sd[nd.fc2 + ".weight"], sd[nd.fc2 + ".bias"]))
                self.gates.append(s.detach().flatten(1))
                if self.const_gate is not None:
                    s = torch.full_like(s, self.const_gate)
                y = src * s
                if nd.residual is not None:
                    y = y + val[nd.residual]
                if nd.relu:
                    y = F.relu(y)
            elif nd.op == "maxpool":
                y = F.max_pool2d(src, nd.k, nd.stride, nd.pad, ceil_mode=nd.ceil_mode)
            else:
                raise NotImplementedError(nd.op)
            val[nd.dst] = y
        return [val[t] for t in self.hooks]

    def run(self, x, hook_grads=None):
        """(hook features, d sum_i <hook_i, hook_grads_i> / dx or None).  `hook_grads` are taken as given: d(cost)/d(hook)."""
        x = x.to(self.dtype).clone().requires_grad_(hook_grads is not None)
        feats = self.features(x)
        gx = None
        if hook_grads is not None:
            tot = sum((f * h.to(self.dtype)).sum() for f, h in zip(feats, hook_grads))
            gx, = torch.autograd.grad(tot, x)
        return [f.detach() for f in feats], gx

    # -- the interface oracle.restate.run_attack drives --
    def forward(self, x):
        self._x = x.detach().to(self.dtype).requires_grad_(True)
        self._feats = self.features(self._x)
        return [f.detach() for f in self._feats]

    def backward(self, hook_grads):
        return torch.autograd.grad(self._feats, self._x, [h.to(self.dtype).reshape(f.shape) for h, f in zip(hook_grads, self._feats)])[0].detach()


def reference(graph, sd, hooks, x, hg):
    """The float64 results of a case: (features, gated hook gradients, input gradient, the reference).  The gradients are gated by the
    float64 features' ReLU, as the device tests gate theirs."""
    r64 = SeRef(graph, sd, hooks, torch.float64)
    f64, _ = r64.run(x)
    gated = [h * (f > 0).to(h.dtype) if graph.tensors[t].post_relu else h for h, f, t in zip(hg, f64, hooks)]
    _, g64 = r64.run(x, gated)
    return f64, gated, g64, r64


def fp32_cpu_errors(graph, sd, hooks, x, hg):
    """Relative L2 error of the float32 CPU run of this reference against its float64 run: per hook, and of the input gradient."""
    f64, gated, g64, _ = reference(graph, sd, hooks, x, hg)
    f32, g32 = SeRef(graph, sd, hooks, torch.float32).run(x, gated)
    return {"hooks": [rel_l2(a, b) for a, b in zip(f32, f64)], "gx": rel_l2(g32, g64)}


def gate_condition(graph, sd, hooks, x):
    """What keeps a dead or constant gate from passing: (relative L2 distance, per hook, between the float64 features and the float64
    features with every gate replaced by 0.5; smallest and largest true gate over the case)."""
    r64 = SeRef(graph, sd, hooks, torch.float64)
    f64, _ = r64.run(x)
    s = torch.cat([g.flatten() for g in r64.gates])
    half, _ = SeRef(graph, sd, hooks, torch.float64, const_gate=0.5).run(x)
    return [rel_l2(a, b) for a, b in zip(half, f64)], float(s.min()), float(s.max())
