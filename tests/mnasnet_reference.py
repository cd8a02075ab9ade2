"""TEST INFRASTRUCTURE: torchvision's MNASNet restated on plain torch functions over the graph IR -- the depthwise nodes are
`F.conv2d(..., groups=C)` -- in float64 or float32 on the CPU.  The interpreter is the one of tests/resnet_family_reference.py (it
takes `groups`, eval-mode BatchNorm, residual addends and ReLU from the nodes); this module adds the depthwise node cases."""
from tests.resnet_family_reference import FamilyRef, case_inputs, dense_twin, fp32_cpu_errors, rel_l2  # noqa: F401


def node_alone_graph(C, k, plane, stride):
    """One depthwise node: k x k / `stride` / pad k // 2 over C channels (BN, ReLU) -> hook 1.  The engine does not plan a depthwise (or
    grouped) node directly on the caller's frames, and a gradient gate exists only behind a ReLU, so the C channels are made from
    the 3-channel input by a 1x1 convolution (BN, ReLU) and nothing else: no spatial stem."""
    from i2v_amd import graphs
    g = graphs.Graph("dwconv_case", (plane, plane))
    x = g.new_tensor(3, plane, plane, False, "input")
    g.input = x
    a = g.conv(x, C, 1, 1, 0, "lift.weight", bn="lift_bn", relu=True, name="lift")
    y = g.conv(a, C, k, stride, k // 2, "dw.weight", bn="dw_bn", relu=True, name="dw", groups=C)
    g.hooks[1] = y
    return g


#: the depthwise node alone: (C, k, plane, stride, frames)
NODE_CASES = [(8, 3, 7, 1, 3),        # 49 is not a multiple of 32: gate words straddle frames
              (5, 5, 9, 2, 3),        # odd channel count, odd plane, 9 -> 5
              (16, 3, 8, 2, 2),       # stride 2 on an even plane
              (24, 5, 14, 2, 2),
              (16, 5, 2, 1, 2),       # filter larger than the plane
              (16, 5, 2, 2, 3),       # 2 x 2 -> 1 x 1
              (1152, 5, 7, 1, 2),     # full channel width
              (32, 3, 112, 1, 1)]     # the largest plane


def case_id(case):
    return "C%d_k%d_p%d_s%d" % tuple(case[:4])


def n_depthwise(graph, hooks):
    return sum(1 for nd in graph.truncated(list(hooks)).nodes if nd.op == "conv" and nd.groups > 1)
