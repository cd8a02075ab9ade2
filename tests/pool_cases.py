"""TEST INFRASTRUCTURE: the case table of the pooling kernels (csrc/i2v_kernels.hip: `pool_fwd_kernel`, `pool_bwd_kernel<K,S,P>`,
`pool_bwd_321_kernel`, `pool3d_*`, `avgpool_*`) and their float64 reference.  tests/test_pool_cpu.py runs the table on the host
simulation, tests/test_gpu_pool.py on the device.

Every case is the graph  input(3) -> 3x3 conv `a` to C channels -> the pool under test -> 3x3 conv `c` to 8 channels -> hook.
The reference is torch functional code in float64 differentiated by autograd (not OracleNet's hand-written backward).

Two data constructions:
  random   seeded synthetic weights (BatchNorm behind `a`), seeded normal input.
  exact    `a` has a bias and no BatchNorm; its weights, its bias and the input are drawn from {-1, 0, 1}: every activation ahead of
           the pool is the same small integer (|v| <= 28) in fp32 and fp64, whatever the order of the sums.  Ties are everywhere
           and are decided by the rule (first maximum in scan order, as ATen), never by rounding; a ReLU'd `a` adds all-zero windows.

Band arithmetic of the 2-D max-pool launches (k_pool_fwd / k_pool_bwd; POOL_FWD_LDS_FLOATS = 4096, POOL_LDS_FLOATS / 2 = 4096 --
re-derive the comments at the banded cases when either changes):
  forward   band = (4096 // Ws - k) // stride + 1 output rows
  backward  out_rows = 4096 // Wo; out_rows >= Ho: one band; else band = (out_rows - 1) * stride - k + 1 input rows
  patch     (3/2/1, even plane halved exactly, Ws % 4 == 0) pairs = 4096 // Wo - 1 pair rows
"""
import functools
from dataclasses import dataclass
from typing import Tuple

import torch
import torch.nn.functional as F

from i2v_amd import graphs, weights
from oracle.restate import BN_EPS

HOOK_C = 8


@dataclass(frozen=True)
class Case:
    id: str
    op: str                     # "max" | "max3d" | "avg"
    k: int
    stride: int
    pad: int
    plane: Tuple[int, int]      # rows x columns
    data: str                   # "random" | "exact"
    relu: bool                  # conv `a` ends in a ReLU (the pool launch then finalises a gated gradient)
    ceil: bool = False
    N: int = 2                  # frames (image cases) / clips (video cases)
    C: int = 8
    T: int = 1                  # frames per clip (video cases)
    kt: int = 1
    stride_t: int = 1
    pad_t: int = 0
    seed: int = 0

    @property
    def frames(self):
        return self.N * self.T


def _both(id, op, k, s, p, plane, relu_random=True, relu_exact=(True, False), **kw):
    out = [Case(id + "-random", op, k, s, p, plane, "random", relu_random, **kw)]
    for r in relu_exact:
        out.append(Case(f"{id}-exact-{'relu' if r else 'linear'}", op, k, s, p, plane, "exact", r, **kw))
    return out


def _exact(id, op, k, s, p, plane, **kw):
    return [Case(f"{id}-exact-{'relu' if r else 'linear'}", op, k, s, p, plane, "exact", r, **kw) for r in (True, False)]


# ---- 2-D max pool over more than one band (wide, short planes: the cost stays trivial)
BANDED = (
    # 24 x 1000 -> 12 x 500.  Patch kernel (Ho * 2 == Hs, Wo * 2 == Ws, Ws % 4 == 0): pairs = 4096 // 500 - 1 = 7 of the 12 pair
    # rows -> 2 bands (7 + 5); output row 7 is staged by both.  Forward: 4096 // 1000 = 4 rows -> band = (4 - 3) // 2 + 1 = 1: 12 bands.
    _both("patch321", "max", 3, 2, 1, (24, 1000), seed=1)
    # 25 x 1000 -> 13 x 500: Ho * 2 != Hs, so the generic <3,2,1> on its float4 path.  out_rows = 4096 // 500 = 8 < 13:
    # band = 7 * 2 - 3 + 1 = 12 input rows -> 3 bands (12, 12, 1).  Forward: 13 bands of 1 row.
    # (seed 2 has one window -- frame 1, channel 4, output (5, 234) -- whose two largest values differ by 2.2e-7 of 0.82: fp32 and fp64
    #  pick different arg-maxes there and a whole gradient cone moves, 0.045 of max|gradient| on correct code.  Hence seed 9.)
    + _both("g321_vec", "max", 3, 2, 1, (25, 1000), relu_exact=(True,), seed=9)
    # 25 x 998 -> 13 x 499: the same bands (4096 // 499 = 8) on the 4-byte path (998 % 4 == 2).
    + [Case("g321_scalar-random", "max", 3, 2, 1, (25, 998), "random", True, seed=3)]
    # 40 x 1200 -> 20 x 600: <2,2,0>; out_rows = 4096 // 600 = 6 < 20: band = 5 * 2 - 2 + 1 = 9 input rows -> 5 bands (9, 9, 9, 9, 4);
    # 9 is odd, so the two rows of every other band-edge window lie in different bands.  Forward: 4096 // 1200 = 3 -> 20 bands of 1.
    + _both("p220", "max", 2, 2, 0, (40, 1200), relu_exact=(False,), seed=4)
    # 26 x 1001 and 26 x 1000 -> 13 x 500 (ceil_mode): <3,2,0>; the last row of windows hangs over the bottom edge (rows 24 .. 26),
    # at 1000 columns the last column of windows over the right edge too (columns 998 .. 1000); 1001 runs the 4-byte path, 1000 the
    # float4 path.  out_rows = 8 < 13: band = 12 input rows -> 3 bands (12, 12, 2).  Forward: 13 bands of 1 row.
    + _both("p320_ceil_1001", "max", 3, 2, 0, (26, 1001), relu_exact=(True,), ceil=True, seed=5)
    + _both("p320_ceil_1000", "max", 3, 2, 0, (26, 1000), relu_exact=(False,), ceil=True, seed=6)
    # 20 x 1000 -> 20 x 1000: generic <0,0,0>; out_rows = 4096 // 1000 = 4 < 20: band = 3 * 1 - 3 + 1 = 1 -> 20 backward bands of ONE
    # input row, each staging 3 output rows.  Forward: band = (4 - 3) // 1 + 1 = 2 -> 10 bands.
    + _exact("gen_k3s1", "max", 3, 1, 1, (20, 1000), seed=7)
    # 48 x 800 -> 16 x 267: generic <0,0,0>; out_rows = 4096 // 267 = 15 < 16: band = 14 * 3 - 5 + 1 = 38 input rows -> 2 bands
    # (38, 10).  Forward: 4096 // 800 = 5 -> band = (5 - 5) // 3 + 1 = 1: 16 bands.
    + [Case("gen_k5s3-random", "max", 5, 3, 2, (48, 800), "random", True, seed=8)]
)

# ---- small exact planes, one band each: the tie rule and the window table of the patch kernel are the whole point
SMALL = (_exact("s321_13x11", "max", 3, 2, 1, (13, 11), seed=11)
         + _exact("s321_12x16", "max", 3, 2, 1, (12, 16), seed=12)                 # the patch kernel on a small plane
         + _exact("s320_ceil_13x11", "max", 3, 2, 0, (13, 11), ceil=True, seed=13)
         + _exact("s220_ceil_13x11", "max", 2, 2, 0, (13, 11), ceil=True, seed=14)
         + _exact("s311_9x12", "max", 3, 1, 1, (9, 12), seed=15))


def _vid(id, kt, k, st, s, pt, p, T=5, relu=True, **kw):
    return Case(id, "max3d", k, s, p, kw.pop("plane", (9, 12)), kw.pop("data", "random"), relu, T=T, kt=kt, stride_t=st, pad_t=pt, **kw)


# ---- video max pool, 2 clips: overlapping / padded temporal windows, odd clip lengths, the clip boundary
VIDEO = (_vid("v33_22_11", 3, 3, 2, 2, 1, 1, seed=21),
         _vid("v21_21_00", 2, 1, 2, 1, 0, 0, seed=22),              # T = 5: the last frame of a clip is in no window
         _vid("v31_11_10", 3, 1, 1, 1, 1, 0, seed=23),
         _vid("v23_12_01", 2, 3, 1, 2, 0, 1, T=4, seed=24),
         _vid("v32_22_10", 3, 2, 2, 2, 1, 0, T=7, relu=False, seed=25),
         # 2 * 8 * 16 * 64 * 72 = 1 179 648 elements in both passes > 4096 blocks * 256 threads = 1 048 576: a second trip of the
         # grid-stride loop.  Exact data: the arg-max of a million windows does not depend on rounding.
         _vid("v33_11_11-stride-exact", 3, 3, 1, 1, 1, 1, T=8, C=16, plane=(64, 72), data="exact", seed=26))

# ---- average pool (pad 0; k / stride as the add call accepts them)
AVG = (Case("a22_13x11", "avg", 2, 2, 0, (13, 11), "random", False, seed=31),       # the leftover row and column get zero
       Case("a23_13x11", "avg", 2, 3, 0, (13, 11), "random", False, seed=32),       # gaps between the windows get zero
       Case("a33_14x16", "avg", 3, 3, 0, (14, 16), "random", False, seed=33),
       Case("a22_relu", "avg", 2, 2, 0, (13, 11), "random", True, seed=34),         # the pool launch finalises a ReLU-gated gradient (ungated before: 0.58 of max|ref|)
       Case("a32_13x11", "avg", 3, 2, 0, (13, 11), "random", False, seed=35),       # overlapping windows (one window per element before: 0.87)
       # 3 * 24 * 128 * 120 = 1 105 920 input elements > 1 048 576: a second trip of the backward grid-stride loop
       Case("a22_stride", "avg", 2, 2, 0, (128, 120), "random", False, N=3, C=24, seed=36))

CASES = tuple(BANDED) + tuple(SMALL) + VIDEO + AVG
BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES)
# planned for 4 frames, run with 2: the bits of a net planned for 2
FEWER_FRAMES = BY_ID["patch321-random"]
# 6 x 1400, 3/2/1: 4096 // 1400 = 2 < k -- the forward launch refuses the plane before anything runs
REFUSED = Case("refused_6x1400", "max", 3, 2, 1, (6, 1400), "random", True, seed=41)
REFUSAL_TEXT = "max-pool row too wide for the LDS band"


@dataclass
class Built:
    case: Case
    graph: "graphs.Graph"
    pool: int                   # tensor id of the pooled tensor
    hook: int                   # tensor id of the hooked feature
    sd: dict
    x: torch.Tensor             # (frames, 3, H, W) float32, frame-major
    hg: torch.Tensor            # d(cost) / d(hook), frame-major, float32


@functools.lru_cache(maxsize=None)
def build(case: Case) -> Built:
    H, W = case.plane
    video = case.op == "max3d"
    g = graphs.Graph("poolcase", (H, W), video=video)
    x = g.new_tensor(3, H, W, False, "input", T=case.T)
    g.input = x
    norm = dict(bias="a.bias") if case.data == "exact" else dict(bn="a_bn")
    if video:
        a = g.conv3d(x, case.C, (1, 3), (1, 1), (0, 1), "a.weight", relu=case.relu, name="a", **norm)
        pl = g.maxpool3d(a, (case.kt, case.k), (case.stride_t, case.stride), (case.pad_t, case.pad), name="pool")
        y = g.conv3d(pl, HOOK_C, (1, 3), (1, 1), (0, 1), "c.weight", bn="c_bn", relu=True, name="c")
    else:
        a = g.conv(x, case.C, 3, 1, 1, "a.weight", relu=case.relu, name="a", **norm)
        if case.op == "avg":
            pl = g.avgpool(a, case.k, case.stride, name="pool")
        else:
            pl = g.maxpool(a, case.k, case.stride, case.pad, ceil_mode=case.ceil, name="pool")
        y = g.conv(pl, HOOK_C, 3, 1, 1, "c.weight", bn="c_bn", relu=True, name="c")
    g.hooks[1] = y
    sd = weights.synthetic_state_dict(g, case.seed)
    gen = torch.Generator().manual_seed(1000 + case.seed)
    n = case.frames
    if case.data == "exact":
        sd["a.weight"] = torch.randint(-1, 2, sd["a.weight"].shape, generator=gen).float()
        sd["a.bias"] = torch.randint(-1, 2, sd["a.bias"].shape, generator=gen).float()
        xin = torch.randint(-1, 2, (n, 3, H, W), generator=gen).float()
    else:
        xin = torch.randn(n, 3, H, W, generator=gen)
    t = g.tensors[y]
    hg = torch.randn(n // case.T * t.T, t.C, t.H, t.W, generator=gen)
    return Built(case, g, pl, y, sd, xin, hg)


def _clips(t, T):
    """frame-major (b*T, C, H, W) -> (b, C, T, H, W)"""
    n, c, h, w = t.shape
    return t.reshape(n // T, T, c, h, w).permute(0, 2, 1, 3, 4)


def _frames(t):
    b, c, tt, h, w = t.shape
    return t.permute(0, 2, 1, 3, 4).reshape(b * tt, c, h, w)


@functools.lru_cache(maxsize=None)
def reference(case: Case):
    """float64: {"pool", "feat", "gx"} frame-major, by torch functional code and torch.autograd.grad."""
    b = build(case)
    sd = {k: v.double() for k, v in b.sd.items()}

    def bn(t, pre):
        return F.batch_norm(t, sd[pre + ".running_mean"], sd[pre + ".running_var"], sd[pre + ".weight"], sd[pre + ".bias"], False, 0.0, BN_EPS)
    x = b.x.double().requires_grad_(True)
    if case.op == "max3d":
        a = F.conv3d(_clips(x, case.T), sd["a.weight"], sd.get("a.bias"), 1, (0, 1, 1))
    else:
        a = F.conv2d(x, sd["a.weight"], sd.get("a.bias"), 1, 1)
    if case.data != "exact":
        a = bn(a, "a_bn")
    if case.relu:
        a = F.relu(a)
    if case.op == "max3d":
        p = F.max_pool3d(a, (case.kt, case.k, case.k), (case.stride_t, case.stride, case.stride), (case.pad_t, case.pad, case.pad))
        y = F.relu(bn(F.conv3d(p, sd["c.weight"], None, 1, (0, 1, 1)), "c_bn"))
        p, y = _frames(p), _frames(y)
    else:
        if case.op == "avg":
            p = F.avg_pool2d(a, case.k, case.stride)
        else:
            p = F.max_pool2d(a, case.k, case.stride, case.pad, ceil_mode=case.ceil)
        y = F.relu(bn(F.conv2d(p, sd["c.weight"], None, 1, 1), "c_bn"))
    gx, = torch.autograd.grad((y * b.hg.double()).sum(), x)
    return {"pool": p.detach(), "feat": y.detach(), "gx": gx.detach(), "src": (a if case.op != "max3d" else _frames(a)).detach()}


def tied_windows(case: Case) -> int:
    """2-D max-pool windows of the reference whose maximum occurs more than once among their in-plane taps."""
    assert case.op == "max"
    ref = reference(case)
    a, p = ref["src"], ref["pool"]
    far = case.k + case.stride                              # room for ceil_mode's overhanging windows
    ap = F.pad(a, (case.pad, far, case.pad, far), value=float("-inf"))
    u = ap.unfold(2, case.k, case.stride).unfold(3, case.k, case.stride)[:, :, :p.shape[2], :p.shape[3]]
    hits = (u == p[..., None, None]).sum((-1, -2))
    assert int(hits.min()) >= 1
    return int((hits > 1).sum())


def run(eng, case: Case, to_dev, write_grads, planned=None, passes=1):
    """Plan the case's net on `eng` (for `planned` frames instead of the case's own), run the case's frames through it `passes`
    times: a list of ({tensor id: activation}, input gradient) on the CPU, one per pass.  The hook gradient is gated by the
    REFERENCE feature's ReLU, so every backend gets the same bits."""
    b = build(case)
    ref = reference(case)
    g = b.graph
    n = case.frames
    t_in = case.T
    net = eng.build_net(g, b.sd, [b.hook], planned or case.frames)
    out = []
    try:
        for _ in range(passes):
            net.forward(to_dev(b.x[:n]))
            acts = {}
            for nd in net.graph.nodes:
                acts[nd.dst] = net.read_tensor(nd.dst, n // t_in * g.tensors[nd.dst].T).cpu()
            nh = n // t_in * g.tensors[b.hook].T
            write_grads(net, [ref["feat"][:nh]], [b.hg[:nh]], nh)
            gx = to_dev(torch.full((n, 3) + case.plane, float("nan")))
            net.backward(gx)
            out.append((acts, gx.cpu()))
    finally:
        net.close()
    return out


def errors(case: Case, built: Built, acts, gx, ref):
    """(pooled max-abs error, feature error / bound, gradient error / max|ref|) of one pass against the reference."""
    pool, feat = acts[built.pool].double(), acts[built.hook].double()
    rp, rf, rg = ref["pool"][:pool.shape[0]], ref["feat"][:feat.shape[0]], ref["gx"][:gx.shape[0]]
    return (float((pool - rp).abs().max()), float((feat - rf).abs().max() / rf.abs().max()),
            float((gx.double() - rg).abs().max() / rg.abs().max()))


def check(case: Case, built: Built, acts, gx, ref):
    """The bounds of test_maxpool_geometries / test_conv_property_based (the same graph shape): pooled tensor rtol 1e-5, atol 1e-6
    (exact data: equal); hooked feature and input gradient max|got - ref| <= 1e-5 * max|ref| + 1e-6 / 1e-7."""
    pool, feat = acts[built.pool].double(), acts[built.hook].double()
    rp, rf, rg = ref["pool"][:pool.shape[0]], ref["feat"][:feat.shape[0]], ref["gx"][:gx.shape[0]]
    assert pool.shape == rp.shape and feat.shape == rf.shape and gx.shape == rg.shape
    assert bool(torch.isfinite(gx).all()), "the backward pass left input-gradient elements unwritten"
    if case.data == "exact":
        assert torch.equal(pool, rp), f"{case.id}: pooled tensor differs from the exact reference at {int((pool != rp).sum())} elements"
    assert torch.allclose(pool, rp, rtol=1e-5, atol=1e-6), (case.id, float((pool - rp).abs().max()))
    assert (feat - rf).abs().max() <= 1e-5 * rf.abs().max() + 1e-6, (case.id, float((feat - rf).abs().max()), float(rf.abs().max()))
    assert float(rg.abs().max()) > 0
    err = (gx.double() - rg).abs().max()
    assert err <= 1e-5 * rg.abs().max() + 1e-7, (case.id, float(err / rg.abs().max()))
