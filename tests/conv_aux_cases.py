"""TEST INFRASTRUCTURE: the case table of the grouped 3x3 convolution (csrc/i2v_gconv.hip), the depthwise k x k convolution
(csrc/i2v_dwconv.hip) and the squeeze-and-excitation node (csrc/i2v_se.hip; scalar twin csrc/i2v_se_host.h), with input generators and a
float64 reference per case.  tests/test_gpu_conv_aux.py runs the table on the device through the C entries of
include/i2v_conv_aux_launch.h; tests/test_conv_aux_cpu.py checks the packers (exported by every build), runs the SE cases on the host
simulation, and checks that the table, the reference and `check` can tell a wrong kernel from a right one.  The buffer helpers are
those of tests/xf_cases.py, imported.

A case is one forward launch and one input-gradient launch of the same layer.  `run(engine, case)` returns {name: CPU tensor} (a
`Result`: `.plans` holds what the entries reported); `reference(case)` returns {name: (kind, ...)} over the SAME names.

Kinds and bounds (`check`):
  planes   a value output.  The error is taken per (frame, channel) plane: max|got - want| over the plane divided by the plane's scale;
           the case's error is its worst plane, held to max(2e-6, 4 e32) (tests/xf_cases.py's floor and DESIGN.md section 14's factor).
           Convolutions: the scale is the plane's largest float64 PRE-ACTIVATION magnitude (sum + shift, before ReLU and gate), so a plane
           that ReLU or the gate zeroes entirely still has one.  SE: the plane's max|want|, the tensor's where the plane is identically
           zero; the vectors m, h, s, t, dmh are taken per frame (a frame's vector is the plane).  Where the backward gate or mask is off
           the output must be +0.0 bit for bit.
  gate     the gate rows a forward launch wrote: every bit equals (the device's OWN dst value > 0) -- self-consistency, so a value within
           rounding of zero cannot make the test ambiguous --, the unused high bits of a row's last written word are 0, and every later
           word and all slack keep the sentinel.  (`rmw`: the host twin sets and clears bits in place, the unused bits keep what they held.)
  exact    equal bits: the slack around every output, the gap between frames where dst_nstride exceeds the frame included.
e32 is the same measure on a float32 CPU evaluation of the reference against float64, committed as
tests/golden/conv_aux_fp32_cpu_errors.json (tests/make_conv_aux_fixtures.py); nothing in a bound comes from the device.  For the two
convolutions it is the larger of (a) float32 torch (`F.conv2d`, its autograd gradient) and (b) the float32 fma chain in the order
csrc/i2v_params.h states -- gconv: ci outer, tap inner; dwconv: row-major taps; the taps a class does not own skipped -- evaluated in
numpy with float64 standing in for each fma (`params_eval(chain=True)` on the operands of the library's own packers): a correct kernel
with 576-term sequential chains need not look like torch's blocked sums.

Buffers (xf_cases._Buf).  Every operand lies FRONT = 128 floats into a larger allocation with a tail behind it; everything of an OUTPUT
allocation that is not an addressed element is SENTINEL, its addressed elements start as NaN; everything of an INPUT allocation that is
not an addressed element is NaN (gate rows: all ones), so a stray read poisons a checked output.

THE PLAN ARITHMETIC BELOW (`gconv_plan`, `dwconv_plan`, `lpr`) IS A RESTATEMENT of k_gconv_plan / gconv_rows (csrc/i2v_gconv.hip) and
k_dwconv_plan / dwconv_rows / dwconv_v4 (csrc/i2v_dwconv.hip).  Re-derive it, and the branch comments at the cases, when those or the
40 KB / 160 KB (gconv) and 32 KB / 64 KB (dwconv) limits change.  The device test asserts the plan each entry REPORTS against it.
  k_gconv: a block is 64 w positions (w = 4, 2, 1: the widest whose LDS image gw x rows x (Ws + 2) floats fits 40 KB, else the smallest
    image; refused above 160 KB; above 64 KB hipFuncSetAttribute raises the limit).  Staging: lpr = 64 halved while >= 16 and lpr / 2 >=
    pitch = Ws + 2 lanes along a row; pitch > 64 takes a second trip of the column loop.
  k_dwconv: w = 1 doubled while < 16 and 64 w < 8 Wg_max, then halved while rows x pitch floats > 32 KB (refused if > 64 KB at w = 1).
    V4 (16-byte staging, pitch Ws + 8): Ws % 4 == 0, src_nstride % 4 == 0, src 16-byte aligned; else pitch Ws + 2 pad.  Instantiations:
    K 3 / 5 x ALL (every class owns every slot: forward, stride-1 gradient) / tapmask (stride-2 gradient) x V4 / plain.
  SE: squeeze, one wave per plane, lane l owns elements e with (e / 4) % 64 == l: a second trip from HW > 256; 16-byte loads where HW % 4
    == 0 and x (and g) are aligned; four waves per block (C % 4: a partly empty block).  Excite: lanes over c = l, l + 64, .. (C > 64: a
    second trip; C % 64: a partial one), the block's four waves over j (rd % 4), 256 threads over c (C > 256).  Scale: 256 x V positions
    per block, V = 4 where HW % 4 == 0 and x / g, r, dst are aligned.
The 2^31-position guards of the three launches are left to code reading: a refusal there could only be tested by a call whose failure
would run a kernel out of bounds.
"""
import ctypes
import functools
import zlib

import numpy as np
import torch
import torch.nn.functional as F

from i2v_amd import lib
from tests.xf_cases import FLOOR, FRONT, SENTINEL, Case, P, _Buf, _Ctx, bound, same_bits  # noqa: F401  (same_bits: for the test modules)

SENT_BITS = int(torch.tensor([SENTINEL]).view(torch.int32).item())
GFRONT, GTAIL = 32, 96                    # words ahead of and behind the gate rows
VALUE = {"gconv": ("y", "dx"), "dwconv": ("y", "dx"), "se": ("m", "h", "s", "y", "t", "dmh", "dx")}
# forward (shift, relu, gate_out) and backward (gate | mask | none) epilogues, cycled over the cases of a kernel
EPI = ((0, 0, 0, "none"), (1, 0, 0, "mask"), (1, 1, 1, "gate"), (0, 1, 1, "mask"), (1, 1, 0, "none"), (0, 1, 0, "gate"))
GAPS = ((0, 0), (3, 1), (4, 4), (1, 0))   # (dst frame stride - frame, src frame stride - frame) in floats, cycled (gconv)


def out_plane(v, st):
    return (v - 1) // st + 1


class Result(dict):
    plans = None


# ---------------------------------------------------------------------------------------------------------------------------
# the plan arithmetic, restated (see the docstring)
# ---------------------------------------------------------------------------------------------------------------------------
def classes(H, W, st, backward):
    """[(Hg, Wg, oh0, ow0)] of a launch whose convolution has the input plane (H, W): conv_aux::conv_classes."""
    if not backward:
        return [(out_plane(H, st), out_plane(W, st), 0, 0)]
    return [((H - ph + st - 1) // st, (W - pw + st - 1) // st, ph, pw) for ph in range(st) for pw in range(st)]


def _rows(cls, Hs, S, P_, k):
    RP, worst = Hs + 2 * (k // 2), k
    for Hg, Wg, _, _ in cls:
        HW = Hg * Wg
        for b in range(max(HW, 0)):
            q0, q1 = b * P_, b * P_ + P_ - 1
            nv = (q1 // HW) * RP + ((q1 % HW) // Wg) * S + k - 1 - ((q0 // HW) * RP + ((q0 % HW) // Wg) * S) + 1
            worst = max(worst, nv)
    return worst


def _src_plane(H, W, st, backward):
    return (out_plane(H, st), out_plane(W, st)) if backward else (H, W)


def gconv_plan(gw, H, W, st, backward):
    """{waves, rows, pitch, lds_bytes, v4, first_lds} of k_gconv_plan, or None where it refuses (first_lds: the w = 4 image)."""
    Hs, Ws = _src_plane(H, W, st, backward)
    cls, S, pitch, best, first = classes(H, W, st, backward), (1 if backward else st), Ws + 2, None, None
    for w in (4, 2, 1):
        rows = _rows(cls, Hs, S, 64 * w, 3)
        lds = gw * rows * pitch * 4
        first = lds if first is None else first
        if best is None or lds < best[2]:
            best = (w, rows, lds)
        if lds <= 40 * 1024:
            best = (w, rows, lds)
            break
    if best[2] > 160 * 1024:
        return None
    return dict(waves=best[0], rows=best[1], pitch=pitch, lds_bytes=best[2], v4=0, first_lds=first)


def gconv_refused_lds(gw, H, W, st, backward):
    """The smallest LDS image k_gconv_plan finds for a shape it refuses."""
    Hs, Ws = _src_plane(H, W, st, backward)
    cls, S = classes(H, W, st, backward), (1 if backward else st)
    return min(gw * _rows(cls, Hs, S, 64 * w, 3) * (Ws + 2) * 4 for w in (4, 2, 1))


def lpr(pitch):
    v = 64
    while v > 8 and (v >> 1) >= pitch:
        v >>= 1
    return v


def dwconv_plan(k, H, W, st, backward, aligned=True, nstride4=True):
    """{waves, rows, pitch, lds_bytes, v4, first_waves} of k_dwconv_plan, or None where it refuses."""
    Hs, Ws = _src_plane(H, W, st, backward)
    cls, S = classes(H, W, st, backward), (1 if backward else st)
    v4 = int(Ws % 4 == 0 and aligned and nstride4)
    pitch = Ws + 8 if v4 else Ws + 2 * (k // 2)
    wmax = max([1] + [c[1] for c in cls if c[0] > 0 and c[1] > 0])
    w = 1
    while w < 16 and 64 * w < 8 * wmax:
        w <<= 1
    first = w
    while True:
        rows = _rows([c for c in cls if c[0] > 0 and c[1] > 0], Hs, S, 64 * w, k)
        lds = rows * pitch * 4
        if lds <= 32 * 1024 or w == 1:
            if lds > 64 * 1024:
                return None
            return dict(waves=w, rows=rows, pitch=pitch, lds_bytes=lds, v4=v4, first_waves=first)
        w >>= 1


def port_plan(case, backward, src_off=0, sgap=None):
    kw = case.kw
    if case.op == "gconv":
        return gconv_plan(kw["gw"], kw["H"], kw["W"], kw["st"], backward)
    Hs, Ws = _src_plane(kw["H"], kw["W"], kw["st"], backward)
    sgap = kw["sgap"] if sgap is None else sgap
    return dwconv_plan(kw["k"], kw["H"], kw["W"], kw["st"], backward, src_off % 4 == 0, (kw["C"] * Hs * Ws + sgap) % 4 == 0)


# ---------------------------------------------------------------------------------------------------------------------------
# the table
# ---------------------------------------------------------------------------------------------------------------------------
def _conv(op, i, N, H, W, st, epi=None, gap=None, sgap=None, **kw):
    shift, relu, gout, bwd = EPI[i % 6] if epi is None else EPI[epi]
    dg, sg = GAPS[i % 4]
    d = dict(N=N, H=H, W=W, st=st, shift=shift, relu=relu, gout=gout, bwd=bwd, gap=dg if gap is None else gap, sgap=sg if sgap is None else sgap, **kw)
    what = f"g{kw['G']}x{kw['gw']}" if op == "gconv" else f"c{kw['C']}-k{kw['k']}"
    id = f"{op}-{what}-{H}x{W}-s{st}-n{N}-" + ("b" if shift else "") + ("r" if relu else "") + ("g" if gout else "") + "-" + bwd
    return Case(id, op, tuple(sorted(d.items())))


def _gconv_cases():
    # (groups, gw, H, W, N): the input plane of the convolution; each at stride 1 and 2.  N covers 1, 2, 5.
    shapes = (
        (3, 4, 5, 9, 2),        # gw 4, H < W; lpr 16
        (2, 8, 9, 5, 5),        # gw 8, H > W; five frames
        (3, 16, 6, 15, 2),      # pitch 17: lpr 32
        (2, 32, 5, 9, 1),       # gw 32 (two COB blocks of 16), one frame
        (2, 64, 9, 5, 2),       # gw 64 (four COB blocks)
        (2, 4, 2, 63, 2),       # pitch 65: the second trip of the staging loop; stride 1: waves 4, rows 14, 14 560 B
        (2, 4, 5, 1, 5),        # a 1-wide plane (lpr 8): rows 360 at stride 1
        (3, 4, 1, 1, 2),        # a 1 x 1 plane
        (2, 32, 3, 56, 1),      # no width fits 40 KB: the smallest image is taken, waves 1, 44 544 B
        (2, 64, 3, 56, 1),      # above 64 KB, the attribute path: 89 088 B; its stride-2 gradient 115 200 B
        (2, 16, 5, 28, 2),      # stride 2: forward lpr 32, gradient (3 x 14) lpr 16 and waves 2; classes 3x14, 3x14, 2x14, 2x14
        (3, 8, 7, 9, 1),        # odd in both axes: stride 2 gives 4 x 5 and four classes of four sizes
        (2, 4, 8, 8, 2),        # N Hg Wg = 128: a multiple of 64 (every other shape here is not)
    )
    out, i = [], 0
    for G, gw, H, W, N in shapes:
        for st in (1, 2):
            out.append(_conv("gconv", i, N, H, W, st, G=G, gw=gw))
            i += 1
    return out


def _dwconv_cases():
    # (C, k, H, W, N, strides, epilogue or None: cycled, src frame gap)
    shapes = (
        (3, 5, 6, 12, 2, (1, 2), None, 0),      # k 5 with 16-byte staging: forward V4, pitch 20; stride-2 gradient source 3 x 6: plain, pitch 10
        (5, 3, 5, 8, 2, (1, 2), None, 4),       # k 3: forward V4; stride-2 gradient source 3 x 4: V4 with a tap mask; frame stride + 4 keeps V4
        (3, 5, 2, 160, 2, (2,), None, 0),       # first choice 16 waves, planned 8: 31 584 B
        (2, 5, 2, 200, 1, (2,), None, 0),       # 16 -> 4: two halvings
        (3, 5, 2, 2, 2, (1, 2), None, 0),       # planes smaller than the filter
        (3, 5, 1, 1, 5, (1, 2), None, 0),
        (3, 3, 1, 7, 2, (1, 2), None, 0),
        (5, 3, 7, 1, 1, (1, 2), None, 0),
        (6, 3, 7, 7, 3, (1,), 2, 0),            # 49-position planes, three frames: gate words straddle frames
        (6, 5, 7, 7, 1, (1,), 3, 0),            # ... and one frame: 17 unused bits in the last word
        (3, 5, 5, 16, 2, (2,), None, 0),        # k 5 stride-2 gradient on a 3 x 8 source: V4 with a tap mask
        (3, 3, 7, 9, 1, (2,), None, 1),         # k 3 stride-2 gradient on a 4 x 5 source: plain with a tap mask
        (3, 3, 5, 9, 2, (1,), None, 0),         # k 3 plain, every slot
    )
    out, i = [], 0
    for C, k, H, W, N, sts, epi, sgap in shapes:
        for st in sts:
            out.append(_conv("dwconv", i, N, H, W, st, epi=epi, gap=(0, 3, 4)[i % 3], sgap=sgap, C=C, k=k))
            i += 1
    return out


SE_EPI = ((1, 1, 1), (0, 1, 1), (1, 0, 0), (0, 0, 0), (1, 1, 0))      # (residual, relu, gate_out)


def _se(i, N, C, rd, HW, hot=0, epi=None):
    res, relu, gout = SE_EPI[i % 5] if epi is None else SE_EPI[epi]
    d = dict(N=N, C=C, rd=rd, HW=HW, res=res, relu=relu, gout=gout, hot=hot, gap=(0, 4, 8)[i % 3])
    id = f"se-n{N}-c{C}-rd{rd}-hw{HW}-" + ("a" if res else "") + ("r" if relu else "") + ("g" if gout else "") + ("-hot" if hot else "")
    return Case(id, "se", tuple(sorted(d.items())))


def _se_cases():
    shapes = (
        (2, 6, 1, 289),         # 17 x 17: the scalar squeeze's second trip; C 6: a partly empty squeeze block; rd 1
        (2, 8, 6, 260),         # 16-byte path with a partial second trip; N HW = 520: a multiple of 4, not of 1024; rd 6
        (3, 4, 2, 1),           # HW 1
        (3, 6, 6, 3),           # HW 3; N HW = 9: no multiple of 32
        (2, 70, 16, 4),         # HW 4; C 70: above 64 and no multiple of it; rd 16
        (1, 300, 6, 16),        # C 300: the second trip of the per-thread channel loop
        (5, 12, 3, 64),         # five frames, rd 3
    )
    out = [_se(i, *s) for i, s in enumerate(shapes)]
    out.append(_se(7, 2, 16, 6, 20, hot=1, epi=0))       # saturated sigmoids and exactly zero h
    out.append(_se(8, 1, 2048, 128, 49, epi=1))          # the full-width row
    return out


GCONV_CASES, DWCONV_CASES, SE_CASES = tuple(_gconv_cases()), tuple(_dwconv_cases()), tuple(_se_cases())
CONV_CASES = GCONV_CASES + DWCONV_CASES
CASES = CONV_CASES + SE_CASES
BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES)
HOT = next(c for c in SE_CASES if c.kw["hot"])
FRAME_INVARIANCE = ("gconv-g2x8-9x5-s2-n5-rg-mask", "gconv-g2x4-5x1-s1-n5--none", "dwconv-c6-k3-7x7-s1-n3-brg-gate", "dwconv-c3-k5-1x1-s2-n5-rg-mask",
                    "se-n5-c12-rd3-hw64-rg", "se-n3-c6-rd6-hw3-")
# 16-byte staging dropped by alignment alone: (case, how) -- no bit of any output may change
V4_DROPPED = tuple((cid, how) for cid in ("dwconv-c3-k5-6x12-s1-n2--none", "dwconv-c5-k3-5x8-s2-n2-rg-mask", "dwconv-c3-k5-5x16-s2-n2-br-none")
                   for how in (dict(src_off=1), dict(sgap=1)))
SE_MISALIGNED = ("se-n2-c8-rd6-hw260-rg", "se-n2-c70-rd16-hw4-ar")


# ---------------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def inputs(case: Case):
    """{name: CPU tensor} in the operation's own shapes; read-only, shared by run and reference."""
    kw, g = case.kw, torch.Generator().manual_seed(zlib.crc32(case.id.encode()))
    rn = lambda *s: torch.randn(*s, generator=g)
    N = kw["N"]
    if case.op == "se":
        C, rd, HW = kw["C"], kw["rd"], kw["HW"]
        inp = {"x": rn(N, C, HW), "g": rn(N, C, HW), "r": rn(N, C, HW), "w1": rn(rd, C) * C ** -0.5, "b1": 3.0 + 0.3 * rn(rd),      # (every h > 0: exact zeros are the `hot` case's)
               "w2": rn(C, rd) * rd ** -0.5, "b2": 0.5 * rn(C)}
        if kw["hot"]:
            c, j = torch.arange(C), torch.arange(rd)
            inp["b2"] = torch.where(c % 2 == 0, torch.where(c % 4 == 0, 30.0, -30.0), inp["b2"])      # half the channels saturate
            inp["b1"] = torch.where(j % 3 == 0, -50.0, inp["b1"] - 3.0)                               # h[j] exactly 0 there
        return inp
    C = kw["G"] * kw["gw"] if case.op == "gconv" else kw["C"]
    cin, k = (kw["gw"], 3) if case.op == "gconv" else (1, kw["k"])
    H, W, st = kw["H"], kw["W"], kw["st"]
    Ho, Wo = out_plane(H, st), out_plane(W, st)
    on = torch.rand(N, C, H, W, generator=g) < 0.6
    pos, neg = rn(N, C, H, W).abs() + 0.25, -(rn(N, C, H, W).abs() + 0.25)
    which = (torch.cumsum((~on).reshape(-1).long(), 0) % 3).reshape(N, C, H, W)        # the off positions cycle through the three
    off = torch.where(which == 0, torch.tensor(0.0), torch.where(which == 1, torch.tensor(-0.0), neg))    # planted +0.0, -0.0, negatives
    return {"x": rn(N, C, H, W), "w": rn(C, cin, k, k) * (cin * k * k) ** -0.5, "shift": rn(C), "gy": rn(N, C, Ho, Wo),
            "on": on, "mask": torch.where(on, pos, off)}


def channels(case):
    return case.kw["G"] * case.kw["gw"] if case.op == "gconv" else case.kw["C"]


# ---------------------------------------------------------------------------------------------------------------------------
# the formulas of csrc/i2v_params.h on packed operands, as a plain loop (float64; chain=True: the float32 fma chain)
# ---------------------------------------------------------------------------------------------------------------------------
def params_eval(src, w, cls, S, os_, out_hw, k, groups=None, chain=False, bleed=False):
    """dst[n][c][i os + oh0][j os + ow0] = sum over the class's slots (a, b), and for the grouped kernel over ci, of w * src[..][i S + a -
    pad][j S + b - pad], as I2VGConvParams / I2VDwConvParams state it.  src (N, C, Hs, Ws) numpy; w: [class][group][ci][3 a + b][co]
    (grouped, `groups` = (G, gw)) or [class][C][k a + b]; cls: rows (Hg, Wg, oh0, ow0, tapmask).  chain: float32 operands, every fma
    evaluated in float64 and rounded once, in the kernel's order (ci outer, slot inner; row-major slots).  bleed: a WRONG variant -- the
    zero rows between frames left out, frame n's padding rows hold its neighbours' edge rows."""
    N, C, Hs, Ws = src.shape
    pad, dt = k // 2, (np.float32 if chain else np.float64)
    sp = np.zeros((N, C, Hs + 2 * pad, Ws + 2 * pad), dt)
    sp[:, :, pad:pad + Hs, pad:pad + Ws] = src
    if bleed:
        r = min(pad, Hs)
        sp[1:, :, pad - r:pad, pad:pad + Ws] = src[:-1, :, Hs - r:, :]
        sp[:-1, :, pad + Hs:pad + Hs + r, pad:pad + Ws] = src[1:, :, :r, :]
    out = np.zeros((N, C) + tuple(out_hw), dt)
    w = np.asarray(w, dt)
    for ci_cls, (Hg, Wg, oh0, ow0, tm) in enumerate(cls):
        if Hg <= 0 or Wg <= 0:
            continue
        acc = np.zeros((N, C, Hg, Wg), dt)
        G, gw = groups if groups else (C, 1)
        accv = acc.reshape(N, G, gw, Hg, Wg)
        for ci in range(gw):
            for t in range(k * k):
                if not (tm >> t) & 1:
                    continue
                a, b = divmod(t, k)
                xs = sp[:, :, a:a + (Hg - 1) * S + 1:S, b:b + (Wg - 1) * S + 1:S].reshape(N, G, gw, Hg, Wg)[:, :, ci:ci + 1]
                wv = (w[ci_cls, :, ci, t, :] if groups else w[ci_cls, :, t][:, None])[None, :, :, None, None]
                if chain:
                    accv[...] = (wv.astype(np.float64) * xs.astype(np.float64) + accv.astype(np.float64)).astype(np.float32)
                else:
                    accv += wv * xs
        out[:, :, oh0:oh0 + (Hg - 1) * os_ + 1:os_, ow0:ow0 + (Wg - 1) * os_ + 1:os_] = acc
    return out


_host_capi = None


def host_capi():
    """A library that exports the packers: the host simulation (the CPU suite and the fixture writer)."""
    global _host_capi
    if _host_capi is None:
        from tests.hostsim_util import hostsim_engine
        _host_capi = hostsim_engine().capi
        lib.bind(_host_capi, lib.CONV_AUX_HOST_PROTOS)
    return _host_capi


@functools.lru_cache(maxsize=None)
def packed(case: Case):
    """(forward operand [1][...], gradient operand [classes][...], gradient classes (st^2, 5)) from the library's own packers."""
    kw, w = case.kw, inputs(case)["w"].contiguous()
    capi, st, H, W = host_capi(), kw["st"], kw["H"], kw["W"]
    cls = np.zeros((st * st, 5), np.int32)
    vp = lambda a: P(a.ctypes.data)
    if case.op == "gconv":
        G, gw = kw["G"], kw["gw"]
        fwd, bwd = np.full((1, G, gw, 9, gw), np.nan, np.float32), np.full((st * st, G, gw, 9, gw), np.nan, np.float32)
        lib.check(capi, capi.i2v_gconv_pack_f32(P(w.data_ptr()), G, gw, st, H, W, vp(fwd), vp(bwd), vp(cls)))
    else:
        C, k = kw["C"], kw["k"]
        fwd, bwd = w.numpy().reshape(1, C, k * k).copy(), np.full((st * st, C, k * k), np.nan, np.float32)
        lib.check(capi, capi.i2v_dwconv_pack_f32(P(w.data_ptr()), C, k, st, H, W, vp(bwd), vp(cls)))
    return fwd, bwd, [tuple(int(v) for v in row) for row in cls]


def conv_by_params(case, chain=False, bleed=False, swap_classes=False):
    """(forward pre-activation sum, gradient sum) of the case through `params_eval` on the packed operands, numpy."""
    kw, inp = case.kw, inputs(case)
    fwd, bwd, bcls = packed(case)
    k, st, H, W = (3 if case.op == "gconv" else kw["k"]), kw["st"], kw["H"], kw["W"]
    groups = (kw["G"], kw["gw"]) if case.op == "gconv" else None
    dt = np.float32 if chain else np.float64
    Ho, Wo = out_plane(H, st), out_plane(W, st)
    y = params_eval(inp["x"].numpy().astype(dt), fwd, [(Ho, Wo, 0, 0, (1 << (k * k)) - 1)], st, 1, (Ho, Wo), k, groups, chain, bleed)
    if swap_classes and st == 2:        # a WRONG variant: classes (0, 1) and (1, 0) read each other's operand and tap mask
        bwd = bwd[[0, 2, 1, 3]]
        bcls = [bcls[0], bcls[1][:4] + (bcls[2][4],), bcls[2][:4] + (bcls[1][4],), bcls[3]]
    dx = params_eval(inp["gy"].numpy().astype(dt), bwd, bcls, 1, st, (H, W), k, groups, chain, bleed)
    return y, dx


# ---------------------------------------------------------------------------------------------------------------------------
# references
# ---------------------------------------------------------------------------------------------------------------------------
def _slack_ref():
    return ("exact",)


def conv_eval(case, dt=torch.float64, route=None, frames=None, sums=None, transposed=False, last_col=False, next_group=False,
              shift_after_relu=False, mask_ge=False):
    """{name: (kind, ...)}.  sums: (y sum, dx sum) computed elsewhere (the chain, a wrong variant) in place of torch's convolution; the
    remaining switches are WRONG variants for tests/test_conv_aux_cpu.py."""
    kw, inp = case.kw, inputs(case)
    N = kw["N"] if frames is None else frames
    st, k = kw["st"], (3 if case.op == "gconv" else kw["k"])
    groups = kw["G"] if case.op == "gconv" else kw["C"]
    x, gy, shift = inp["x"][:N].to(dt), inp["gy"][:N].to(dt), inp["shift"].to(dt).view(1, -1, 1, 1)
    w64 = inp["w"].double()
    if sums is None:
        w = inp["w"].to(dt)
        if transposed:
            w = w.transpose(-1, -2)
        if next_group and case.op == "gconv":
            w = torch.roll(w.reshape(groups, -1), -1, 0).reshape(w.shape)
        xr = x.clone().requires_grad_(True)
        ysum = F.conv2d(xr, w, None, st, k // 2, 1, groups)
        dxsum = torch.autograd.grad(ysum, xr, gy)[0]
        ysum = ysum.detach()
    else:
        ysum, dxsum = (torch.from_numpy(np.ascontiguousarray(s))[:N].to(dt) for s in sums)
    # the scales: float64 pre-activation magnitudes per (frame, channel) plane, whatever `dt` and the switches are
    x64 = inp["x"][:N].double().requires_grad_(True)
    y64 = F.conv2d(x64, w64, None, st, k // 2, 1, groups)
    dx64 = torch.autograd.grad(y64, x64, inp["gy"][:N].double())[0]
    ypre64 = y64.detach() + (inp["shift"].double().view(1, -1, 1, 1) if kw["shift"] else 0)
    if shift_after_relu and kw["shift"] and kw["relu"]:
        y = torch.relu(ysum) + shift
    else:
        y = ysum + shift if kw["shift"] else ysum
        y = torch.relu(y) if kw["relu"] else y
    route = kw["bwd"] if route is None else route
    off = None
    if route != "none":
        on = inp["on"][:N] if not (mask_ge and route == "mask") else (inp["mask"][:N] >= 0)
        off = ~inp["on"][:N]
        dx = torch.where(on, dxsum, torch.zeros((), dtype=dt))
    else:
        dx = dxsum
    if last_col:
        y, dx = y.clone(), dx.clone()
        if y.shape[-1] > 1:
            y[..., -1] = y[..., -2]
        if dx.shape[-1] > 1:
            dx[..., -1] = dx[..., -2]
    out = {"y": ("planes", y, ypre64.abs().amax((2, 3)), None), "y_slack": _slack_ref(),
           "dx": ("planes", dx, dx64.abs().amax((2, 3)), off), "dx_slack": _slack_ref()}
    if kw["gout"]:
        out["ygate"] = ("gate", "y")
    return out


def se_eval(case, dt=torch.float64, frames=None, mean_short=False, ds_plain=False, h_ge=False):
    """The node in `dt`, written out (tests/test_conv_aux_cpu.py holds it against a literal SE module and autograd); the switches are
    WRONG variants."""
    kw, inp = case.kw, inputs(case)
    N = kw["N"] if frames is None else frames
    x, g, r = (inp[n][:N].to(dt) for n in ("x", "g", "r"))
    w1, b1, w2, b2 = (inp[n].to(dt) for n in ("w1", "b1", "w2", "b2"))
    HW = kw["HW"]
    m = x.sum(-1) / ((HW - 1) if mean_short else HW)
    h = torch.relu(m @ w1.t() + b1)
    s = torch.sigmoid(h @ w2.t() + b2)
    y = x * s.unsqueeze(-1) + (r if kw["res"] else 0)
    y = torch.relu(y) if kw["relu"] else y
    t = (g * x).sum(-1)
    dz2 = t * s if ds_plain else (t * s) * (1 - s)
    dh = dz2 @ w2
    dh = torch.where((h >= 0) if h_ge else (h > 0), dh, torch.zeros((), dtype=dt))
    dmh = (dh @ w1) / HW
    dx = g * s.unsqueeze(-1) + dmh.unsqueeze(-1)
    out = {}
    for name, v in (("m", m), ("h", h), ("s", s), ("t", t), ("dmh", dmh)):
        out[name] = ("planes", v, None, None)
        out[name + "_slack"] = _slack_ref()
    for name, v in (("y", y), ("dx", dx)):
        out[name] = ("planes", v, None, None)
        out[name + "_slack"] = _slack_ref()
    if kw["gout"]:
        out["ygate"] = ("gate", "y")
    return out


def evaluate(case: Case, dt=torch.float64, **how):
    return (se_eval if case.op == "se" else conv_eval)(case, dt, **how)


@functools.lru_cache(maxsize=None)
def reference(case: Case):
    return evaluate(case)


def error(got, want, scale=None):
    """The error of one `planes` output: the worst plane of max|got - want| / scale.  want (N, C, ...) with scale (N, C), or, scale None
    (SE), want (N, C, HW) per (frame, channel) and want (N, L) per frame, the scale the plane's max|want| (the tensor's where that is 0)."""
    got, want = got.double(), want.double()
    assert got.shape == want.shape, (tuple(got.shape), tuple(want.shape))
    if not bool(torch.isfinite(got).all()):
        return float("inf")
    lead = 2 if want.dim() > 2 else 1
    d = (got - want).abs().reshape(*want.shape[:lead], -1).amax(-1)
    if scale is None:
        scale = want.abs().reshape(*want.shape[:lead], -1).amax(-1)
        scale = torch.where(scale > 0, scale, want.abs().max())
    assert float(scale.min()) > 0
    return float((d / scale.double()).max())


def fp32_errors(case: Case):
    """{output: e32}: float32 CPU evaluations of the reference against float64, measured as the bound is.  Convolutions: the larger of
    float32 torch and the float32 fma chain of csrc/i2v_params.h."""
    r64 = reference(case)
    evals = [evaluate(case, torch.float32)]
    if case.op != "se":
        evals.append(conv_eval(case, torch.float32, sums=conv_by_params(case, chain=True)))
    return {n: max(error(e[n][1], r64[n][1], r64[n][2]) for e in evals) for n in VALUE[case.op]}


def gate_words(values, stride, rmw=False):
    """The gate allocation a launch that produced `values` (N, C, pixels) must leave: GFRONT sentinel words, C rows of `stride` words with
    bit n pixels + p of row c = (value > 0) in the first ceil(N pixels / 32) words, sentinel elsewhere."""
    N, C = values.shape[:2]
    bits = (values.reshape(N, C, -1) > 0).permute(1, 0, 2).reshape(C, -1).numpy()
    nb = bits.shape[1]
    nw = (nb + 31) // 32
    padded = np.zeros((C, nw * 32), bool)
    padded[:, :nb] = bits
    words = np.packbits(padded, axis=1, bitorder="little").view(np.uint32).reshape(C, nw).copy()
    if rmw and nb % 32:
        words[:, -1] |= np.uint32(SENT_BITS & 0xFFFFFFFF) & ~np.uint32((1 << (nb % 32)) - 1)
    full = np.full(GFRONT + C * stride + GTAIL, SENT_BITS & 0xFFFFFFFF, np.uint32)
    rows = full[GFRONT:GFRONT + C * stride].reshape(C, stride)
    rows[:, :nw] = words
    return torch.from_numpy(full.view(np.int32).copy())


def gate_stride(case, frames=None):
    kw = case.kw
    pixels = kw["HW"] if case.op == "se" else out_plane(kw["H"], kw["st"]) * out_plane(kw["W"], kw["st"])
    return ((kw["N"] if frames is None else frames) * pixels + 31) // 32 + 2           # two words past the last written one


def as_got(case, evaluated, frames=None):
    """What a kernel computing `evaluated` exactly would hand back."""
    got = {}
    for name, ref in evaluated.items():
        if ref[0] == "planes":
            got[name] = ref[1].to(torch.float32, copy=True)
    for name, ref in evaluated.items():
        if ref[0] == "exact":
            got[name] = torch.full((16,), SENTINEL)
        elif ref[0] == "gate":
            v = got[ref[1]]
            got[name] = gate_words(v.reshape(v.shape[0], v.shape[1], -1), gate_stride(case, frames))
    return got


def check(case: Case, got, e32, report=None, rmw=False, ref=None):
    """Hold every output of `got` to its bound; `e32`: this case's entry of the committed fixture.  Returns {output: error}."""
    ref = reference(case) if ref is None else ref
    assert set(got) == set(ref), (case.id, sorted(got), sorted(ref))
    assert set(e32) == set(VALUE[case.op]), (case.id, sorted(e32))
    errs = {}
    for name, r in ref.items():
        g = got[name]
        if r[0] == "exact":
            assert g.dtype == torch.float32 and bool((g.view(torch.int32) == SENT_BITS).all()), (
                f"{case.id}: {name}: {int((g.view(torch.int32) != SENT_BITS).sum())} of {g.numel()} float(s) outside the output changed")
        elif r[0] == "gate":
            v = got[r[1]]
            want = gate_words(v.reshape(v.shape[0], v.shape[1], -1), (g.numel() - GFRONT - GTAIL) // v.shape[1], rmw)
            assert g.shape == want.shape and bool(torch.equal(g, want)), (
                f"{case.id}: {name} differs from (the launch's own {r[1]} > 0) / zero high bits / sentinel at {int((g != want).sum())} of {g.numel()} word(s)")
        else:
            _, want, scale, off = r
            errs[name] = error(g, want, scale)
            if report is not None:
                report(f"{case.id:40s} {name:3s} error {errs[name]:.3g}  bound {bound(e32[name]):.3g}  (e32 {e32[name]:.3g})")
            if off is not None:
                assert bool((g[off].view(torch.int32) == 0).all()), f"{case.id}: {name} is not +0.0 at {int((g[off].view(torch.int32) != 0).sum())} position(s) whose gate is off"
    for name, err in errs.items():
        assert err <= bound(e32[name]), f"{case.id}: {name} error {err:.3g} > bound {bound(e32[name]):.3g} = max({FLOOR:g}, 4 * {e32[name]:.3g})"
    return errs


# ---------------------------------------------------------------------------------------------------------------------------
# running a case through the C entries
# ---------------------------------------------------------------------------------------------------------------------------
def _ctx(engine):
    cx = _Ctx(engine)
    if not getattr(cx.capi, "_conv_aux_bound", False):
        lib.bind(cx.capi, lib._CONV_AUX_PROTOS if hasattr(cx.capi, "i2v_gconv_f32") else lib.CONV_AUX_HOST_PROTOS)
        cx.capi._conv_aux_bound = True
    return cx


def _frames_idx(N, frame, nstride, off=0):
    return FRONT + off + (torch.arange(N).view(-1, 1) * nstride + torch.arange(frame).view(1, -1))


def _fin(cx, t, gap=0, off=0):
    """Input frames t (N, ...) at frame stride frame + gap, `off` floats past FRONT, NaN around and between them."""
    N, frame = t.shape[0], t[0].numel()
    return _Buf(cx, FRONT + off + N * (frame + gap) + 256, _frames_idx(N, frame, frame + gap, off), t, float("nan"))


def _fout(cx, N, frame, gap=0, off=0):
    return _Buf(cx, FRONT + off + N * (frame + gap) + 256, _frames_idx(N, frame, frame + gap, off), torch.full((N * frame,), float("nan")), SENTINEL)


class _Words:
    """An int32 allocation on the engine's device."""

    def __init__(self, cx, host):
        self.cx, self.dev = cx, (host.to(cx.eng.device) if cx.cuda else host.clone())

    def ptr(self, words=0):
        return P(self.dev.data_ptr() + 4 * words)

    def host(self):
        self.cx.sync()
        return self.dev.detach().cpu().clone()


def _gate_in(cx, on):
    """Gate rows for `on` (N, C, H, W) bool: bit n H W + pixel of row c; the unused bits of the last word, a spare word per row and the
    words around the rows are all ones."""
    N, C = on.shape[:2]
    bits = on.reshape(N, C, -1).permute(1, 0, 2).reshape(C, -1).numpy()
    nb = bits.shape[1]
    stride = (nb + 31) // 32 + 1
    padded = np.ones((C, stride * 32), bool)
    padded[:, :nb] = bits
    rows = np.packbits(padded, axis=1, bitorder="little").view(np.uint32).reshape(C, stride)
    full = np.full(GFRONT + C * stride + GTAIL, 0xFFFFFFFF, np.uint32)
    full[GFRONT:GFRONT + C * stride] = rows.reshape(-1)
    return _Words(cx, torch.from_numpy(full.view(np.int32).copy())), stride


def _gate_out(cx, C, stride):
    return _Words(cx, torch.full((GFRONT + C * stride + GTAIL,), SENT_BITS, dtype=torch.int32))


def conv_desc(case, **f):
    kw = case.kw
    d = lib.ConvAuxDesc()
    d.N, d.C, d.H, d.W, d.stride = kw["N"], channels(case), kw["H"], kw["W"], kw["st"]
    d.groups, d.k = kw.get("G", 0), kw.get("k", 3)
    for n, v in f.items():
        setattr(d, n, v)
    return d


def _run_conv(cx, case, inp, frames=None, route=None, src_off=0, sgap=None):
    kw = case.kw
    N, C, H, W, st = (kw["N"] if frames is None else frames), channels(case), kw["H"], kw["W"], kw["st"]
    Ho, Wo = out_plane(H, st), out_plane(W, st)
    gap, sgap = kw["gap"], kw["sgap"] if sgap is None else sgap
    route = kw["bwd"] if route is None else route
    entry = "i2v_gconv_f32" if case.op == "gconv" else "i2v_dwconv_f32"
    w = inp["w"].contiguous()
    out, plans = Result(), {}
    # forward
    x, y = _fin(cx, inp["x"][:N], sgap, src_off), _fout(cx, N, C * Ho * Wo, gap)
    shift = _fin(cx, inp["shift"].view(1, -1)) if kw["shift"] else None
    d = conv_desc(case, N=N, src=x.ptr(FRONT + src_off), src_nstride=C * H * W + sgap, dst=y.ptr(FRONT), dst_nstride=C * Ho * Wo + gap,
                  filter=w.data_ptr(), shift=shift.ptr(FRONT) if shift else None, relu=kw["relu"])
    yg = None
    if kw["gout"]:
        yg = _gate_out(cx, C, gate_stride(case, N))
        d.gate_out, d.gate_out_stride = yg.ptr(GFRONT), gate_stride(case, N)
    plan = lib.ConvAuxPlan()
    cx.call(entry, ctypes.byref(d), ctypes.byref(plan))
    plans["fwd"] = {n: getattr(plan, n) for n, _ in plan._fields_}
    y.collect(out, "y", (N, C, Ho, Wo))
    if yg is not None:
        out["ygate"] = yg.host()
    # input gradient
    gy, dx = _fin(cx, inp["gy"][:N], sgap, src_off), _fout(cx, N, C * H * W, gap)
    d = conv_desc(case, N=N, src=gy.ptr(FRONT + src_off), src_nstride=C * Ho * Wo + sgap, dst=dx.ptr(FRONT), dst_nstride=C * H * W + gap,
                  filter=w.data_ptr(), backward=1)
    keep = None
    if route == "gate":
        keep, d.gate_stride = _gate_in(cx, inp["on"][:N])
        d.gate = keep.ptr(GFRONT)
    elif route == "mask":
        keep = _fin(cx, inp["mask"][:N], 5)
        d.mask, d.mask_nstride = keep.ptr(FRONT), C * H * W + 5
    cx.call(entry, ctypes.byref(d), ctypes.byref(plan))
    plans["bwd"] = {n: getattr(plan, n) for n, _ in plan._fields_}
    dx.collect(out, "dx", (N, C, H, W))
    out.plans = plans
    return out


def se_desc(case, **f):
    kw = case.kw
    d = lib.SeLaunchDesc()
    d.N, d.C, d.rd, d.HW = kw["N"], kw["C"], kw["rd"], kw["HW"]
    for n, v in f.items():
        setattr(d, n, v)
    return d


def _run_se(cx, case, inp, frames=None, mis=None):
    kw = case.kw
    N, C, rd, HW, gap = (kw["N"] if frames is None else frames), kw["C"], kw["rd"], kw["HW"], kw["gap"]
    o = lambda n: 1 if mis == n else 0
    x, g, r = (_fin(cx, inp[n][:N], gap, o(n)) for n in ("x", "g", "r"))
    y, dx = _fout(cx, N, C * HW, gap, o("dst")), _fout(cx, N, C * HW, gap, o("dst"))
    vec = {n: _fout(cx, 1, N * (rd if n == "h" else C)) for n in ("m", "h", "s", "t", "dmh")}
    w = [inp[n].contiguous() for n in ("w1", "b1", "w2", "b2")]
    common = dict(N=N, x=x.ptr(FRONT + o("x")), x_nstride=C * HW + gap, w1=w[0].data_ptr(), b1=w[1].data_ptr(), w2=w[2].data_ptr(), b2=w[3].data_ptr(),
                  **{n: b.ptr(FRONT) for n, b in vec.items()})
    d = se_desc(case, dst=y.ptr(FRONT + o("dst")), dst_nstride=C * HW + gap, relu=kw["relu"], **common)
    if kw["res"]:
        d.r, d.r_nstride = r.ptr(FRONT + o("r")), C * HW + gap
    yg = None
    if kw["gout"]:
        yg = _gate_out(cx, C, gate_stride(case, N))
        d.gate_out, d.gate_out_stride = yg.ptr(GFRONT), gate_stride(case, N)
    cx.call("i2v_se_f32", ctypes.byref(d))
    d = se_desc(case, g=g.ptr(FRONT + o("g")), g_nstride=C * HW + gap, dst=dx.ptr(FRONT + o("dst")), dst_nstride=C * HW + gap, backward=1, **common)
    cx.call("i2v_se_f32", ctypes.byref(d))
    out = Result()
    for n, b in vec.items():
        b.collect(out, n, (N, rd if n == "h" else C))
    y.collect(out, "y", (N, C, HW))
    dx.collect(out, "dx", (N, C, HW))
    if yg is not None:
        out["ygate"] = yg.host()
    return out


def run(engine, case: Case, **how):
    """The case through the C entries of `engine.capi`: {name: CPU tensor} over the names of `reference(case)`.  frames = k: the first k
    frames as a call of their own.  Convolutions: route = "gate" | "mask" | "none" (the gradient's gate), src_off = 1 (the sources one
    float off 16-byte alignment), sgap (the sources' frame stride minus the frame).  SE: mis = "x" | "g" | "r" | "dst" (that operand one
    float off)."""
    return (_run_se if case.op == "se" else _run_conv)(_ctx(engine), case, inputs(case), **how)


# ---------------------------------------------------------------------------------------------------------------------------
# N = 0 and the refusals (device): (label, entry, launch named in the message, thunk returning the status)
# ---------------------------------------------------------------------------------------------------------------------------
STATS = {"i2v_gconv_f32": b"gconv_launches", "i2v_dwconv_f32": b"dwconv_launches", "i2v_se_f32": b"se_launches"}


def refusals(engine):
    cx = _ctx(engine)
    capi, s, dev = cx.capi, cx.eng.stream, cx.eng.device
    zeros = lambda n: torch.zeros(n + 8, device=dev)
    sents = lambda n: torch.full((n + 8,), SENTINEL, device=dev)
    p = lambda t, off=0: t.data_ptr() + 4 * off
    # conv operands big enough for every thunk below: nothing is launched, no thunk depends on their contents
    src, dst, gate = zeros(1 << 16), sents(1 << 16), sents(1 << 12)
    filt = torch.zeros(64 * 64 * 25)
    plan = lib.ConvAuxPlan()

    def conv(entry, **f):
        base = dict(src=p(src), src_nstride=1 << 14, dst=p(dst), dst_nstride=1 << 14, filter=filt.data_ptr(), N=1, C=8, H=6, W=8, stride=1, groups=2, k=3)
        base.update(f)
        d = lib.ConvAuxDesc()
        for n, v in base.items():
            setattr(d, n, v)
        return lambda: getattr(capi, entry)(ctypes.byref(d), ctypes.byref(plan), s())
    G, D = "i2v_gconv_f32", "i2v_dwconv_f32"
    thunks = [
        ("gw 12", G, "k_gconv_plan", conv(G, C=24, groups=2)),
        ("gate_out on a strided-output gradient launch", G, "k_gconv", conv(G, backward=1, stride=2, gate_out=p(gate), gate_out_stride=4)),
        ("gw 64 on 2 x 130: 202 752 B", G, "k_gconv_plan", conv(G, C=128, groups=2, H=2, W=130)),
        ("gw 64 / stride 2 / 3 x 3 gradient plane: 261 120 B", G, "k_gconv_plan", conv(G, C=128, groups=2, H=3, W=3, stride=2, backward=1)),
        ("gw 64 / stride 2 / 2 x 2 forward source: 261 120 B", G, "k_gconv_plan", conv(G, C=128, groups=2, H=2, W=2, stride=2)),
        ("k 4", D, "k_dwconv_plan", conv(D, k=4)), ("k 7", D, "k_dwconv_plan", conv(D, k=7)),
        ("stride 3", D, "k_dwconv_plan", conv(D, stride=3)),
        ("1 x 3300 at k 5: 132 320 B", D, "k_dwconv_plan", conv(D, C=2, k=5, H=1, W=3300)),
        ("gate_out on a strided-output gradient launch", D, "k_dwconv", conv(D, backward=1, stride=2, gate_out=p(gate), gate_out_stride=4)),
        ("planned for an aligned source, launched one float off", D, "k_dwconv", conv(D, plan_src=p(src), src=p(src, 1))),
    ]
    # SE
    x, sedst, vec = zeros(1 << 17), sents(1 << 17), sents(1 << 17)
    hw = torch.zeros(8193 * 4)

    def se(**f):
        base = dict(x=p(x), x_nstride=64, g=p(x), g_nstride=64, dst=p(sedst), dst_nstride=64, w1=hw.data_ptr(), b1=hw.data_ptr(), w2=hw.data_ptr(),
                    b2=hw.data_ptr(), m=p(vec), h=p(vec), s=p(vec), t=p(vec), dmh=p(vec), N=2, C=4, rd=2, HW=16)
        base.update(f)
        d = lib.SeLaunchDesc()
        for n, v in base.items():
            setattr(d, n, v)
        return lambda: capi.i2v_se_f32(ctypes.byref(d), s())
    E = "i2v_se_f32"
    thunks += [
        ("rd 8193", E, "k_se_excite", se(rd=8193, launches=2)),
        ("gate_out without ReLU", E, "k_se_scale", se(gate_out=p(gate), gate_out_stride=4, launches=4)),
        ("backward with ReLU", E, "k_se_scale", se(backward=1, relu=1, launches=4)),
        ("C 0", E, "k_se_plan", se(C=0)), ("HW 0", E, "k_se_plan", se(HW=0)),
        ("65 536 frames on the squeeze", E, "k_se_squeeze", se(N=65536, C=1, HW=1, x_nstride=1, launches=1)),
    ]

    def untouched():
        cx.sync()
        return all(bool((t == SENTINEL).all()) for t in (dst, gate, sedst, vec))
    return thunks, untouched, (src, dst, gate, filt, x, sedst, vec, hw)


def run_empty(engine):
    """N = 0 on each entry: [(entry, status, launch counter before, after)] and `untouched()`."""
    cx = _ctx(engine)
    capi, s, dev = cx.capi, cx.eng.stream, cx.eng.device
    src, dst, vec = torch.zeros(4096, device=dev), torch.full((4096,), SENTINEL, device=dev), torch.full((4096,), SENTINEL, device=dev)
    filt, p = torch.zeros(4096), (lambda t: t.data_ptr())
    rows, plan = [], lib.ConvAuxPlan()
    for entry in ("i2v_gconv_f32", "i2v_dwconv_f32"):
        d = lib.ConvAuxDesc()
        for n, v in dict(src=p(src), src_nstride=512, dst=p(dst), dst_nstride=512, filter=p(filt), N=0, C=8, H=6, W=8, stride=1, groups=2, k=3,
                         shift=p(src), relu=1, gate_out=p(vec), gate_out_stride=4).items():
            setattr(d, n, v)
        before = capi.i2v_backend_stat(STATS[entry])
        rows.append((entry, getattr(capi, entry)(ctypes.byref(d), ctypes.byref(plan), s()), before, capi.i2v_backend_stat(STATS[entry])))
    for backward in (0, 1):
        d = lib.SeLaunchDesc()
        for n, v in dict(x=p(src), x_nstride=64, g=p(src), g_nstride=64, dst=p(dst), dst_nstride=64, w1=p(filt), b1=p(filt), w2=p(filt), b2=p(filt),
                         m=p(vec), h=p(vec), s=p(vec), t=p(vec), dmh=p(vec), N=0, C=4, rd=2, HW=16, backward=backward).items():
            setattr(d, n, v)
        before = capi.i2v_backend_stat(STATS["i2v_se_f32"])
        rows.append(("i2v_se_f32", capi.i2v_se_f32(ctypes.byref(d), s()), before, capi.i2v_backend_stat(STATS["i2v_se_f32"])))

    def untouched():
        cx.sync()
        return bool((dst == SENTINEL).all()) and bool((vec == SENTINEL).all())
    return rows, untouched
