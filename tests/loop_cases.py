"""TEST INFRASTRUCTURE: the case table of the loop kernels -- the loss, step and gradient-shaping launches behind
csrc/i2v_loop_api.cpp (csrc/i2v_kernels.hip: `cos_*`, `std_*`, `ilaf_*`, `head_*`, `grad_post_*`, `tap_*`, `aens_*`, `dwconv1d`,
`resample_nearest*`, `tt_grad_mix`, `compose`) -- with their input generators and a float64 reference per entry.
tests/test_loop_kernels_cpu.py runs the table on the host simulation, tests/test_gpu_loop_kernels.py on the device.

`run(engine, case)` calls the C entries through `engine.capi` with buffers on the engine's device and returns {name: CPU tensor}.
`reference(case)` returns {name: (kind, float64 or exact tensor)} over the SAME names: nothing an entry writes is left unchecked.

Kinds and bounds (`check`):
  tensor   max|got - want| <= max(2e-6, 4 e32) * max|want|          (2e-6: test_cossim_fwd_bwd's gradient bound)
  cos      max|got - want| <= max(2e-7, 4 e32)                      (2e-7 absolute: test_cossim_fwd_bwd's cosine bound)
  scalar   |got - want| <= max(1e-5, 4 e32) * |want|, element by element   (1e-5 relative: test_ilaf_kernels' loss bound)
  exact    equal bits (data movement, selection, untouched slack, gated zeros)
e32 is the error of the same reference evaluated in float32 by plain torch on the CPU, normalised the same way and committed as
tests/golden/loop_fp32_cpu_errors.json (tests/make_loop_fixtures.py); the factor 4 is DESIGN.md section 14's.  With `accumulate`
the wanted tensor is base + reference, so max|want| is max|base + ref|: the fp32 add of a base of order one to a gradient of order
1e-3 rounds at the base's size.

Buffers: every strided operand (`a`, `b`, `grad`) is a view into a larger allocation, `off` floats in (off = 1: the base is
misaligned by 4 bytes) with row stride D + pad.  The slack of `grad` -- the floats ahead of the view and the columns [D, stride) -- is
pre-filled with SENTINEL and must come back unchanged; its interior starts as NaN (or as a random base when accumulating), so an
element no thread wrote fails the comparison.

Branch arithmetic (re-derive the comments at the cases when any of it changes):
  cos_nblk(D) = clamp(D // 4096, 1, 64) blocks per frame in every `*_reduce`; the cosine chunk is ceil(D / nblk) rounded UP to a
  multiple of 4, the std / ILAF chunk is ceil(D / nblk) as it is.  The elementwise gradient launches use min(ceil(D / 2048), 64)
  blocks of 256 threads: a grid-stride second pass from D = 64 * 256 + 1, and all 64 blocks from D = 129025.
  stream_grid(total, per) = clamp(ceil(total / per), 1, 4096) blocks of 256 threads; per = 1024 for the elementwise launches, so the
  cap binds from 4 194 305 elements.  grad_post splits a group over ceil(elements / 65536) blocks; tap_sign_abs keeps at most 1024
  partials (stream_grid(n, 4096) capped): 2 blocks from n = 4097, the cap from n = 4096 * 1024 + 1.
  head_logits_kernel: 256 threads over K (a second trip from K = 257; with K < 64 the max / sum trees run on padding).
  cos_reduce_kernel takes the 16-byte path when both strides are multiples of 4 AND both bases are 16-byte aligned.
"""
import ctypes
import functools
import zlib
from dataclasses import dataclass
from typing import Tuple

import numpy as np
import torch
import torch.nn.functional as F

from i2v_amd import lib
from oracle import restate

SENTINEL = -123.25
FLOOR = {"tensor": 2e-6, "cos": 2e-7, "scalar": 1e-5}
P = ctypes.c_void_p
NULL = P(0)


@dataclass(frozen=True)
class Case:
    id: str
    op: str
    items: Tuple[Tuple[str, object], ...]
    host_bits: bool = True          # the device's bits equal the host simulation's
    why_not: str = ""               # ... or the one-line reason they need not

    @property
    def kw(self):
        return dict(self.items)


def _case(op, id, host_bits=True, why_not="", **kw):
    return Case(f"{op}-{id}", op, tuple(sorted(kw.items())), host_bits, why_not)


FLAGS = ((1, 0), (0, 0), (1, 1), (0, 1))        # (mask_relu, accumulate)


def _fl(m, a):
    return f"m{m}a{a}"


# ---------------------------------------------------------------------------------------------------------------------------
# the table
# ---------------------------------------------------------------------------------------------------------------------------
def _cos_cases():
    out = []
    # D: nblk 1 (1, 3, 37, 4095, 4096, 8191), 2 (8192: chunk 4096; 8193: chunk 4097 -> 4100, D % 4 = 1; 8197: chunk 4099 -> 4100, the second
    # block's 4097 elements end in a scalar tail), 64 (262151: chunk 4097 -> 4100, the last block holds 3851; cos_grad's 64-block cap
    # makes 17 grid-stride passes).  pad and flags cycle over the sizes.
    for i, (D, frames) in enumerate([(1, 5), (3, 6), (37, 2), (4095, 3), (4096, 2), (8191, 2), (8192, 3), (8193, 2), (8197, 4), (262151, 2)]):
        m, a = FLAGS[(i + 3) % 4]        # (D = 1 accumulates, unmasked: its gradient is 0 in exact arithmetic, only base + gradient has a scale)
        out.append(_case("cos", f"D{D}-pad{i % 4}-{_fl(m, a)}", D=D, frames=frames, pad=i % 4, off=0, mask=m, acc=a, coef=bool(i & 1), zero_row=-1))
    # stride: pad 0 with an aligned base is the 16-byte path, pads 1..3 the scalar branch by stride, pad 0 one float in the scalar branch
    # by base; at 37 (one block, tail only) and 8197 (two blocks, 16-byte body + scalar tail in both)
    for D, frames in ((37, 3), (8197, 2)):
        for pad, off in ((0, 0), (1, 0), (2, 0), (3, 0), (0, 1), (4, 0), (4, 1)):
            out.append(_case("cos", f"D{D}-pad{pad}-off{off}", D=D, frames=frames, pad=pad, off=off, mask=1, acc=0, coef=False, zero_row=-1))
    for m, a in FLAGS:
        for coef in (False, True):
            out.append(_case("cos", f"D8193-{_fl(m, a)}-coef{int(coef)}", D=8193, frames=3, pad=3, off=0, mask=m, acc=a, coef=coef, zero_row=-1))
    # a frame whose `a` row is all zero: the 1e-8 clamp of the norm; cos = 0 and the gradient b / (1e-8 |b|)
    out.append(_case("cos", "zero-row", D=37, frames=3, pad=3, off=0, mask=0, acc=0, coef=False, zero_row=1))
    out.append(_case("cos", "zero-row-acc", D=4100, frames=2, pad=0, off=0, mask=0, acc=1, coef=True, zero_row=0))
    return out


def _std_cases():
    out = []
    # D: 1 with 2 frames (the smallest total_count the entry takes), 5, 37 (one block), 8197 (2 blocks of 4099 and 4098: no rounding of
    # the chunk), 262151 (64 blocks of 4097, the last of 4040; 17 passes of the gradient's grid-stride loop)
    for i, (D, frames) in enumerate([(1, 2), (5, 3), (37, 6), (8197, 4), (262151, 2)]):
        for pad in (0, 3):
            for m, a in FLAGS:
                out.append(_case("std", f"D{D}-f{frames}-pad{pad}-{_fl(m, a)}", D=D, frames=frames, pad=pad, off=0, mask=m, acc=a, how="fused"))
    # the two-call form with total_count = frames * D, and the sharded form: the sums of a second shard are added to the first's between
    # the calls, total_count counts both (Net.stdloss's `exchange`)
    for D, frames in ((37, 3), (8197, 2)):
        out.append(_case("std", f"D{D}-split", D=D, frames=frames, pad=3, off=1, mask=1, acc=0, how="split"))
        out.append(_case("std", f"D{D}-two-shards", D=D, frames=frames, pad=3, off=0, mask=1, acc=1, how="shards"))
    return out


ILAF_SHAPES = ((5, 3, 1), (37, 6, 2), (8197, 4, 4), (8197, 6, 3))       # (D, frames, frames per segment)


def _ilaf_cases():
    out = []
    for i, (D, frames, fps) in enumerate(ILAF_SHAPES):
        for pad in (0, 3):
            for m, a in FLAGS if D == 37 else (FLAGS[(i + pad) % 4], FLAGS[(i + pad + 2) % 4]):
                out.append(_case("ilaf", f"D{D}-f{frames}-seg{fps}-pad{pad}-{_fl(m, a)}", D=D, frames=frames, fps=fps, pad=pad, off=0, mask=m, acc=a, one=False))
    # the one-clip entries (host-side initial norm)
    out.append(_case("ilaf", "D37-f6-one-clip", D=37, frames=6, fps=6, pad=3, off=1, mask=1, acc=0, one=True))
    out.append(_case("ilaf", "D8197-f4-one-clip", D=8197, frames=4, fps=4, pad=0, off=0, mask=0, acc=1, one=True))
    return out


def _tapd_cases():
    out = []
    for i, (D, frames, fps) in enumerate(ILAF_SHAPES):
        for pad in (0, 3):
            for m, a in FLAGS if D == 37 else (FLAGS[(i + pad) % 4], FLAGS[(i + pad + 2) % 4]):
                out.append(_case("tapd", f"D{D}-f{frames}-seg{fps}-pad{pad}-{_fl(m, a)}", D=D, frames=frames, fps=fps, pad=pad, off=0, mask=m, acc=a))
    return out


# (C1, HW1, C2, HW2, T, clips, K): K = 300 and 257 take a second trip of the 256-thread loops over K (257: one class in it), K = 2 runs
# the 64-lane max / sum trees on 62 padding lanes; C1 = 300 a second trip of the loop over Ctot; HW = 1 a pool over T alone
HEAD_SHAPES = ((5, 9, 3, 4, 2, 3, 300), (7, 1, 2, 49, 1, 1, 2), (300, 3, 1, 1, 3, 2, 257))


def _head_cases():
    out = []
    for si, shp in enumerate(HEAD_SHAPES):
        combos = [(bias, pad, m, a) for bias in (True, False) for pad in (0, 1, 3) for m, a in FLAGS]
        if si != 1:                                        # every combination at the smallest shape, a cycle through them at the others
            combos = [c for j, c in enumerate(combos) if j % 5 == si]
        for bias, pad, m, a in combos:
            out.append(_case("head", f"s{si}-bias{int(bias)}-pad{pad}-{_fl(m, a)}", shape=shp, bias=bias, pad=pad, off=0, mask=m, acc=a, fused=False))
    for si, shp in enumerate(HEAD_SHAPES):                 # the fused single-feature entry
        for j, (m, a) in enumerate(FLAGS):
            out.append(_case("head", f"fused-s{si}-{_fl(m, a)}", shape=shp, bias=bool((si + j) & 1), pad=(1, 3, 0, 1)[j], off=0, mask=m, acc=a, fused=True))
    return out


GP_MODES = (0, 1, 2, 3, 4)          # none, frame, clip, column, l1


def _gp_cases():
    out = []
    # (2,3,2,150,150): frame groups of 67 500 elements -> 2 splits, clip groups of 135 000 -> 3, l1 270 000 -> 5, column 900 -> 1
    for shape in ((1, 3, 1, 1, 1), (2, 3, 3, 5, 7), (2, 3, 2, 150, 150)):
        for mode in GP_MODES:
            for fm in (0, 1):
                for mom in (0, 1):
                    out.append(_case("gp", "x".join(map(str, shape)) + f"-mode{mode}-fm{fm}-mom{mom}", shape=shape, mode=mode, fm=fm, mom=mom))
    # 4 816 896 elements: 4704 blocks' worth > the 4096-block cap, so the apply launch makes a second grid-stride pass; 74 splits
    out.append(_case("gp", "1x3x32x224x224-mode2-fm1-mom1", shape=(1, 3, 32, 224, 224), mode=2, fm=1, mom=1))
    return out


def _misc_cases():
    out = []
    for shape in ((2, 3, 3, 5, 7), (1, 3, 1, 1, 1)):
        out.append(_case("tap_perts", "x".join(map(str, shape)), shape=shape))
        out.append(_case("tap_grad", "x".join(map(str, shape)), shape=shape))
    # n: 1 block (1), 2 blocks (4097, 5000), the 1024-partial cap with a grid-stride pass (4096 * 1024 + 5)
    for n in (1, 4097, 5000, 4096 * 1024 + 5):
        out.append(_case("tap_sign", f"n{n}", n=n))
    # one 64-lane wave per row: frames 1, 63 (a lane idle), 65 (a second trip), 100
    for L, frames in ((1, 1), (6, 100), (64, 63), (64, 65)):
        out.append(_case("aens_reduce", f"L{L}-f{frames}", L=L, frames=frames))
    why = "the scalar twin sums its fp32 softmax in index order with glibc's expf, the one-wave kernel as an xor butterfly with the device's"
    for L, same in ((1, False), (6, False), (64, False), (6, True)):
        out.append(_case("aens_coeffs", f"L{L}" + ("-equal-prev" if same else ""), host_bits=False, why_not=why, L=L, same=same))
    # len 3 < k = 15 (every window hangs over both ends), k = 1, k = 15 along a middle axis, k = 5 along the frame axis
    for shape, axis, k in (((2, 3, 3, 4, 5), 2, 15), ((1, 1, 1, 1, 7), 4, 1), ((2, 3, 4, 6, 5), 3, 15), ((2, 3, 20, 3, 3), 2, 5)):
        out.append(_case("dwconv", "x".join(map(str, shape)) + f"-axis{axis}-k{k}", shape=shape, axis=axis, k=k))
    out.append(_case("resample", "5x7-to-7x9"))
    for D in (1, 3, 64):
        for w in (0.0, 0.3, 1.0):
            out.append(_case("ttmix", f"D{D}-w{w}", D=D, w=w))
    for vl in (0, 1):
        out.append(_case("compose", f"layout{vl}", video_layout=vl))
    return out


CASES = tuple(_cos_cases() + _std_cases() + _ilaf_cases() + _tapd_cases() + _head_cases() + _gp_cases() + _misc_cases())
BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES)


# ---------------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------------
def _gen(case, salt=0):
    return torch.Generator().manual_seed(zlib.crc32(case.id.encode()) + salt)


def _signed(t):
    """Few elements: alternate the signs, so that a ReLU mask gates about half of them whatever the seed."""
    if t.numel() < 64:
        f = t.abs().flatten()
        f[1::2] *= -1
        return f.view_as(t).contiguous()
    return t


def _act_inputs(case, rows, D, extra=()):
    """`a` (rows, D) with both signs, a random accumulate base, and the named further (rows, D) tensors."""
    g = _gen(case)
    inp = {"a": _signed(torch.randn(rows, D, generator=g)), "base": torch.randn(rows, D, generator=g)}
    for name, noise in extra:
        inp[name] = (inp["a"] + noise * torch.randn(rows, D, generator=g)).contiguous()
    return inp


@functools.lru_cache(maxsize=4)
def inputs(case: Case):
    kw, g = case.kw, _gen(case)
    op = case.op
    if op == "cos":
        inp = _act_inputs(case, kw["frames"], kw["D"], (("b", 0.5),))
        if kw["zero_row"] >= 0:
            inp["a"][kw["zero_row"]] = 0.0
        inp["coef"] = torch.tensor([3.0, 0.7, -2.0])
        return inp
    if op == "std":
        inp = _act_inputs(case, kw["frames"], kw["D"])
        inp["other"] = torch.randn(kw["frames"] + 1, kw["D"], generator=g) * 2.0 + 0.5       # the second shard ("shards")
        return inp
    if op == "ilaf":
        return _act_inputs(case, kw["frames"], kw["D"], (("ori", 0.3), ("adv0", 0.2)))
    if op == "tapd":
        inp = _act_inputs(case, kw["frames"], kw["D"], (("clean", 0.3),))
        a = inp["a"].flatten()
        a[::5] = 0.0                                        # exact zeros (gradient 0), next to the negatives `_act_inputs` gives
        a[2::7] = -a[2::7].abs()
        inp["a"] = a.view(kw["frames"], kw["D"]).contiguous()
        inp["clean"].flatten()[3::11] = 0.0
        return inp
    if op == "head":
        C1, HW1, C2, HW2, T, clips, K = kw["shape"]
        Ctot = C1 if kw["fused"] else C1 + C2
        inp = {"a1": _signed(torch.randn(clips * T, C1 * HW1, generator=g)), "base1": torch.randn(clips * T, C1 * HW1, generator=g),
               "a2": _signed(torch.randn(clips * T, C2 * HW2, generator=g)), "base2": torch.randn(clips * T, C2 * HW2, generator=g),
               "W": torch.randn(K, Ctot, generator=g), "bias": 2.0 * torch.randn(K, generator=g)}
        lab = [0, K - 1, K // 2]
        if clips == 1:
            lab = [K - 1] if kw["mask"] else [0]
        inp["labels"] = torch.tensor(lab[:clips], dtype=torch.int32)
        return inp
    if op == "gp":
        b, c, f, h, w = kw["shape"]
        shp = (b, f, c, h, w) if kw["fm"] else (b, c, f, h, w)
        return {"g": torch.randn(shp, generator=g), "mom": torch.randn(b, c, f, h, w, generator=g) * 2.0}
    if op == "tap_perts":
        return {"adv": torch.randn(kw["shape"], generator=g), "vid": torch.randn(kw["shape"], generator=g)}
    if op == "tap_grad":
        b, c, f, h, w = kw["shape"]
        return {"gx": torch.randn(b, f, c, h, w, generator=g), "bs": torch.randn(b, c, f, h, w, generator=g).sign()}
    if op == "tap_sign":
        x = torch.randn(kw["n"], generator=g)
        x[3::3] = 0.0
        x[6::6] = -0.0
        return {"x": x}
    if op == "aens_reduce":
        return {"cos": torch.rand(kw["L"], kw["frames"], generator=g) * 2 - 1, "coeffs": torch.softmax(torch.randn(kw["L"], generator=g), 0)}
    if op == "aens_coeffs":
        prev = torch.full((kw["L"],), 3.5) if kw["same"] else 3.0 + torch.rand(kw["L"], generator=g)
        return {"prev": prev, "coeffs": torch.softmax(torch.randn(kw["L"], generator=g), 0)}
    if op == "dwconv":
        return {"x": torch.randn(kw["shape"], generator=g), "taps": torch.rand(kw["k"], generator=g) + 0.1 * torch.arange(kw["k"])}      # asymmetric
    if op == "resample":
        # monotone maps with padding (-1) at both ends and repeats; source rows 1 and 4 and columns 2, 3 and 5 are read by nothing
        my, mx = [-1, 0, 0, 2, 3, 3, -1], [-1, -1, 0, 1, 1, 1, 4, 6, -1]
        return {"x": torch.randn(2, 3, 5, 7, generator=g), "g": torch.randn(2, 3, 7, 9, generator=g),
                "my": torch.tensor(my, dtype=torch.int32), "mx": torch.tensor(mx, dtype=torch.int32)}
    if op == "ttmix":
        D, T = kw["D"], 5
        mv = torch.randint(-2 * T - 1, 2 * T + 2, (D,), generator=g, dtype=torch.int32)
        mv[0] = -7                                          # negative and |move| > T whatever the seed
        if D > 2:
            mv[1], mv[2] = 6, -1
        return {"g": torch.randn(D, 2, 3, T, 3, 3, generator=g), "k": torch.rand(D, generator=g) + 0.05, "moves": mv}
    if op == "compose":
        b, f, h, w = 2, 3, 5, 7
        eps = 16 / 255
        u = torch.rand(b * f, 3, h, w, generator=g)
        d = (torch.rand(b * f, 3, h, w, generator=g) - 0.5) * 0.2        # a good part beyond +-eps
        e32 = float(np.float32(eps))
        d[0, 0, 0, :4] = torch.tensor([e32, -e32, e32, -e32])            # delta exactly +-eps
        u[1, 1, 1, :2], d[1, 1, 1, :2] = 0.96875, 0.03125               # u + delta exactly 1
        u[2, 2, 2, :2], d[2, 2, 2, :2] = 0.03125, -0.03125              # ... exactly 0
        u[3, 0, 3, :2], d[3, 0, 3, :2] = 0.99, 0.05                     # beyond 1
        u[4, 1, 4, :2], d[4, 1, 4, :2] = 0.01, -0.05                    # below 0
        return {"u": u, "d": d, "eps": eps, "bf": (b, f)}
    raise KeyError(op)


# ---------------------------------------------------------------------------------------------------------------------------
# float64 (or, for the committed fixture, float32) references: plain torch and autograd
# ---------------------------------------------------------------------------------------------------------------------------
def _finish_grad(out, name, r, a, base, kw, mask=None):
    """Gate the raw gradient by a > 0 afterwards, add the base, and say what the slack and the gated elements must hold."""
    mask = kw["mask"] if mask is None else mask
    gate = ~(a > 0)
    if mask:
        r = r * (a > 0)
    out[name] = ("tensor", base.to(r.dtype) + r if kw["acc"] else r)
    pad_elems = a.shape[0] * kw["pad"] + kw["off"]
    out[name + "_x_slack"] = ("exact", torch.full((pad_elems,), SENTINEL))
    if kw["mask"]:
        out[name + "_x_gated"] = ("exact", base[gate] if kw["acc"] else torch.zeros(int(gate.sum())))


def _ref_cos(kw, inp, dt, drop):
    a, b = inp["a"].to(dt), inp["b"].to(dt)
    cos, grad = restate.cosine_fwd_bwd(a, b)
    coef = 0.5 * (float(inp["coef"][1]) if kw["coef"] else 1.0)
    out = {"cos": ("cos", cos)}
    _finish_grad(out, "grad", coef * grad, inp["a"], inp["base"], kw, mask=0 if drop == "mask" else None)
    return out


def _ref_std(kw, inp, dt, drop):
    a = inp["a"].to(dt).requires_grad_(True)
    x = torch.cat([a, inp["other"].to(dt)]) if kw["how"] == "shards" else a
    s = x.std()
    g, = torch.autograd.grad(s, a)
    out = {"std": ("scalar", s.detach().reshape(1))}
    _finish_grad(out, "grad", g, inp["a"], inp["base"], kw, mask=0 if drop == "mask" else None)
    return out


def _ref_ilaf(kw, inp, dt, drop):
    fps = kw["frames"] if drop == "segments" else kw["fps"]
    a = inp["a"].to(dt).requires_grad_(True)
    ori, adv0 = inp["ori"].to(dt), inp["adv0"].to(dt)
    D = kw["D"]
    d, d0 = (a - ori).view(-1, fps * D), (adv0 - ori).view(-1, fps * D)
    n, n0 = d.norm(dim=1), d0.norm(dim=1)
    loss = -(0.5 * n / n0 + ((d0 / n0[:, None]) * (d / n[:, None])).sum(1))
    g, = torch.autograd.grad(loss.sum(), a)
    out = {"loss": ("scalar", loss.detach())} if drop != "segments" else {}
    _finish_grad(out, "grad", g, inp["a"], inp["base"], kw, mask=0 if drop == "mask" else None)
    return out


def _ref_tapd(kw, inp, dt, drop):
    fps = kw["frames"] if drop == "segments" else kw["fps"]
    a = inp["a"].to(dt).requires_grad_(True)
    clean = inp["clean"].to(dt)

    def r(x):
        return x.sign() * x.abs().sqrt()
    dist = (r(a) - r(clean)).view(-1, fps * kw["D"]).norm(dim=1)
    g, = torch.autograd.grad(0.7 * dist.sum(), a)
    g = torch.where(inp["a"] == 0, torch.zeros_like(g), g)           # (sqrt's derivative at 0 is infinite: the gradient there is 0 by rule)
    out = {"dist": ("scalar", dist.detach())} if drop != "segments" else {}
    _finish_grad(out, "grad", g, inp["a"], inp["base"], kw, mask=0 if drop == "mask" else None)
    return out


HEAD_SCALE = 1.7


def _ref_head(kw, inp, dt, drop):
    C1, HW1, C2, HW2, T, clips, K = kw["shape"]
    a1 = inp["a1"].to(dt).requires_grad_(True)
    a2 = inp["a2"].to(dt).requires_grad_(True)
    W = inp["W"].to(dt)
    pooled = a1.view(clips, T, C1, HW1).mean((1, 3))
    if not kw["fused"]:
        second = a2.view(clips, T, C2, HW2).mean((1, 3))
        pooled = torch.cat([pooled, torch.zeros_like(second) if drop == "second" else second], 1)
    logits = pooled @ W.t()
    if kw["bias"] and drop != "bias":
        logits = logits + inp["bias"].to(dt)
    loss_each = F.cross_entropy(logits, inp["labels"].long(), reduction="none")
    feats = [a1] if kw["fused"] else [a1, a2]
    gs = torch.autograd.grad(HEAD_SCALE * loss_each.mean(), feats, allow_unused=True)
    out = {"logits": ("tensor", logits.detach()), "loss_each": ("scalar", loss_each.detach())}
    for i, g in enumerate(gs):
        _finish_grad(out, f"grad{i + 1}", g if g is not None else torch.zeros_like(feats[i]), inp[f"a{i + 1}"], inp[f"base{i + 1}"], kw,
                     mask=0 if drop == "mask" else None)
    return out


GP_DECAY = 0.9


def _ref_gp(kw, inp, dt, drop):
    g = inp["g"].to(dt)
    if kw["fm"]:
        g = g.permute(0, 2, 1, 3, 4)
    dims = {1: (1, 3, 4), 2: (1, 2, 3, 4), 3: (1, 2, 3)}
    mode = kw["mode"]
    if mode in dims:
        g = g / g.abs().mean(dims[mode], keepdim=True)
    elif mode == 4:
        g = g / g.abs().sum()
    g = g.contiguous()
    if not kw["mom"]:
        return {"out": ("tensor", g)}
    if drop != "momentum":
        g = g + GP_DECAY * inp["mom"].to(dt)
    return {"out": ("tensor", g), "mom": ("tensor", g), "x_mom_is_out": ("exact", torch.tensor(True))}


def _cstd(dt):
    return torch.tensor(restate.STD, dtype=dt).view(1, 3, 1, 1, 1)


def _ref_misc(case, inp, dt, drop):
    kw, op = case.kw, case.op
    if op == "tap_perts":
        return {"out": ("tensor", (inp["adv"].to(dt) - inp["vid"].to(dt)) / _cstd(dt))}
    if op == "tap_grad":
        return {"out": ("tensor", inp["gx"].to(dt).permute(0, 2, 1, 3, 4) + TAP_WEIGHT * inp["bs"].to(dt) / _cstd(dt))}
    if op == "tap_sign":
        return {"x_sign": ("exact", torch.sign(inp["x"]).view(torch.int32)), "reg": ("scalar", inp["x"].to(dt).abs().sum().reshape(1))}
    if op == "aens_reduce":
        s = inp["cos"].to(dt).sum(1)
        return {"feat_sum": ("tensor", s), "weighted": ("tensor", inp["coeffs"].to(dt) * s)}
    if op == "aens_coeffs":
        return {"coeffs": ("tensor", restate.aens_coeffs(inp["prev"].to(dt), inp["coeffs"].to(dt), AENS_MOMENTUM))}
    if op == "dwconv":
        x, k, axis = inp["x"].to(dt), kw["k"], kw["axis"]
        xm = x.movedim(axis, -1)
        y = F.conv1d(xm.reshape(-1, 1, xm.shape[-1]), inp["taps"].to(dt).view(1, 1, k), padding=k // 2)     # (a correlation, as conv1d is)
        return {"out": ("tensor", y.view(xm.shape).movedim(-1, axis).contiguous())}
    if op == "resample":
        my, mx = inp["my"].long(), inp["mx"].long()
        x = inp["x"].to(dt).requires_grad_(True)
        y = x[:, :, my.clamp_min(0)][:, :, :, mx.clamp_min(0)] * ((my >= 0)[:, None] & (mx >= 0)[None, :]).to(dt)
        gs, = torch.autograd.grad((y * inp["g"].to(dt)).sum(), x)
        fwd = inp["x"][:, :, my.clamp_min(0)][:, :, :, mx.clamp_min(0)] * ((my >= 0)[:, None] & (mx >= 0)[None, :]).float()
        return {"x_fwd": ("exact", fwd + 0.0), "bwd": ("tensor", gs)}
    if op == "ttmix":
        g, k, w = inp["g"].to(dt), inp["k"].to(dt), float(np.float32(kw["w"]))
        plain = sum(k[d] * g[d] for d in range(kw["D"]))
        rolled = sum(k[d] * torch.roll(g[d], -int(inp["moves"][d]), 2) for d in range(kw["D"]))
        return {"out": ("tensor", (1 - w) * plain + w * rolled)}
    if op == "compose":
        xn, _ = restate.compose(inp["u"], inp["d"], inp["eps"])          # bit-exact against float32 whatever `dt`
        if kw["video_layout"]:
            xn = restate.unflatten_frames(xn, *inp["bf"]).contiguous()
        return {"x_out": ("exact", xn)}
    raise KeyError(op)


TAP_WEIGHT = 0.37
AENS_MOMENTUM = 0.7
_REFS = {"cos": _ref_cos, "std": _ref_std, "ilaf": _ref_ilaf, "tapd": _ref_tapd, "head": _ref_head, "gp": _ref_gp}


def evaluate(case: Case, dt=torch.float64, drop=None, raw=False):
    """The reference in `dt`; `drop` removes one ingredient ("mask", "bias", "second", "momentum", "segments") for the sanity checks,
    `raw` the accumulate base (so that the checks weigh the entry's own result)."""
    inp = inputs(case)
    if case.op in _REFS:
        return _REFS[case.op](dict(case.kw, acc=0) if raw and "acc" in case.kw else case.kw, inp, dt, drop)
    return _ref_misc(case, inp, dt, drop)


@functools.lru_cache(maxsize=4)
def reference(case: Case):
    return evaluate(case)


def _scale(kind, want):
    return 1.0 if kind == "cos" else float(want.abs().max())


def error(kind, got, want):
    """The error of one output, normalised as its bound is."""
    got, want = got.double(), want.double()
    assert got.shape == want.shape, (tuple(got.shape), tuple(want.shape))
    if got.numel() == 0:
        return 0.0
    if not bool(torch.isfinite(got).all()):
        return float("inf")
    if kind == "scalar":
        return float(((got - want).abs() / want.abs()).max())
    return float((got - want).abs().max()) / _scale(kind, want)


def fp32_errors(case: Case):
    """{output: error of the float32 CPU evaluation of the reference against its float64 evaluation} for the floating outputs."""
    r64, r32 = reference(case), evaluate(case, torch.float32)
    return {name: error(kind, r32[name][1], want) for name, (kind, want) in r64.items() if kind != "exact"}


def same_bits(a, b):
    if a.dtype.is_floating_point:
        a, b = a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)
    return a.shape == b.shape and bool(torch.equal(a, b))


def check(case: Case, got, e32, report=None):
    """Hold every output of `got` to its bound; `e32`: this case's entry of the committed fixture.  Returns {output: error}."""
    ref = reference(case)
    assert set(got) == set(ref), (case.id, sorted(got), sorted(ref))
    assert set(e32) == {n for n, (k, _) in ref.items() if k != "exact"}, (case.id, sorted(e32))
    errs = {}
    for name, (kind, want) in ref.items():
        if kind == "exact":
            g = got[name]
            assert g.dtype == want.dtype and same_bits(g, want), f"{case.id}: {name} differs from the exact reference at {int((g != want).sum()) if g.shape == want.shape else 'every'} element(s)"
            continue
        if kind != "cos" and want.numel():
            assert float(want.abs().max()) > 0, (case.id, name)
        errs[name] = error(kind, got[name], want)
        bound = max(FLOOR[kind], 4 * e32[name])
        if report is not None:
            report(f"{case.id:44s} {name:10s} {kind:6s} error {errs[name]:.3g}  bound {bound:.3g}  (e32 {e32[name]:.3g})")
    for name, err in errs.items():
        kind = ref[name][0]
        bound = max(FLOOR[kind], 4 * e32[name])
        assert err <= bound, f"{case.id}: {name} ({kind}) error {err:.3g} > bound {bound:.3g} = max({FLOOR[kind]:g}, 4 * {e32[name]:.3g})"
    return errs


# ---------------------------------------------------------------------------------------------------------------------------
# running a case through the C entries
# ---------------------------------------------------------------------------------------------------------------------------
class _Ctx:
    def __init__(self, eng):
        self.eng, self.capi, self.cuda = eng, eng.capi, eng.device.type == "cuda"

    def up(self, t):
        return t.to(self.eng.device) if self.cuda else t.clone()

    def new(self, *shape, fill=float("nan"), dtype=torch.float32):
        return torch.full(shape, fill, dtype=dtype, device=self.eng.device)

    def scratch(self, nbytes):
        return torch.zeros((int(nbytes) + 7) // 8 + 8, dtype=torch.float64, device=self.eng.device)

    def call(self, name, *args):
        lib.check(self.capi, getattr(self.capi, name)(*args, self.eng.stream()))

    def down(self, t):
        if self.cuda:
            torch.cuda.synchronize()
        return t.detach().cpu().clone()


def _view(buf, rows, D, pad, off):
    return buf[off:off + rows * (D + pad)].view(rows, D + pad)


class _Strided:
    """A (rows, D) operand as a view `off` floats into its own allocation with row stride D + pad."""

    def __init__(self, cx, t, pad, off, slack=0.0):
        rows, D = t.shape
        buf = torch.full((off + rows * (D + pad),), slack)
        _view(buf, rows, D, pad, off)[:, :D] = t
        self.cx, self.rows, self.D, self.pad, self.off = cx, rows, D, pad, off
        self.buf = cx.up(buf)
        self.view = _view(self.buf, rows, D, pad, off)
        self.ptr, self.stride = P(self.view.data_ptr()), D + pad
        assert self.view.data_ptr() == self.buf.data_ptr() + 4 * off


class _Grad(_Strided):
    """The gradient operand: SENTINEL in the slack; the base when accumulating, NaN otherwise."""

    def __init__(self, cx, base, kw):
        super().__init__(cx, base if kw["acc"] else torch.full_like(base, float("nan")), kw["pad"], kw["off"], SENTINEL)

    def collect(self, out, name, a, kw):
        buf = self.cx.down(self.buf)
        v = _view(buf, self.rows, self.D, self.pad, self.off)
        out[name] = v[:, :self.D].contiguous()
        out[name + "_x_slack"] = torch.cat([buf[:self.off], v[:, self.D:].reshape(-1)])
        if kw["mask"]:
            out[name + "_x_gated"] = out[name][~(a > 0)]


def _run_cos(cx, kw, inp):
    D, n = kw["D"], kw["frames"]
    a, b = _Strided(cx, inp["a"], kw["pad"], kw["off"]), _Strided(cx, inp["b"], kw["pad"], kw["off"])
    g = _Grad(cx, inp["base"], kw)
    cos, coef = cx.new(n), cx.up(inp["coef"])
    sc = cx.scratch(cx.capi.i2v_cossim_scratch_bytes(D, n))
    cx.call("i2v_cossim_fwd_bwd_f32", a.ptr, a.stride, b.ptr, b.stride, D, n, P(coef.data_ptr()) if kw["coef"] else NULL, 1, 0.5,
            kw["mask"], kw["acc"], P(cos.data_ptr()), g.ptr, g.stride, P(sc.data_ptr()))
    out = {"cos": cx.down(cos)}
    g.collect(out, "grad", inp["a"], kw)
    return out


def _run_std(cx, kw, inp):
    D, n = kw["D"], kw["frames"]
    a, g = _Strided(cx, inp["a"], kw["pad"], kw["off"]), _Grad(cx, inp["base"], kw)
    std = cx.new(1)
    sc = cx.scratch(cx.capi.i2v_cossim_scratch_bytes(D, n + 1))
    tail = (kw["mask"], kw["acc"], P(std.data_ptr()), g.ptr, g.stride, P(sc.data_ptr()))
    if kw["how"] == "fused":
        cx.call("i2v_std_fwd_bwd_f32", a.ptr, a.stride, D, n, *tail)
    else:
        total = n * D
        if kw["how"] == "shards":
            o = _Strided(cx, inp["other"], 1, 0)
            cx.call("i2v_std_reduce_f32", o.ptr, o.stride, D, n + 1, P(sc.data_ptr()))
            other = sc[:2].clone()
            total += (n + 1) * D
        cx.call("i2v_std_reduce_f32", a.ptr, a.stride, D, n, P(sc.data_ptr()))
        if kw["how"] == "shards":
            sc[:2] += other                                   # what an all-reduce of the two shards' sums leaves
        cx.call("i2v_std_grad_f32", a.ptr, a.stride, D, n, total, *tail)
    out = {"std": cx.down(std)}
    g.collect(out, "grad", inp["a"], kw)
    return out


def _run_ilaf(cx, kw, inp):
    D, n, fps = kw["D"], kw["frames"], kw["fps"]
    nseg = n // fps
    a, g = _Strided(cx, inp["a"], kw["pad"], kw["off"]), _Grad(cx, inp["base"], kw)
    ori, adv0 = cx.up(inp["ori"]), cx.up(inp["adv0"])
    po, p0 = P(ori.data_ptr()), P(adv0.data_ptr())
    loss = cx.new(nseg)
    nbytes = cx.capi.i2v_ilaf_scratch_bytes(D, n, 0 if kw["one"] else fps)
    sc0, sc = cx.scratch(nbytes), cx.scratch(nbytes)
    if kw["one"]:
        cx.call("i2v_ilaf_reduce_f32", p0, D, po, p0, D, n, P(sc0.data_ptr()))
        n0 = float(cx.down(sc0)[0]) ** 0.5
        cx.call("i2v_ilaf_reduce_f32", a.ptr, a.stride, po, p0, D, n, P(sc.data_ptr()))
        cx.call("i2v_ilaf_grad_f32", a.ptr, a.stride, po, p0, D, n, n0, kw["mask"], kw["acc"], P(loss.data_ptr()), g.ptr, g.stride, P(sc.data_ptr()))
    else:
        cx.call("i2v_ilaf_reduce_seg_f32", p0, D, po, p0, D, n, fps, P(sc0.data_ptr()))
        init_sq = sc0[:2 * nseg:2].contiguous()              # |adv0 - ori|^2 per segment, read from the scratch of the initial call
        cx.call("i2v_ilaf_reduce_seg_f32", a.ptr, a.stride, po, p0, D, n, fps, P(sc.data_ptr()))
        cx.call("i2v_ilaf_grad_seg_f32", a.ptr, a.stride, po, p0, D, n, fps, P(init_sq.data_ptr()), kw["mask"], kw["acc"], P(loss.data_ptr()),
                g.ptr, g.stride, P(sc.data_ptr()))
    out = {"loss": cx.down(loss)}
    g.collect(out, "grad", inp["a"], kw)
    return out


def _run_tapd(cx, kw, inp):
    D, n, fps = kw["D"], kw["frames"], kw["fps"]
    a, g = _Strided(cx, inp["a"], kw["pad"], kw["off"]), _Grad(cx, inp["base"], kw)
    clean = cx.up(inp["clean"])
    dist = cx.new(n // fps)
    sc = cx.scratch(cx.capi.i2v_ilaf_scratch_bytes(D, n, fps))
    cx.call("i2v_tap_distance_f32", a.ptr, a.stride, P(clean.data_ptr()), D, n, fps, 0.7, kw["mask"], kw["acc"], P(dist.data_ptr()), g.ptr, g.stride,
            P(sc.data_ptr()))
    out = {"dist": cx.down(dist)}
    g.collect(out, "grad", inp["a"], kw)
    return out


def _run_head(cx, kw, inp):
    C1, HW1, C2, HW2, T, clips, K = kw["shape"]
    feats = [(C1, HW1, "1")] if kw["fused"] else [(C1, HW1, "1"), (C2, HW2, "2")]
    Ctot = sum(f[0] for f in feats)
    acts = [_Strided(cx, inp["a" + s], kw["pad"], kw["off"]) for _, _, s in feats]
    grads = [_Grad(cx, inp["base" + s], kw) for _, _, s in feats]
    W, bias, labels = cx.up(inp["W"]), cx.up(inp["bias"]), cx.up(inp["labels"])
    pb = P(bias.data_ptr()) if kw["bias"] else NULL
    logits, loss_each = cx.new(clips, K), cx.new(clips)
    sc = cx.scratch(cx.capi.i2v_head_scratch_bytes(Ctot, clips))
    ps = P(sc.data_ptr())
    if kw["fused"]:
        cx.call("i2v_head_ce_f32", acts[0].ptr, acts[0].stride, C1, HW1, T, clips, P(W.data_ptr()), pb, K, P(labels.data_ptr()), HEAD_SCALE,
                kw["mask"], kw["acc"], P(logits.data_ptr()), P(loss_each.data_ptr()), grads[0].ptr, grads[0].stride, ps)
    else:
        off = 0
        for (C, HW, _), a in zip(feats, acts):
            cx.call("i2v_head_pool_f32", a.ptr, a.stride, C, HW, T, clips, Ctot, off, ps)
            off += C
        cx.call("i2v_head_logits_ce_f32", Ctot, clips, P(W.data_ptr()), pb, K, P(labels.data_ptr()), HEAD_SCALE, P(logits.data_ptr()),
                P(loss_each.data_ptr()), ps)
        off = 0
        for (C, HW, _), a, g in zip(feats, acts, grads):
            cx.call("i2v_head_grad_f32", a.ptr, a.stride, C, HW, T, clips, Ctot, off, kw["mask"], kw["acc"], g.ptr, g.stride, ps)
            off += C
    out = {"logits": cx.down(logits), "loss_each": cx.down(loss_each)}
    for (_, _, s), g in zip(feats, grads):
        g.collect(out, "grad" + s, inp["a" + s], kw)
    return out


def _run_gp(cx, kw, inp):
    b, c, f, h, w = kw["shape"]
    g, out = cx.up(inp["g"]), cx.new(b, c, f, h, w)
    mom = cx.up(inp["mom"]) if kw["mom"] else None
    sc = cx.scratch(cx.capi.i2v_grad_post_scratch_bytes(b, c, f, h, w, kw["mode"]))
    cx.call("i2v_grad_post_f32", P(g.data_ptr()), P(mom.data_ptr()) if kw["mom"] else NULL, P(out.data_ptr()), b, c, f, h, w, kw["fm"], kw["mode"],
            GP_DECAY, P(sc.data_ptr()))
    res = {"out": cx.down(out)}
    if kw["mom"]:
        res["mom"] = cx.down(mom)
        res["x_mom_is_out"] = torch.tensor(same_bits(res["mom"], res["out"]))
    return res


def _run_misc(cx, case, inp):
    kw, op = case.kw, case.op
    if op == "tap_perts":
        adv, vid = cx.up(inp["adv"]), cx.up(inp["vid"])
        out = cx.new(*kw["shape"])
        cx.call("i2v_tap_perts_f32", P(adv.data_ptr()), P(vid.data_ptr()), P(out.data_ptr()), *kw["shape"])
        return {"out": cx.down(out)}
    if op == "tap_grad":
        gx, bs = cx.up(inp["gx"]), cx.up(inp["bs"])
        out = cx.new(*kw["shape"])
        cx.call("i2v_tap_grad_f32", P(gx.data_ptr()), P(bs.data_ptr()), P(out.data_ptr()), *kw["shape"], TAP_WEIGHT)
        return {"out": cx.down(out)}
    if op == "tap_sign":
        x, sg, reg = cx.up(inp["x"]), cx.new(kw["n"]), cx.new(1)
        sc = cx.scratch(cx.capi.i2v_tap_scratch_bytes(kw["n"]))
        cx.call("i2v_tap_sign_abs_f32", P(x.data_ptr()), P(sg.data_ptr()), P(reg.data_ptr()), kw["n"], P(sc.data_ptr()))
        return {"x_sign": cx.down(sg).view(torch.int32), "reg": cx.down(reg)}
    if op == "aens_reduce":
        cos, co = cx.up(inp["cos"]), cx.up(inp["coeffs"])
        fs, wt = cx.new(kw["L"]), cx.new(kw["L"])
        cx.call("i2v_aens_reduce_f32", P(cos.data_ptr()), P(co.data_ptr()), kw["L"], kw["frames"], P(fs.data_ptr()), P(wt.data_ptr()))
        return {"feat_sum": cx.down(fs), "weighted": cx.down(wt)}
    if op == "aens_coeffs":
        prev, co = cx.up(inp["prev"]), cx.up(inp["coeffs"])
        cx.call("i2v_aens_coeffs_f32", P(prev.data_ptr()), P(co.data_ptr()), AENS_MOMENTUM, kw["L"])
        return {"coeffs": cx.down(co)}
    if op == "dwconv":
        x, taps = cx.up(inp["x"]), inp["taps"].contiguous()          # (the taps are a host array)
        out = cx.new(*kw["shape"])
        shp, ax = kw["shape"], kw["axis"]
        cx.call("i2v_dwconv1d_f32", P(x.data_ptr()), P(out.data_ptr()), int(np.prod(shp[:ax])), shp[ax], int(np.prod(shp[ax + 1:])),
                P(taps.data_ptr()), kw["k"])
        return {"out": cx.down(out)}
    if op == "resample":
        x, g, my, mx = (cx.up(inp[k]) for k in ("x", "g", "my", "mx"))
        planes, (Hs, Ws), (Hd, Wd) = 6, x.shape[-2:], g.shape[-2:]
        fwd, bwd = cx.new(2, 3, Hd, Wd), cx.new(2, 3, Hs, Ws)
        cx.call("i2v_resample_nearest_f32", P(x.data_ptr()), P(fwd.data_ptr()), planes, Hs, Ws, Hd, Wd, P(my.data_ptr()), P(mx.data_ptr()))

        def ranges(m, n):        # per source index: the contiguous run of output positions that read it (empty: lo == hi)
            lo, hi = torch.zeros(n, dtype=torch.int32), torch.zeros(n, dtype=torch.int32)
            for s in range(n):
                hit = (m == s).nonzero().flatten()
                if hit.numel():
                    lo[s], hi[s] = int(hit[0]), int(hit[-1]) + 1
            return cx.up(lo), cx.up(hi)
        ylo, yhi = ranges(inp["my"], Hs)
        xlo, xhi = ranges(inp["mx"], Ws)
        cx.call("i2v_resample_nearest_bwd_f32", P(g.data_ptr()), P(bwd.data_ptr()), planes, Hd, Wd, Hs, Ws, P(ylo.data_ptr()), P(yhi.data_ptr()),
                P(xlo.data_ptr()), P(xhi.data_ptr()))
        return {"x_fwd": cx.down(fwd), "bwd": cx.down(bwd)}
    if op == "ttmix":
        g = cx.up(inp["g"])
        D, N, C_, T, H, W = g.shape
        out = cx.new(N, C_, T, H, W)
        k, mv = inp["k"].contiguous(), inp["moves"].contiguous()      # (host arrays)
        cx.call("i2v_tt_grad_mix_f32", P(g.data_ptr()), P(out.data_ptr()), P(k.data_ptr()), P(mv.data_ptr()), D, N * C_, T, H * W, kw["w"])
        return {"out": cx.down(out)}
    if op == "compose":
        u, d = cx.up(inp["u"]), cx.up(inp["d"])
        b, f = inp["bf"]
        h, w = u.shape[-2:]
        out = cx.new(b, 3, f, h, w) if kw["video_layout"] else cx.new(b * f, 3, h, w)
        cx.call("i2v_compose_f32", P(u.data_ptr()), P(d.data_ptr()), P(out.data_ptr()), b, f, h, w, inp["eps"], kw["video_layout"])
        return {"x_out": cx.down(out)}
    raise KeyError(op)


_RUNS = {"cos": _run_cos, "std": _run_std, "ilaf": _run_ilaf, "tapd": _run_tapd, "head": _run_head, "gp": _run_gp}


def run(engine, case: Case):
    """One case through the C entries of `engine.capi`: {output name: CPU tensor}."""
    cx, inp = _Ctx(engine), inputs(case)
    if case.op in _RUNS:
        return _RUNS[case.op](cx, case.kw, inp)
    return _run_misc(cx, case, inp)


# ---------------------------------------------------------------------------------------------------------------------------
# refusals: valid argument lists, and the one argument to spoil
# ---------------------------------------------------------------------------------------------------------------------------
def refusals(engine):
    """([(label, entry name, thunk -> status)], buffers to keep alive): every thunk must return non-zero and leave the entry's name in
    i2v_last_error.  No thunk launches anything: each is refused by the entry's argument check."""
    cx = _Ctx(engine)
    buf = cx.new(4096, fill=0.0)
    host = torch.zeros(64)
    hosti = torch.zeros(64, dtype=torch.int32)
    B = [P(buf.data_ptr() + 1024 * i) for i in range(8)]
    H, HI = P(host.data_ptr()), P(hosti.data_ptr())
    valid = {
        "i2v_compose_f32": [B[0], B[1], B[2], 1, 1, 2, 2, 0.1, 0],
        "i2v_cossim_fwd_bwd_f32": [B[0], 8, B[1], 8, 8, 2, NULL, 0, 1.0, 0, 0, B[2], B[3], 8, B[4]],
        "i2v_std_reduce_f32": [B[0], 8, 8, 2, B[4]],
        "i2v_std_grad_f32": [B[0], 8, 8, 2, 16, 0, 0, B[2], B[3], 8, B[4]],
        "i2v_std_fwd_bwd_f32": [B[0], 8, 8, 2, 0, 0, B[2], B[3], 8, B[4]],
        "i2v_ilaf_reduce_f32": [B[0], 8, B[1], B[2], 8, 2, B[4]],
        "i2v_ilaf_grad_f32": [B[0], 8, B[1], B[2], 8, 2, 1.0, 0, 0, B[5], B[3], 8, B[4]],
        "i2v_ilaf_reduce_seg_f32": [B[0], 8, B[1], B[2], 8, 4, 2, B[4]],
        "i2v_ilaf_grad_seg_f32": [B[0], 8, B[1], B[2], 8, 4, 2, B[6], 0, 0, B[5], B[3], 8, B[4]],
        "i2v_tap_distance_f32": [B[0], 8, B[1], 8, 4, 2, 0.7, 0, 0, B[5], B[3], 8, B[4]],
        "i2v_head_ce_f32": [B[0], 8, 4, 2, 1, 2, B[1], NULL, 3, B[6], 1.0, 0, 0, B[2], B[5], B[3], 8, B[4]],
        "i2v_head_pool_f32": [B[0], 8, 4, 2, 1, 2, 6, 2, B[4]],
        "i2v_head_logits_ce_f32": [6, 2, B[1], NULL, 3, B[6], 1.0, B[2], B[5], B[4]],
        "i2v_head_grad_f32": [B[0], 8, 4, 2, 1, 2, 6, 2, 0, 0, B[3], 8, B[4]],
        "i2v_tt_grad_mix_f32": [B[0], B[1], H, HI, 3, 2, 5, 4, 0.3],
        "i2v_resample_nearest_f32": [B[0], B[1], 1, 2, 2, 2, 2, B[6], B[7]],
        "i2v_resample_nearest_bwd_f32": [B[0], B[1], 1, 2, 2, 2, 2, B[4], B[5], B[6], B[7]],
        "i2v_dwconv1d_f32": [B[0], B[1], 2, 4, 3, H, 3],
        "i2v_grad_post_f32": [B[0], NULL, B[1], 1, 3, 2, 2, 2, 0, 1, 0.9, B[4]],
        "i2v_tap_perts_f32": [B[0], B[1], B[2], 1, 3, 2, 2, 2],
        "i2v_tap_sign_abs_f32": [B[0], B[1], B[2], 16, B[4]],
        "i2v_tap_grad_f32": [B[0], B[1], B[2], 1, 3, 2, 2, 2, 0.5],
        "i2v_aens_coeffs_f32": [B[0], B[1], 0.7, 6],
        "i2v_aens_reduce_f32": [B[0], B[1], 6, 4, B[2], B[3]],
    }
    spoil = [(name, "null pointer", 0, NULL) for name in valid if name != "i2v_head_logits_ce_f32"]
    spoil += [
        ("i2v_head_logits_ce_f32", "null pointer", 2, NULL),
        ("i2v_cossim_fwd_bwd_f32", "D = 0", 4, 0), ("i2v_std_reduce_f32", "D = 0", 2, 0), ("i2v_std_grad_f32", "D = -1", 2, -1),
        ("i2v_std_fwd_bwd_f32", "D = 0", 2, 0), ("i2v_ilaf_reduce_f32", "D = 0", 4, 0), ("i2v_ilaf_grad_f32", "D = 0", 4, 0),
        ("i2v_ilaf_reduce_seg_f32", "D = 0", 4, 0), ("i2v_ilaf_grad_seg_f32", "D = 0", 4, 0), ("i2v_tap_distance_f32", "D = 0", 3, 0),
        ("i2v_ilaf_reduce_seg_f32", "frames % frames_per_seg", 6, 3), ("i2v_ilaf_grad_seg_f32", "frames % frames_per_seg", 6, 3),
        ("i2v_tap_distance_f32", "frames % frames_per_seg", 5, 3),
        ("i2v_std_grad_f32", "total_count = 1", 4, 1),
        ("i2v_dwconv1d_f32", "even k", 6, 4), ("i2v_dwconv1d_f32", "k = 65", 6, 65), ("i2v_dwconv1d_f32", "in place", 1, B[0]),
        ("i2v_grad_post_f32", "in place", 2, B[0]), ("i2v_grad_post_f32", "mode 5", 9, 5),
        ("i2v_aens_coeffs_f32", "L = 65", 3, 65), ("i2v_tt_grad_mix_f32", "D = 65", 4, 65),
        ("i2v_tap_perts_f32", "c = 4", 4, 4), ("i2v_tap_grad_f32", "c = 4", 4, 4),
        ("i2v_head_pool_f32", "c_off + C > Ctot", 7, 3), ("i2v_head_grad_f32", "c_off + C > Ctot", 7, 3),
    ]
    out = []
    for name, what, idx, value in spoil:
        args = list(valid[name])
        args[idx] = value
        out.append((f"{name}: {what}", name, functools.partial(getattr(cx.capi, name), *args, engine.stream())))
    # one frame of one element: frames * D = 1 < 2 inside the fused entry
    args = list(valid["i2v_std_fwd_bwd_f32"])
    args[2], args[3] = 1, 1
    out.append(("i2v_std_fwd_bwd_f32: total_count = 1", "i2v_std_fwd_bwd_f32", functools.partial(cx.capi.i2v_std_fwd_bwd_f32, *args, engine.stream())))
    return out, (buf, host, hosti)
