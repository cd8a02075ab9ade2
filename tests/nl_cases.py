"""TEST INFRASTRUCTURE: the case table of the I3D non-local block's launches (csrc/i2v_kernels.hip: `attn_gemm_kernel<1|2|3>`,
`attn_split_reduce_kernel`, `softmax_rows_kernel`) and of `addmask_kernel`, which sits next to them in a net's launch list; scalar twins
in tests/hostsim/hostsim_backend.cpp (`k_attn_gemm`, `k_softmax_rows`, `k_addmask`).  tests/test_nl_kernels_cpu.py runs every case on
the host simulation, tests/test_gpu_nl_kernels.py on the device, and holds the two to the same bits.

`run(engine, case)` calls the C entries of include/i2v_nl_launch.h through `engine.capi` with buffers on the engine's device and returns
{name: CPU tensor}.  `reference(case)` returns {name: (kind, tensor)} over the SAME names: nothing an entry writes is left unchecked.
The references are the formulas of csrc/i2v_params.h (I2VAttnGemm, I2VSoftmaxRows, I2VAddMaskParams) in plain torch: `einsum` for
the three product forms, `softmax` and its autograd for the row softmax and its backward.

Kinds and bounds (`check`), the loop table's rule:
  tensor   max|got - want| <= max(2e-6, 4 e32) * max|want|      (2e-6: tests/loop_cases.py's `tensor` floor; 4: DESIGN.md section 14)
  exact    equal bits: addmask (one fp32 sum in the kernel's order ((0 + a0) + a1) + a2, the gate, the gain: every step correctly
           rounded), the slack of every output, the inputs after the launch, the uniform softmax row (1 / N, N a power of two), the
           N = 1 row (P = 1, dS = 0) and the empty-segment identity (K = 64 in three segments has the bits of K = 64 in two)
e32 is the error of the same reference evaluated in float32 by plain torch on the CPU, normalised the same way and committed as
tests/golden/nl_fp32_cpu_errors.json (tests/make_nl_fixtures.py).

Buffers.  Every operand is a view into a larger flat allocation: FRONT = 128 floats ahead of it (+ `off`: 1 misaligns the base by 4
bytes); an activation view's frames lie `nstride` floats apart (`gap` = nstride - channels * HW floats between them); after the last
frame come 4 * nstride + 256 floats (a dense matrix: 256) -- four whole frames, so that a group of four positions read past the end of
the last clip at HW = 1 still lands inside the allocation.  Everything of an OUTPUT allocation that is not an addressed element is
SENTINEL and must come back bit for bit (`<name>_slack`); its addressed elements start as NaN, or as a random base under `accumulate`,
so an element no lane wrote fails.  Everything of an INPUT allocation that is not an addressed element is NaN -- a stray read poisons a
checked output -- and the whole allocation must have its bits after the launch (`inputs_unchanged`).

Branch arithmetic of csrc/i2v_kernels.hip (re-derive the comments at the cases when any of it changes):
  attn_gemm_kernel<FORM>: one block of 256 threads = 4 waves (wd = wave / 2 down the rows, wp = wave % 2 across the columns) owns a
    64 x 64 output tile, each wave a 32 x 32 quarter on v_mfma_f32_32x32x2_f32.  (rows, columns, K) = (M, N, Cc) in form 1, (Cc, M, N)
    in form 2, (Cc, N, M) in form 3.  blockIdx.x = tile_row * tiles_n + tile_col with tiles_n = ceil(columns / 64): a 3 x 1 grid
    against a 1 x 3 one tells `/` from `%`.  blockIdx.y = clip (per-clip offsets clip * M * N of the dense matrix, clip * T frames of
    a view), blockIdx.z = K segment.
    K is walked in chunks of KC = 32, double-buffered: ceil(K / 32) chunks; one chunk prefetches nothing (K <= 32), two use both LDS
    buffers (33 .. 64), three wrap the parity (65 .. 96), four end on the odd buffer again (97).  A chunk is 16 MFMA steps of
    k = 2 s + lk (lk = lane / 32): K = 1 runs one step's lk = 0 half, K = 2 one whole step; rows of the chunk past K are zero fill.
    `fetch`, two pieces h = 0, 1 per thread t: an operand whose contiguous axis is the tile's (form 1: A and B; form 3: the dense
    matrix) gives k = t / 16 + 16 h and four columns from 4 (t % 16), lim = count - column; one whose contiguous axis is K (forms 2, 3:
    A; form 2: the dense matrix) gives row t / 4 and four k from 4 (t % 4) + 16 h, lim = K - k: the K tail of 1 .. 3.  A group of four
    is one float4 load when lim >= 4 AND the operand's flag is set, else min(lim, 4) scalar loads, each with its own frame / position
    split (`load4_act`): with HW = 1, 3, 9, 49 a group crosses frames.  Flags: a view's = HW % 4 == 0 and nstride % 4 == 0 and a
    16-byte aligned base; the dense input's = N % 4 == 0 and a 16-byte aligned base.
    Epilogue: column = n0 + 32 wp + lane % 32, row = m0 + 32 wd + (r & 3) + 8 (r >> 2) + 4 lk for r < 16: edges at 32 (a wave's
    quarter) and 64 (the tile); 130 = two tiles and two rows / columns of a third.  Form 1 stores scale * acc (scale == 1: acc) to the
    dense matrix; forms 2 / 3 store or add (accumulate) through the output view's own (C_T, C_HW, C_nstride).
  K-split (forms 2 / 3, ksplit > 1; form 1 ignores it): segment z = [z * kseg, min((z + 1) * kseg, K)) with
    attn_kseg(K, ksplit) = ceil(ceil(K / ksplit) / 32) * 32, a whole number of chunks, so segment starts stay 16-byte aligned;
    K = 64, ksplit = 3 gives kseg 32 and an EMPTY third segment (the planner never plans one: ksplit = min(8, K / 256) from K >= 512
    and at most 128 tiles per clip, i2v_plan.cpp; its smallest is K = 512 in two segments of 256).  Segment sums go to
    part[clip][z][row][column]; attn_split_reduce_kernel adds them in z order, then stores or adds through the view.
  softmax_rows_kernel: one block of 256 threads per row, thread t owns columns t, t + 256, ...: a second trip from N = 257, a third
    from 513; a wave's 64 partial values are folded by shuffles, the four wave values in order.  Rows are dense (row r starts at
    r * N), so with N odd they start at every alignment.
  addmask_kernel: one thread per element in a grid-stride loop of at most 4096 blocks of 256: a second pass above 1 048 576 elements
    (3 x 7 x 50021 = 1 050 441 takes it); 1-bit gates are rows of gate_stride 32-bit words per channel, bit n * HW + i: with HW = 5,
    49 frames share words, with HW = 32 each has its own.
"""
import ctypes
import functools
import itertools
import zlib
from dataclasses import dataclass
from typing import Tuple

import torch

from i2v_amd import lib

SENTINEL = -123.25
FLOOR = 2e-6
FRONT = 128
NAN = float("nan")


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


# ---------------------------------------------------------------------------------------------------------------------------
# the table
# ---------------------------------------------------------------------------------------------------------------------------
EDGES = (1, 31, 32, 33, 63, 64, 65, 130)
KS = (2, 34, 66, 96, 97)
INTERIOR = (48, 40, 24)                       # rows, columns, K: every count a multiple of 4 whose default view takes the vector path
VIEW_HW = (1, 3, 9, 49)
VIEW_T = (2, 3, 5)


def _split(n):
    """(T, HW) of a count's default view: T its smallest prime factor (a prime count: HW = 1, every position a frame of its own)."""
    for p in range(2, int(n ** 0.5) + 1):
        if n % p == 0:
            return p, n // p
    return n, 1


def _p(form, id, rows, cols, K, **kw):
    return _case(f"gemm{form}", id, form=form, rows=rows, cols=cols, K=K, **kw)


def _product_cases():
    out = []
    R0, C0, K0 = INTERIOR
    for form in (1, 2, 3):
        # one axis at a time against the interior shape; forms 2 / 3 alternate write and accumulate, form 1 its two scales
        for i, e in enumerate(EDGES):
            alt = dict(scale=(1.0, 0.125)[i % 2]) if form == 1 else dict(acc=i % 2)
            out.append(_p(form, f"rows{e}", e, C0, K0, **alt))
            out.append(_p(form, f"cols{e}", R0, e, K0, **alt))
            out.append(_p(form, f"K{e}", R0, C0, e, **alt))
        # the K loop: one MFMA step (2), two chunks with a tail of 2 (34), three with a tail of 2 (66), three full (96), a tail of 1
        # after three full chunks (97); with the edges above K % 4 takes 1 (1, 33, 65, 97), 2 (2, 34, 66, 130) and 3 (31, 63)
        for K in KS:
            out.append(_p(form, f"K{K}", 33, 31, K))
        # joint corners; 130 x 65 is a 3 x 2 tile grid, 65 x 130 a 2 x 3 one
        for r, c, K in ((1, 1, 1), (65, 65, 33), (130, 65, 31), (65, 130, 65), (64, 64, 32), (63, 33, 97), (31, 130, 2)):
            out.append(_p(form, f"corner-{r}x{c}x{K}", r, c, K))
        # views: HW in {1, 3, 9, 49} x T in {2, 3, 5} for A, the other view (form 1: B; forms 2 / 3: the output) five combinations on,
        # so the two differ in T and in HW; gaps between frames on every second one
        combos = list(itertools.product(VIEW_HW, VIEW_T))
        for i, (hw, t) in enumerate(combos):
            hw2, t2 = combos[(i + 5) % len(combos)]
            gaps = dict(a_gap=3, **({"b_gap": 5} if form == 1 else {"c_gap": 5})) if i % 2 else {}
            if form == 1:
                out.append(_p(1, f"view-A{t}x{hw}-B{t2}x{hw2}", t * hw, t2 * hw2, 5, a=(t, hw), b=(t2, hw2), scale=0.125, **gaps))
            else:
                out.append(_p(form, f"view-A{t}x{hw}-C{t2}x{hw2}", 5, t2 * hw2, t * hw, a=(t, hw), c=(t2, hw2), acc=(i // 2) % 2, **gaps))
        # the vector path: HW = 4 and 16, dense and with a gap of 8 floats between frames
        for t, hw, gap in ((3, 4, 0), (2, 16, 0), (5, 4, 8), (2, 16, 8)):
            if form == 1:
                out.append(_p(1, f"vec-A{t}x{hw}-gap{gap}", t * hw, 2 * 16, 8, a=(t, hw), b=(2, 16), a_gap=gap, b_gap=gap))
            else:
                out.append(_p(form, f"vec-A{t}x{hw}-gap{gap}", 8, 2 * 9, t * hw, a=(t, hw), c=(2, 9), a_gap=gap, c_gap=gap))
        # the vector flags one at a time against a base that keeps them all: HW % 4 (18 for 16), nstride % 4 (a gap of 2), the base
        # one float in; the dense input: N % 4 (N = 34 for 32) and its base one float in.  8 channels.
        if form == 1:
            flags = [("all-set", {}), ("a-hw", dict(a=(2, 18), rows=36)), ("a-nstride", dict(a_gap=2)), ("a-base", dict(a_off=1)),
                     ("b-hw", dict(b=(2, 18), cols=36)), ("b-nstride", dict(b_gap=2)), ("b-base", dict(b_off=1)), ("d-base", dict(d_off=1))]
            for name, kw in flags:
                k = dict(rows=32, cols=32, a=(2, 16), b=(2, 16))
                k.update(kw)
                out.append(_p(1, "flag-" + name, k.pop("rows"), k.pop("cols"), 8, **k))
        else:
            # K = 32 is A's count and one axis of the dense matrix; N is K in form 2 and the column count in form 3
            flags = [("all-set", {}), ("a-hw", dict(a=(2, 18), K=36)), ("a-nstride", dict(a_gap=2)), ("a-base", dict(a_off=1)),
                     ("d-n", dict(K=34, a=(2, 17)) if form == 2 else dict(cols=34, c=(2, 17))), ("d-base", dict(d_off=1)),
                     ("c-base", dict(c_off=1)), ("c-gap", dict(c_gap=3))]
            for name, kw in flags:
                k = dict(cols=32, K=32, a=(2, 16), c=(2, 16))
                k.update(kw)
                out.append(_p(form, "flag-" + name, 8, k.pop("cols"), k.pop("K"), **k))
        # clips: the per-clip offsets of the views and of the dense matrix (3 x 37 x 35: M * N odd, clips 1 and 2 start misaligned)
        out.append(_p(form, "clips3", 37 if form == 1 else 6, 35, 6 if form == 1 else 37, clips=3, **({} if form == 1 else {"acc": 1})))
        out.append(_p(form, "clips3-vec", 32 if form == 1 else 8, 32, 8 if form == 1 else 64, clips=3))
    # K-split, forms 2 / 3 (kseg = attn_kseg(K, ksplit)):
    for form in (2, 3):
        for K, ks, what in ((64, 2, "whole"), (192, 3, "whole"), (256, 8, "whole"),              # kseg 32, 64, 32
                            (100, 2, "short-last"), (170, 3, "short-last"), (500, 8, "short-last"),  # 64 + 36; 64 + 64 + 42; 7 x 64 + 52
                            (70, 2, "sub-chunk-last"), (150, 3, "sub-chunk-last"), (250, 8, "sub-chunk-last")):  # 64 + 6; 64 + 64 + 22; 7 x 32 + 26
            out.append(_p(form, f"split{ks}-K{K}-{what}", 9, 33, K, ksplit=ks))
        out.append(_p(form, "split3-K64-empty-segment", 9, 33, 64, ksplit=3))                     # 32 + 32 + 0: must add exactly zero
        out.append(_p(form, "split8-K300-three-empty", 9, 33, 300, ksplit=8))                     # kseg 64: 4 x 64 + 44, then three empty
        out.append(_p(form, "split2-K100-accumulate", 9, 33, 100, ksplit=2, acc=1))
        out.append(_p(form, "split3-K170-accumulate-clips3", 9, 33, 170, ksplit=3, acc=1, clips=3, c_gap=5))
        out.append(_p(form, "split2-K96-two-tiles", 65, 70, 96, ksplit=2))                        # 2 x 2 tiles per segment
        out.append(_p(form, "split2-K512-planner-smallest", 64, 32, 512, ksplit=2, a=(2, 256), c=(2, 16)))
    out.append(_p(1, "split4-ignored", 33, 31, 70, ksplit=4))                                     # form 1: one z slice, no scratch
    # the block's own ratios: theta T 2, HW 16; phi / g T 2, HW 4 (max-pooled 1 x 2 x 2); 8 channels; 2 clips.  Forward S, y; backward
    # in the planner's order dP, dg, (dS: softmax-block), dtheta, dphi -- each launch on the float32 rounding of the float64 chain
    for form, name in ((1, "S"), (2, "y"), (1, "dP"), (3, "dg"), (2, "dtheta"), (3, "dphi")):
        rows, cols, K = {"S": (32, 8, 8), "y": (8, 32, 8), "dP": (32, 8, 8), "dg": (8, 8, 32), "dtheta": (8, 32, 8), "dphi": (8, 8, 32)}[name]
        views = {"S": dict(a=(2, 16), b=(2, 4)), "y": dict(a=(2, 4), c=(2, 16)), "dP": dict(a=(2, 16), b=(2, 4)),
                 "dg": dict(a=(2, 16), c=(2, 4)), "dtheta": dict(a=(2, 4), c=(2, 16)), "dphi": dict(a=(2, 16), c=(2, 4))}[name]
        out.append(_p(form, "block-" + name, rows, cols, K, clips=2, block=name, **views))
    return out


# clip b of a 3-clip launch has the bits of that clip launched alone (i2v_plan.cpp: "a clip's result does not depend on the batch")
INVARIANCE = ("gemm1-clips3", "gemm2-clips3", "gemm3-clips3", "gemm1-clips3-vec", "gemm2-split3-K170-accumulate-clips3",
              "gemm3-split3-K170-accumulate-clips3")

SM_N = (1, 2, 63, 64, 65, 255, 256, 257, 513)
SM_ROWS = (1, 5)
SM_KINDS = ("one", "sat", "spike")
SM_WHY = "the softmax forward calls expf: the device's and glibc's round differently"


def _sm(id, rows, N, kind, **kw):
    # both modes run per case; only the forward (P) may differ from the host simulation's bits
    return _case("softmax", id, host_bits=False, why_not=SM_WHY, rows=rows, N=N, kind=kind, **kw)


def _softmax_cases():
    out = []
    for i, N in enumerate(SM_N):
        for j, rows in enumerate(SM_ROWS):
            kind = SM_KINDS[(i + j) % 3] if N > 2 else "one"
            out.append(_sm(f"N{N}-r{rows}-{kind}", rows, N, kind, off=(i + j) % 2))
    # every kind past one and past two trips, and at the wave edge
    for N in (65, 257, 513):
        for kind in SM_KINDS:
            out.append(_sm(f"N{N}-r5-{kind}-all-kinds", 5, N, kind, off=1))
    # an all-equal row, N a power of two: exactly 1 / N (N = 1: P = 1 and dS = 0 exactly)
    for N in (1, 2, 64, 256, 512):
        for rows in SM_ROWS:
            out.append(_sm(f"N{N}-r{rows}-equal", rows, N, "equal", off=0))
    out.append(_sm("block", 64, 8, "block", off=0))
    return out


def _addmask_cases():
    out = []
    i = 0
    # every subset of the addends x the three gatings, frames 1 and 3, gains 0 (none) and 0.5, HW cycling over 5, 32, 49
    for adds in itertools.product((0, 1), repeat=3):
        for gate in ("bits", "mask", "none"):
            N, HW = (1, 3)[i % 2], (5, 32, 49)[i % 3]
            out.append(_case("addmask", f"a{''.join(map(str, adds))}-{gate}-N{N}-HW{HW}", adds=adds, gate=gate, N=N, C=3, HW=HW,
                             gain=(0.0, 0.5)[(i // 2) % 2], gate_pad=i % 3))
            i += 1
    # 1-bit rows: HW in {5, 32, 49} x N in {1, 3}, tight rows and rows two words longer than needed
    for HW in (5, 32, 49):
        for N in (1, 3):
            for pad in (0, 2):
                out.append(_case("addmask", f"bits-N{N}-HW{HW}-pad{pad}", adds=(1, 1, 1), gate="bits", N=N, C=4, HW=HW, gain=0.0, gate_pad=pad))
    out.append(_case("addmask", "two-blocks-mask", adds=(1, 0, 1), gate="mask", N=2, C=5, HW=49, gain=0.5, gate_pad=0))     # 490 elements: two blocks of 256
    out.append(_case("addmask", "two-blocks-bits", adds=(0, 1, 1), gate="bits", N=5, C=3, HW=37, gain=0.0, gate_pad=1))     # 555 elements, six words per row
    # the grid-stride loop's second pass: 1 050 441 elements against 4096 x 256 threads
    out.append(_case("addmask", "second-pass-bits", adds=(1, 0, 1), gate="bits", N=3, C=7, HW=50021, gain=0.5, gate_pad=1))
    return out


CASES = tuple(_product_cases() + _softmax_cases() + _addmask_cases())
BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES)
PRODUCT_OPS = ("gemm1", "gemm2", "gemm3")


# ---------------------------------------------------------------------------------------------------------------------------
# views and descriptors of a case
# ---------------------------------------------------------------------------------------------------------------------------
def _view(t_hw, C, gap=0, off=0):
    T, HW = t_hw
    return {"T": T, "HW": HW, "C": C, "nstride": C * HW + gap, "off": off}


def view_vec(v):
    """The launch's vector flag of a view (allocations are 16-byte aligned and FRONT % 4 == 0)."""
    return v["HW"] % 4 == 0 and v["nstride"] % 4 == 0 and v["off"] % 4 == 0


def _view_index(v, clips):
    """Flat positions (clips, C, T * HW) of a view's elements in its allocation, and the allocation's size."""
    i = torch.arange(v["T"] * v["HW"])
    frame = torch.arange(clips).view(-1, 1, 1) * v["T"] + (i // v["HW"]).view(1, 1, -1)
    idx = FRONT + v["off"] + frame * v["nstride"] + torch.arange(v["C"]).view(1, -1, 1) * v["HW"] + (i % v["HW"]).view(1, 1, -1)
    return idx, FRONT + v["off"] + clips * v["T"] * v["nstride"] + 4 * v["nstride"] + 256


def prod_spec(kw):
    form, rows, cols, K, clips = kw["form"], kw["rows"], kw["cols"], kw["K"], kw.get("clips", 1)
    if form == 1:
        Cc, M, N, na = K, rows, cols, rows
    elif form == 2:
        Cc, M, N, na = rows, cols, K, K
    else:
        Cc, M, N, na = rows, K, cols, K
    s = {"form": form, "clips": clips, "Cc": Cc, "M": M, "N": N, "rows": rows, "cols": cols, "K": K,
         "a": _view(kw.get("a", _split(na)), Cc, kw.get("a_gap", 0), kw.get("a_off", 0)), "d_off": kw.get("d_off", 0),
         "scale": float(kw.get("scale", 1.0)), "acc": int(kw.get("acc", 0)), "ksplit": int(kw.get("ksplit", 0))}
    assert s["a"]["T"] * s["a"]["HW"] == na, kw
    if form == 1:
        s["b"] = _view(kw.get("b", _split(N)), Cc, kw.get("b_gap", 0), kw.get("b_off", 0))
        assert s["b"]["T"] * s["b"]["HW"] == N, kw
    else:
        s["c"] = _view(kw.get("c", _split(cols)), Cc, kw.get("c_gap", 0), kw.get("c_off", 0))
        assert s["c"]["T"] * s["c"]["HW"] == cols, kw
    return s


def prod_flags(kw):
    """(a_vec, b_vec or d_vec) as the kernel sets them."""
    s = prod_spec(kw)
    return view_vec(s["a"]), view_vec(s["b"]) if s["form"] == 1 else (s["N"] % 4 == 0 and s["d_off"] % 4 == 0)


def kseg(K, ksplit):
    return K if ksplit <= 1 else ((K + ksplit - 1) // ksplit + 31) // 32 * 32


# ---------------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------------
def _gen(name, salt=0):
    return torch.Generator().manual_seed(zlib.crc32(name.encode()) + salt)


@functools.lru_cache(maxsize=1)
def block_chain():
    """The non-local block at its own ratios in float64, every tensor rounded to float32 where a launch reads it."""
    g = _gen("block-chain")
    rn = lambda *s: torch.randn(*s, generator=g)
    theta, phi, gg, dY = rn(2, 8, 32), rn(2, 8, 8), rn(2, 8, 8), rn(2, 8, 32)
    S = torch.einsum("bci,bcj->bij", theta.double(), phi.double()).float()
    Pm = torch.softmax(S.double(), -1).float()
    dP = torch.einsum("bci,bcj->bij", dY.double(), gg.double()).float()
    Pd, dPd = Pm.double(), dP.double()
    dS = (Pd * (dPd - (dPd * Pd).sum(-1, keepdim=True))).float()
    return {"theta": theta, "phi": phi, "g": gg, "dY": dY, "S": S, "P": Pm, "dP": dP, "dS": dS}


_BLOCK_IN = {"S": ("theta", "phi"), "y": ("g", "P"), "dP": ("dY", "g"), "dg": ("dY", "P"), "dtheta": ("phi", "dS"), "dphi": ("theta", "dS")}


@functools.lru_cache(maxsize=8)
def inputs(case: Case):
    """{name: float32 CPU tensor} in the operation's own shapes (no padding); read-only, shared by run and reference."""
    kw, g = case.kw, _gen(case.id)
    rn = lambda *s: torch.randn(*s, generator=g)
    if case.op in PRODUCT_OPS:
        s = prod_spec(kw)
        clips, Cc, M, N = s["clips"], s["Cc"], s["M"], s["N"]
        na = s["a"]["T"] * s["a"]["HW"]
        inp = {"A": rn(clips, Cc, na), "base": rn(clips, Cc, s["cols"])}
        inp["B" if s["form"] == 1 else "Din"] = rn(clips, Cc, N) if s["form"] == 1 else rn(clips, M, N)
        if kw.get("block"):
            ch = block_chain()
            first, second = _BLOCK_IN[kw["block"]]
            inp["A"], inp["B" if s["form"] == 1 else "Din"] = ch[first], ch[second]
        return inp
    if case.op == "softmax":
        rows, N, kind = kw["rows"], kw["N"], kw["kind"]
        if kind == "block":
            ch = block_chain()
            return {"X": ch["S"].reshape(rows, N), "Pin": ch["P"].reshape(rows, N), "dX": ch["dP"].reshape(rows, N)}
        x = rn(rows, N)
        if kind == "sat":
            # scores spread over +-60, what synthetic weights produce (tests/test_native_classifier.py): nearly one-hot rows
            x = x * (60 / x.abs().max(1, keepdim=True).values.clamp_min(1e-3))
        elif kind == "spike":
            x = x.clamp(-3.5, 3.5)
            x[torch.arange(rows), N - 1 - torch.arange(rows) % N] = 104.0      # one entry 100 above the rest, in the row's LAST trip
        elif kind == "equal":
            x = torch.full((rows, N), 0.7) * (1 + torch.arange(rows).view(-1, 1))
        # the backward's probabilities are an INPUT of their own: the float32 rounding of the float64 softmax of a row of order one (a
        # one-hot P makes P (d - sum d P) vanish and leaves nothing to normalise an error by)
        soft = rn(rows, N) if kind in ("sat", "spike") else x
        return {"X": x.contiguous(), "Pin": torch.softmax(soft.double(), 1).float(), "dX": rn(rows, N)}
    N, C, HW = kw["N"], kw["C"], kw["HW"]
    a = [rn(N, C, HW) for _ in range(3)]
    for t in a:
        t.view(-1)[::11] = -0.0                          # (0 + -0 is +0: the sum starts from +0)
    mask = rn(N, C, HW)
    mask.view(-1)[::5] = 0.0
    mask.view(-1)[2::7] = -0.0
    return {"a0": a[0], "a1": a[1], "a2": a[2], "mask": mask, "keep": torch.rand(N, C, HW, generator=g) < 0.6}


# ---------------------------------------------------------------------------------------------------------------------------
# references: plain torch in `dt` (float64: the reference; float32: its own error e32)
# ---------------------------------------------------------------------------------------------------------------------------
def _slack(n):
    return ("exact", torch.full((n,), SENTINEL))


def _flag():
    return ("exact", torch.ones(1, dtype=torch.int32))


def _dense_size(n, off):
    return FRONT + off + n + 256


def _ref_prod(case, inp, dt):
    kw, s = case.kw, prod_spec(case.kw)
    A = inp["A"].to(dt)
    out = {"inputs_unchanged": _flag()}
    if s["form"] == 1:
        v = torch.einsum("bci,bcj->bij", A, inp["B"].to(dt))                     # D[i][j] = scale * sum_c A[c][i] B[c][j]
        if s["scale"] != 1.0:
            v = torch.tensor(s["scale"], dtype=torch.float32).to(dt) * v
        out["D"] = ("tensor", v)
        out["D_slack"] = _slack(_dense_size(v.numel(), s["d_off"]) - v.numel())
        return out
    D = inp["Din"].to(dt)
    v = torch.einsum("bcj,bij->bci", A, D) if s["form"] == 2 else torch.einsum("bci,bij->bcj", A, D)
    if s["acc"]:
        v = inp["base"].to(dt) + v
    out["C"] = ("tensor", v)
    out["C_slack"] = _slack(_view_index(s["c"], s["clips"])[1] - v.numel())
    if s["ksplit"] > 1:
        out["part_slack"] = _slack(FRONT + 256)
    if "empty-segment" in case.id:
        out["C_has_the_bits_of_two_segments"] = _flag()
    return out


def _softmax_off(kw):
    return kw.get("off", 0)


def _ref_softmax(case, inp, dt):
    kw = case.kw
    rows, N = kw["rows"], kw["N"]
    x = inp["X"].to(dt)
    Pm = torch.softmax(x, 1)
    # the backward by autograd: dS = d/dS sum(softmax(S) o dP) at the point whose softmax is Pin -- log Pin, Pin's own logits
    pin = inp["Pin"].to(dt)
    z = torch.log(pin).requires_grad_(True)
    sm = torch.softmax(z, 1)
    (sm * inp["dX"].to(dt)).sum().backward()
    dS = z.grad.detach()
    n_slack = _dense_size(rows * N, _softmax_off(kw)) - rows * N
    out = {"P": ("tensor", Pm), "P_slack": _slack(n_slack), "dS": ("tensor", dS), "dS_slack": _slack(n_slack), "inputs_unchanged": _flag()}
    if N == 1:                           # P = 1 exactly, and dS = 1 * (d - d) = 0 exactly: nothing to normalise an error by
        out["P"] = ("exact", torch.ones(rows, 1))
        out["dS"] = ("exact", torch.zeros(rows, 1))
    elif kw["kind"] == "equal":
        out["P"] = ("exact", torch.full((rows, N), 1.0 / N, dtype=torch.float64).float())
    return out


def _ref_addmask(case, inp, dt):
    # exact in every precision: the float32 sum in the kernel's order, the gate, the gain -- each step one correctly rounded operation
    kw = case.kw
    N, C, HW = kw["N"], kw["C"], kw["HW"]
    v = torch.zeros(N, C, HW, dtype=torch.float32)
    for i in range(3):
        if kw["adds"][i]:
            v = v + inp[f"a{i}"]
    if kw["gate"] == "bits":
        v = torch.where(inp["keep"], v, torch.zeros(()))
    elif kw["gate"] == "mask":
        v = torch.where(inp["mask"] > 0, v, torch.zeros(()))
    if kw["gain"] != 0.0:
        v = torch.tensor(kw["gain"], dtype=torch.float32) * v
    return {"out": ("exact", v), "out_slack": _slack(_view_index(_addmask_views(kw)["out"], 1)[1] - v.numel()), "inputs_unchanged": _flag()}


def _addmask_views(kw):
    """Distinct frame strides per operand: gaps 1, 0, 3, 6 and 2 floats for out, a0, a1, a2 and the mask."""
    N, C, HW = kw["N"], kw["C"], kw["HW"]
    return {n: _view((N, C * HW), 1, gap, off) for n, gap, off in (("out", 1, 0), ("a0", 0, 1), ("a1", 3, 0), ("a2", 6, 2), ("mask", 2, 0))}


_REFS = {"gemm1": _ref_prod, "gemm2": _ref_prod, "gemm3": _ref_prod, "softmax": _ref_softmax, "addmask": _ref_addmask}


def evaluate(case: Case, dt=torch.float64):
    return _REFS[case.op](case, inputs(case), dt)


@functools.lru_cache(maxsize=8)
def reference(case: Case):
    return evaluate(case)


def error(got, want):
    """The error of one `tensor` output, normalised as its bound is: max|got - want| / max|want|."""
    got, want = got.double(), want.double()
    assert got.shape == want.shape, (tuple(got.shape), tuple(want.shape))
    if not bool(torch.isfinite(got).all()):
        return float("inf")
    return float((got - want).abs().max()) / float(want.abs().max())


def fp32_errors(case: Case):
    """{output: error of the float32 CPU evaluation of the reference against its float64 evaluation} for the `tensor` outputs."""
    r64, r32 = reference(case), evaluate(case, torch.float32)
    return {name: error(r32[name][1], want) for name, (kind, want) in r64.items() if kind == "tensor"}


def same_bits(a, b):
    if a.dtype.is_floating_point:
        a, b = a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)
    return a.shape == b.shape and bool(torch.equal(a, b))


def bound(e32):
    return max(FLOOR, 4 * e32)


def check(case: Case, got, e32, report=None):
    """Hold every output of `got` to its bound; `e32`: this case's entry of the committed fixture.  Returns {output: error}."""
    ref = reference(case)
    assert set(got) == set(ref), (case.id, sorted(got), sorted(ref))
    assert set(e32) == {n for n, (k, _) in ref.items() if k == "tensor"}, (case.id, sorted(e32))
    errs = {}
    for name, (kind, want) in ref.items():
        g = got[name]
        if kind == "exact":
            assert g.dtype == want.dtype and same_bits(g, want), (
                f"{case.id}: {name} differs from the exact reference at "
                f"{int((g.contiguous().view(torch.int32) != want.contiguous().view(torch.int32)).sum()) if g.shape == want.shape else 'every'} of {want.numel()} element(s)")
            continue
        assert float(want.abs().max()) > 0, (case.id, name)
        errs[name] = error(g, want)
        if report is not None:
            report(f"{case.id:44s} {name:9s} error {errs[name]:.3g}  bound {bound(e32[name]):.3g}  (e32 {e32[name]:.3g})")
    for name, err in errs.items():
        assert err <= bound(e32[name]), f"{case.id}: {name} error {err:.3g} > bound {bound(e32[name]):.3g} = max({FLOOR:g}, 4 * {e32[name]:.3g})"
    return errs


# ---------------------------------------------------------------------------------------------------------------------------
# running a case through the C entries
# ---------------------------------------------------------------------------------------------------------------------------
class _Ctx:
    def __init__(self, eng):
        self.eng, self.capi, self.cuda = eng, eng.capi, eng.device.type == "cuda"
        if not getattr(self.capi, "_nl_bound", False):
            lib.bind(self.capi, lib._NL_PROTOS)
            self.capi._nl_bound = True
        self.inputs = []

    def call(self, name, *args):
        lib.check(self.capi, getattr(self.capi, name)(*args, self.eng.stream()))

    def sync(self):
        if self.cuda:
            torch.cuda.synchronize()

    def unchanged(self):
        return torch.tensor([int(all(same_bits(b.before, b.host()) for b in self.inputs))], dtype=torch.int32)


class _Buf:
    """One allocation: `fill` everywhere, `data` scattered to the flat positions `idx`.  An input (fill NaN) is remembered by its
    context, which compares its bits after the launch."""

    def __init__(self, cx, size, idx, data, fill, dtype=torch.float32):
        host = torch.full((size,), fill, dtype=dtype)
        self.idx = idx.reshape(-1)
        assert self.idx.numel() == 0 or (int(self.idx.min()) >= 0 and int(self.idx.max()) < size and self.idx.unique().numel() == self.idx.numel())
        host[self.idx] = data.reshape(-1).to(dtype)
        self.cx, self.shape, self.size = cx, tuple(idx.shape), size
        self.dev = host.to(cx.eng.device) if cx.cuda else host
        assert self.dev.data_ptr() % 16 == 0
        if fill != SENTINEL:
            self.before = host.clone()
            cx.inputs.append(self)

    def addr(self, floats=0):
        return self.dev.data_ptr() + 4 * floats

    def host(self):
        self.cx.sync()
        return self.dev.detach().cpu().clone()

    def collect(self, out, name, shape=None):
        buf = self.host()
        out[name] = buf[self.idx].reshape(shape if shape is not None else self.shape).contiguous()
        keep = torch.ones(self.size, dtype=torch.bool)
        keep[self.idx] = False
        out[name + "_slack"] = buf[keep]


def _view_buf(cx, v, clips, data, fill):
    idx, size = _view_index(v, clips)
    return _Buf(cx, size, idx, data, fill)


def _dense_buf(cx, data, off, fill):
    return _Buf(cx, _dense_size(data.numel(), off), FRONT + off + torch.arange(data.numel()).reshape(data.shape), data, fill)


def _act(buf, v):
    return lib.NlAct(buf.addr(FRONT + v["off"]), v["nstride"], v["T"], v["HW"])


def prod_desc(s, bufs):
    """The descriptor of the spec `s` over `bufs`."""
    d = lib.NlGemmDesc()
    d.form, d.clips, d.Cc, d.M, d.N = s["form"], s["clips"], s["Cc"], s["M"], s["N"]
    d.A = _act(bufs["A"], s["a"])
    d.scale, d.accumulate, d.ksplit = s["scale"], s["acc"], s["ksplit"]
    if s["form"] == 1:
        d.B = _act(bufs["B"], s["b"])
        d.D = bufs["D"].addr(FRONT + s["d_off"])
    else:
        c = s["c"]
        d.Din = bufs["Din"].addr(FRONT + s["d_off"])
        d.C, d.c_nstride, d.c_T, d.c_HW = bufs["C"].addr(FRONT + c["off"]), c["nstride"], c["T"], c["HW"]
        if "part" in bufs:
            d.part = bufs["part"].addr(FRONT)
    return d


def prod_bufs(cx, s, inp):
    clips, form = s["clips"], s["form"]
    bufs = {"A": _view_buf(cx, s["a"], clips, inp["A"], NAN)}
    if form == 1:
        bufs["B"] = _view_buf(cx, s["b"], clips, inp["B"], NAN)
        bufs["D"] = _dense_buf(cx, torch.full((clips, s["M"], s["N"]), NAN), s["d_off"], SENTINEL)
    else:
        bufs["Din"] = _dense_buf(cx, inp["Din"], s["d_off"], NAN)
        init = inp["base"] if s["acc"] else torch.full((clips, s["Cc"], s["cols"]), NAN)
        bufs["C"] = _view_buf(cx, s["c"], clips, init, SENTINEL)
        if s["ksplit"] > 1:
            bufs["part"] = _dense_buf(cx, torch.full((clips, s["ksplit"], s["Cc"], s["cols"]), NAN), 0, SENTINEL)
    return bufs


def _launch_prod(cx, s, inp):
    bufs = prod_bufs(cx, s, inp)
    d = prod_desc(s, bufs)
    cx.call("i2v_nl_gemm_f32", ctypes.byref(d))
    out = {}
    bufs["D" if s["form"] == 1 else "C"].collect(out, "D" if s["form"] == 1 else "C")
    if "part" in bufs:
        part = {}
        bufs["part"].collect(part, "part")
        out["part_slack"] = part["part_slack"]
    out["inputs_unchanged"] = cx.unchanged()
    return out


def _run_prod(cx, case, inp):
    s = prod_spec(case.kw)
    out = _launch_prod(cx, s, inp)
    if "empty-segment" in case.id:
        two = _launch_prod(_Ctx(cx.eng), dict(s, ksplit=2), inp)
        out["C_has_the_bits_of_two_segments"] = torch.tensor([int(same_bits(out["C"], two["C"]))], dtype=torch.int32)
    return out


def run_clip_alone(engine, case: Case, b):
    """Clip `b` of a product case as a launch of its own: {"D" or "C": (1, ...), ...}."""
    inp = {k: v[b:b + 1] for k, v in inputs(case).items()}
    return _launch_prod(_Ctx(engine), dict(prod_spec(case.kw), clips=1), inp)


def _run_softmax(cx, case, inp):
    kw = case.kw
    rows, N, off = kw["rows"], kw["N"], _softmax_off(kw)
    X = _dense_buf(cx, inp["X"], off, SENTINEL)
    cx.call("i2v_nl_softmax_rows_f32", X.addr(FRONT + off), None, rows, N, 0)
    Pin = _dense_buf(cx, inp["Pin"], off, NAN)
    dX = _dense_buf(cx, inp["dX"], off, SENTINEL)
    cx.call("i2v_nl_softmax_rows_f32", dX.addr(FRONT + off), Pin.addr(FRONT + off), rows, N, 1)
    out = {}
    X.collect(out, "P")
    dX.collect(out, "dS")
    out["inputs_unchanged"] = cx.unchanged()
    return out


def gate_words(kw):
    return (kw["N"] * kw["HW"] + 31) // 32 + kw["gate_pad"]


def _run_addmask(cx, case, inp):
    kw = case.kw
    N, C, HW = kw["N"], kw["C"], kw["HW"]
    views = _addmask_views(kw)
    d = lib.NlAddMaskDesc()
    ob = _view_buf(cx, views["out"], 1, torch.full((N, C * HW), NAN).reshape(1, 1, -1), SENTINEL)
    d.out, d.out_nstride = ob.addr(FRONT + views["out"]["off"]), views["out"]["nstride"]
    keep = [ob]
    for i in range(3):
        if kw["adds"][i]:
            v = views[f"a{i}"]
            b = _view_buf(cx, v, 1, inp[f"a{i}"].reshape(1, 1, -1), NAN)
            d.a[i], d.a_nstride[i] = b.addr(FRONT + v["off"]), v["nstride"]
            keep.append(b)
    if kw["gate"] == "mask":
        v = views["mask"]
        b = _view_buf(cx, v, 1, inp["mask"].reshape(1, 1, -1), NAN)
        d.mask, d.mask_nstride = b.addr(FRONT + v["off"]), v["nstride"]
        keep.append(b)
    elif kw["gate"] == "bits":
        # rows per channel of gate_words 32-bit words, bit n * HW + i; the unused bits and words are SET, so a wrong index that lands
        # on one keeps an element the reference zeroes
        W = gate_words(kw)
        bits = torch.ones(C, W * 32, dtype=torch.bool)
        bits[:, :N * HW] = inp["keep"].permute(1, 0, 2).reshape(C, N * HW)
        words = (bits.view(C, W, 32).to(torch.int64) << torch.arange(32)).sum(-1)
        words = torch.where(words >= 2 ** 31, words - 2 ** 32, words).to(torch.int32)
        b = _Buf(cx, FRONT + C * W + 64, FRONT + torch.arange(C * W), words, -1, dtype=torch.int32)
        d.gate, d.gate_stride = b.addr(FRONT), W
        keep.append(b)
    d.N, d.C, d.HW, d.gain = N, C, HW, kw["gain"]
    cx.call("i2v_nl_addmask_f32", ctypes.byref(d))
    out = {}
    ob.collect(out, "out", (N, C, HW))
    out["inputs_unchanged"] = cx.unchanged()
    del keep
    return out


_RUNS = {"gemm1": _run_prod, "gemm2": _run_prod, "gemm3": _run_prod, "softmax": _run_softmax, "addmask": _run_addmask}


def run(engine, case: Case):
    """The case through the C entries of `engine.capi`: {name: CPU tensor} over the names of `reference(case)`."""
    return _RUNS[case.op](_Ctx(engine), case, inputs(case))


# ---------------------------------------------------------------------------------------------------------------------------
# refusals: (label, the entry the message names, thunk returning the status); `keep` holds the buffers
# ---------------------------------------------------------------------------------------------------------------------------
def refusals(engine):
    cx = _Ctx(engine)
    st = cx.eng.stream
    thunks, outs = [], []
    G, SM, AM = cx.capi.i2v_nl_gemm_f32, cx.capi.i2v_nl_softmax_rows_f32, cx.capi.i2v_nl_addmask_f32
    keep = []
    for cid in ("gemm1-flag-all-set", "gemm2-split2-K100-accumulate", "gemm3-flag-all-set"):
        case = BY_ID[cid]
        s = prod_spec(case.kw)
        bufs = prod_bufs(cx, dict(s, acc=0), inputs(case))
        keep.append(bufs)
        outs.append(bufs["D" if s["form"] == 1 else "C"])
        if "part" in bufs:
            outs.append(bufs["part"])

        def thunk(edit, s=s, bufs=bufs):
            def go():
                d = prod_desc(s, bufs)
                edit(d)
                return G(ctypes.byref(d), st())
            return go
        f = s["form"]

        def sets(obj=None, **kv):
            def edit(d):
                for k, v in kv.items():
                    setattr(getattr(d, obj) if obj else d, k, v)
            return edit
        thunks += [(f"form {f}: form 0", thunk(sets(form=0))), (f"form {f}: form 4", thunk(sets(form=4))),
                   (f"form {f}: A null", thunk(sets("A", p=None))), (f"form {f}: A.HW 0", thunk(sets("A", HW=0))),
                   (f"form {f}: A.T -1", thunk(sets("A", T=-1))), (f"form {f}: A of another count", thunk(sets("A", T=s["a"]["T"] + 1)))]
        if f == 1:
            thunks += [("form 1: B null", thunk(sets("B", p=None))), ("form 1: B.HW 0", thunk(sets("B", HW=0))), ("form 1: B.T 0", thunk(sets("B", T=0))),
                       ("form 1: N != B.T * B.HW", thunk(sets(N=s["N"] + 1))), ("form 1: M != A.T * A.HW", thunk(sets(M=s["M"] - 1))),
                       ("form 1: D null", thunk(sets(D=None))), ("form 1: no channels", thunk(sets(Cc=0)))]
        else:
            thunks += [(f"form {f}: Din null", thunk(sets(Din=None))), (f"form {f}: C null", thunk(sets(C=None))),
                       (f"form {f}: c_HW 0", thunk(sets(c_HW=0))), (f"form {f}: c_T 0", thunk(sets(c_T=0))),
                       (f"form {f}: the output view of another count", thunk(sets(c_T=s["c"]["T"] + 1))),
                       (f"form {f}: the reduced count != A.T * A.HW", thunk(sets(**{"N" if f == 2 else "M": s["K"] + 4}))),
                       (f"form {f}: ksplit 2 without part", thunk(sets(ksplit=2, part=None)))]
    thunks = [(label, "i2v_nl_gemm_f32", t) for label, t in thunks]
    thunks.append(("gemm: null descriptor", "i2v_nl_gemm_f32", lambda: G(None, st())))
    x = _dense_buf(cx, torch.full((5, 9), NAN), 0, SENTINEL)
    pb = _dense_buf(cx, torch.full((5, 9), 0.25), 0, NAN)
    outs.append(x)
    X, Pp = x.addr(FRONT), pb.addr(FRONT)
    thunks += [(label, "i2v_nl_softmax_rows_f32", t) for label, t in (
        ("softmax: mode 2", lambda: SM(X, Pp, 5, 9, 2, st())), ("softmax: mode -1", lambda: SM(X, Pp, 5, 9, -1, st())),
        ("softmax: mode 1 without P", lambda: SM(X, None, 5, 9, 1, st())), ("softmax: N 0", lambda: SM(X, Pp, 5, 0, 0, st())),
        ("softmax: N -3", lambda: SM(X, Pp, 5, -3, 1, st())), ("softmax: X null", lambda: SM(None, Pp, 5, 9, 0, st())))]
    o = _dense_buf(cx, torch.full((2, 3, 5), NAN), 0, SENTINEL)
    a0 = _dense_buf(cx, torch.ones(2, 3, 5), 0, NAN)
    gate = _Buf(cx, FRONT + 64, FRONT + torch.arange(3), torch.full((3,), -1), -1, dtype=torch.int32)
    outs.append(o)

    def am(**kv):
        def go():
            d = lib.NlAddMaskDesc()
            d.out, d.out_nstride, d.N, d.C, d.HW = o.addr(FRONT), 15, 2, 3, 5
            d.a[0], d.a_nstride[0] = a0.addr(FRONT), 15
            for k, v in kv.items():
                setattr(d, k, v)
            return AM(ctypes.byref(d), st())
        return go
    thunks += [(label, "i2v_nl_addmask_f32", t) for label, t in (
        ("addmask: out null", am(out=None)), ("addmask: C 0", am(C=0)), ("addmask: HW -1", am(HW=-1)),
        ("addmask: gate rows of 0 words", am(gate=gate.addr(FRONT), gate_stride=0)),
        ("addmask: gate rows of 32 bits for 2 x 49", am(gate=gate.addr(FRONT), gate_stride=1, HW=49)),
        ("addmask: null descriptor", lambda: AM(None, st())))]
    # nothing to do: 0, and nothing written either
    d0 = prod_desc(prod_spec(BY_ID["gemm1-flag-all-set"].kw), keep[0])
    d0.clips = 0
    nothing = [("gemm: clips 0", lambda: G(ctypes.byref(d0), st())), ("softmax: rows 0", lambda: SM(X, Pp, 0, 9, 0, st())),
               ("softmax: rows -2", lambda: SM(X, Pp, -2, 9, 1, st())), ("addmask: N 0", am(N=0))]

    def untouched():
        for b in outs:
            got = b.host()
            want = torch.full((b.size,), SENTINEL)
            want[b.idx] = NAN
            if not same_bits(got, want):
                return False
        return True
    keep += [x, pb, o, a0, gate]
    return thunks, nothing, untouched, keep
