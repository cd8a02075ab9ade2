"""TEST INFRASTRUCTURE: the case table of the launches every transformer-stack surrogate shares (csrc/i2v_vit.hip: `vit_gemm`,
`vit_layernorm(_bwd)`, `vit_softmax(_bwd)`, `vit_patchify`, `vit_assemble`; scalar twins in csrc/i2v_xf_host.h), with input generators
and a float64 reference per case.  tests/test_xf_kernels_cpu.py runs the cases whose launches have a host twin (ops `gemm`, `ln`,
`patchify`) on the host simulation, tests/test_gpu_xf_kernels.py runs all of them (also `softmax`, `attn`, `embed`) on the device.

`run(engine, case)` calls the C entries (include/i2v_xf_launch.h; for attention and token assembly include/i2v_vit.h) through
`engine.capi` with buffers on the engine's device and returns {name: CPU tensor}.  `reference(case)` returns {name: (kind, tensor)} over
the SAME names: nothing an entry writes is left unchecked.

Kinds and bounds (`check`), the loop table's rule:
  tensor   max|got - want| <= max(2e-6, 4 e32) * max|want|      (2e-6: tests/loop_cases.py's `tensor` floor; 4: DESIGN.md section 14)
  exact    equal bits: data movement (patchify, the prefix rows of assemble where their pos rows are zero), untouched slack, the
           exactly uniform softmax row, the probabilities the softmax backward must not touch
e32 is the error of the same reference evaluated in float32 by plain torch on the CPU, normalised the same way and committed as
tests/golden/xf_fp32_cpu_errors.json (tests/make_xf_fixtures.py).

Buffers.  Every operand is a view into a larger flat allocation: FRONT = 128 floats ahead of it (+ `off`: 1 misaligns the base by 4
bytes), its rows at their leading dimension, and a tail of 129 rows + 256 floats after its last row -- a whole 128-wide tile more than
any launch here may touch, so an overrun by a wrong tail lands inside the allocation.  Everything of an OUTPUT allocation that is not
an addressed element (the floats ahead of the view, the columns past the row's width, the tail) is SENTINEL and must come back bit for
bit (`<name>_slack`); its addressed elements start as NaN (as R where R aliases C, as the addend where dx aliases it).  Everything of
an INPUT allocation that is not an addressed element is NaN: a stray read poisons a checked output.

Branch arithmetic of csrc/i2v_vit.hip (re-derive the comments at the cases when any of it changes):
  vit_gemm_kernel<AK, BK>: AK = A contiguous along K (a_sk == 1), else along M; BK = B contiguous along K (b_sk == 1), else along N.
    One block of 256 threads = 4 waves (wm = wave / 2, wn = wave % 2) owns a TM x TN = 128 x 128 tile of C and walks K in chunks of
    KC = 16, double-buffered: ceil(K / 16) chunks; with one chunk nothing is prefetched, with three the LDS buffer parity wraps.
    Fetch, two pieces h = 0, 1 per thread t: an operand contiguous along K gives row r4 + 64 h (r4 = t / 4) and four k from
    k4 = 4 (t % 4), lim = K - k; one contiguous along M / N gives k = t / 32 + 8 h and four rows from 4 (t % 32), lim = M - m or N - n.
    A quad is one float4 load when lim >= 4 AND the operand's flag (a_vec, b_vec) is set, else min(lim, 4) scalar loads, zero-filled.
    MFMA 32x32x2: step s multiplies k = 2 s + lk (lk = lane / 32): with K odd the lk = 1 half of the last step runs on zero fill.
    Epilogue: row m = m0 + 64 wm + 32 i + lane % 32, column quads n = n0 + 64 wn + 32 j + 8 q + 4 lk (i, j in 0..1, q in 0..3),
    lim = N - n: R and H are read and C and C2 written as float4 when lim >= 4 AND c_vec, else min(lim, 4) scalars; bias likewise
    under bias_vec.  Edges: 32 (an MFMA fragment), 64 (a wave), 128 (the tile); 130 = two tiles with two rows / columns in the second.
    vit_gemm sets  x_vec = base 16-byte aligned, leading dimension % 4 == 0, x_bo % 4 == 0, x_bi % 4 == 0  for x = a, b, c, and c_vec
    also needs R, C2 and H (where given) aligned; bias_vec = bias aligned.  Batch b = outer * nb_in + inner on blockIdx.y (<= 65535).
  Row kernels (LayerNorm forward / backward, softmax forward / backward): 4 rows per block of 256 threads, one wave per row; a wave
    walks its row in float4 steps of stride 256 floats (a second trip from 257 floats: C = 260, 772; N4 = 260, 1024) or, scalar, in
    steps of 64 (a second trip from C = 65; 13 trips at C = 770).  LayerNorm is float4 only when C % 4 == 0 and x, out, gamma, beta (backward: dy, x,
    gamma, dx, add0, add1) are all aligned; softmax is float4 over N4 = N & ~3 and scalar over the tail [N4, N) from column N4 + lane.
  vit_patchify / vit_assemble: one thread per float4, min(ceil(quads / 256), 65536) blocks -- the grid-stride second pass starts
    above 16.7 M quads, a 268 MB operand, which a seconds-long test cannot put through a float64 reference: left out.
"""
import ctypes
import functools
import math
import zlib
from dataclasses import dataclass
from typing import Tuple

import torch

from i2v_amd import lib

SENTINEL = -123.25
FLOOR = 2e-6
FRONT = 128
P = ctypes.c_void_p
NULL = P(0)
HOST_OPS = ("gemm", "ln", "patchify")          # the ops whose launches all have a host twin
LN_EPS = 1e-6


@dataclass(frozen=True)
class Case:
    id: str
    op: str
    items: Tuple[Tuple[str, object], ...]

    @property
    def kw(self):
        return dict(self.items)


def _case(op, id, **kw):
    return Case(f"{op}-{id}", op, tuple(sorted(kw.items())))


def _r4(v):
    return (v + 3) // 4 * 4


# ---------------------------------------------------------------------------------------------------------------------------
# the table
# ---------------------------------------------------------------------------------------------------------------------------
EDGES = (1, 3, 31, 32, 33, 63, 64, 65, 127, 128, 129, 130)
KS = (1, 2, 3, 15, 16, 17, 32, 33, 48)
LAYOUTS = (("k", "k"), ("k", "n"), ("m", "k"), ("m", "n"))        # (A contiguous along, B contiguous along)
EPI = {"plain": 0, "gelu": 1, "gelu_bwd": 2}


def _g(id, M, N, K, la="k", lb="k", **kw):
    return _case("gemm", id, M=M, N=N, K=K, la=la, lb=lb, **kw)


def _gemm_cases():
    out = []
    # every instance with every operand float4 (vec: aligned bases, leading dimensions rounded up to 4) and with every operand scalar
    # (bases one float in, leading dimensions 4 j + 1); 37 x 35 x 19: tails of 1 and 3 in M and N, two chunks with a tail of 3
    for la, lb in LAYOUTS:
        for vec in (True, False):
            out.append(_g(f"A{la}-B{lb}-{'vec' if vec else 'scalar'}", 37, 35, 19, la, lb, vec=vec, bias=True))
    # tile edges cycled over layout, K and path: N runs through EDGES in steps of 5 (coprime with 12), so every value occurs twice in M
    # and twice in N over the 24 cases, once float4 and once scalar
    for i in range(24):
        la, lb = LAYOUTS[i % 4]
        M, N, K = EDGES[i % 12], EDGES[(5 * i + 7) % 12], KS[(i + i // 12) % 9]
        out.append(_g(f"edge-M{M}-N{N}-K{K}-A{la}-B{lb}-{'vec' if i < 12 else 'scalar'}", M, N, K, la, lb, vec=i < 12, bias=bool(i & 1), R="sep" if i % 3 == 0 else None))
    # the K loop: one chunk without a prefetch (1, 2, 3, 15, 16), two (17, 32), three (33, 48: the buffer parity wraps), odd K (the lk
    # half on zero fill), chunk tails; 33 x 31: one row past a fragment, one column short of one
    for i, K in enumerate(KS):
        for vec in (True, False):
            la, lb = LAYOUTS[(i + (0 if vec else 2)) % 4]
            out.append(_g(f"K{K}-A{la}-B{lb}-{'vec' if vec else 'scalar'}", 33, 31, K, la, lb, vec=vec))
    # the vector flags one at a time; the base case keeps all four set.  36 x 40 x 20 has no tail, so every quad of a flagged operand
    # is a float4 and every quad of the unflagged one four scalars.  (outer, inner) = (2, 2) where a batch stride is the switch
    out.append(_g("flags-all-set", 36, 40, 20, bias=True, R="sep"))
    for name, kw in [("a-ld", dict(a_ld=21)), ("a-base", dict(a_off=1)), ("a-bi6", dict(outer=2, inner=2, a_bi=22)),
                     ("a-bo", dict(outer=2, inner=2, a_box=2)),
                     ("b-ld", dict(b_ld=23)), ("b-base", dict(b_off=1)), ("b-bi6", dict(outer=2, inner=2, b_bi=26)),
                     ("b-bo", dict(outer=2, inner=2, b_box=6)),
                     ("c-ld", dict(c_ld=42)), ("c-base", dict(c_off=1)), ("c-bi", dict(outer=2, inner=2, c_bi=42)),
                     ("c-bo", dict(outer=2, inner=2, c_box=1)),
                     ("c-aligned-R-not", dict(R="sep", r_off=1)), ("c-aligned-R-off2", dict(R="sep", r_off=2, bias=True)),
                     ("c-aligned-C2-not", dict(mode="gelu", c2_off=1)),
                     ("c-aligned-H-not", dict(mode="gelu_bwd", h_off=3)), ("bias-not-c-vec", dict(bias=True, bias_off=1)),
                     ("bias-off2-R", dict(bias=True, bias_off=2, R="sep"))]:
        out.append(_g("flag-" + name, 36, 40, 20, **kw))
    for la, lb, name, kw in [("m", "k", "a-ld", dict(a_ld=38)), ("m", "k", "a-base", dict(a_off=3)), ("k", "n", "b-ld", dict(b_ld=41)),
                             ("k", "n", "b-base", dict(b_off=2)), ("m", "n", "a-bi", dict(outer=2, inner=3, a_bi=38)),
                             ("m", "n", "b-bi", dict(outer=2, inner=3, b_bi=42))]:
        out.append(_g(f"flag-A{la}-B{lb}-{name}", 36, 40, 20, la, lb, **kw))
    # a head width of 6 as the inner batch stride (heads 3, dh 6: q k^T, P v and dS^T q as attention lays them out)
    out.append(_g("head6-qk", 5, 5, 6, "k", "k", outer=2, inner=3, a_bi=6, b_bi=6, alpha=0.40824829046386307))
    out.append(_g("head6-pv", 5, 6, 5, "k", "n", outer=2, inner=3, b_bi=6, c_bi=6))
    out.append(_g("head6-dk", 5, 6, 5, "m", "n", outer=2, inner=3, b_bi=6, c_bi=6))
    # tails under a set flag: the padding a too-wide load would read is NaN, the padding a too-wide store would write is SENTINEL
    for r in (1, 2, 3):
        out.append(_g(f"tail-N{4 + r}-ldc8", 9, 4 + r, 8, bias=True, R="sep"))                 # N % 4 = r, c_sm = 8: the probability-matrix situation
        out.append(_g(f"tail-N{64 + r}-gelu", 5, 64 + r, 8, mode="gelu", bias=True))
        out.append(_g(f"tail-N{32 + r}-gelu-bwd", 5, 32 + r, 8, mode="gelu_bwd"))
        out.append(_g(f"tail-K{16 + r}-AkBk", 6, 7, 16 + r))                                    # K % 4 = r, leading dimensions 20
        out.append(_g(f"tail-K{r}-AkBk", 6, 7, r))
        out.append(_g(f"tail-M{4 + r}-Am", 4 + r, 9, 8, "m", "k"))                              # M % 4 = r with A along M
        out.append(_g(f"tail-M{128 + r}-Am", 128 + r, 5, 5, "m", "n"))
        out.append(_g(f"tail-N{4 + r}-Bn", 9, 4 + r, 8, "k", "n"))                              # N % 4 = r with B along N
        out.append(_g(f"tail-N{128 + r}-Bn", 3, 128 + r, 5, "m", "n"))
    # epilogues, float4 and scalar: alpha 1, 0.125 and 0.3 (no power of two); bias alone, R alone, both; GELU with bias and R (C is the
    # pre-activation, C2 = gelu(C)); GELU backward with H across (-6, 6) and zeros
    for vec in (True, False):
        v = "vec" if vec else "scalar"
        out.append(_g(f"epi-plain-{v}", 34, 30, 17, vec=vec))
        out.append(_g(f"epi-alpha0.125-{v}", 34, 30, 17, vec=vec, alpha=0.125))
        out.append(_g(f"epi-alpha0.3-{v}", 34, 30, 17, vec=vec, alpha=0.3, bias=True, R="sep"))
        out.append(_g(f"epi-bias-{v}", 34, 30, 17, vec=vec, bias=True))
        out.append(_g(f"epi-R-{v}", 34, 30, 17, vec=vec, R="sep"))
        out.append(_g(f"epi-bias-R-{v}", 34, 30, 17, vec=vec, bias=True, R="sep"))
        out.append(_g(f"epi-gelu-bias-R-{v}", 34, 30, 17, vec=vec, mode="gelu", bias=True, R="sep"))
        out.append(_g(f"epi-gelu-bwd-{v}", 34, 30, 17, "k", "n", vec=vec, mode="gelu_bwd"))
        out.append(_g(f"epi-gelu-bwd-alpha-{v}", 34, 30, 17, "k", "n", vec=vec, mode="gelu_bwd", alpha=0.3))
    # R == C in place: four tiles, and a scalar-store shape (c_sm = 27)
    out.append(_g("inplace-130x130x33", 130, 130, 33, R="inplace", bias=True))
    out.append(_g("inplace-scalar-33x27x27", 33, 27, 27, R="inplace", bias=True, c_ld=27, a_ld=27, b_ld=27))
    out.append(_g("inplace-gelu-65x36x16", 65, 36, 16, R="inplace", mode="gelu"))
    # XCiT's first stem layer: linear with K = 27 (all-scalar loads), its backward with N = 27 columns (all-scalar stores)
    out.append(_g("stem-linear-K27", 50, 16, 27, a_ld=27, b_ld=27, bias=True, mode="gelu"))
    out.append(_g("stem-linear-bwd-N27", 50, 27, 16, "k", "n", b_ld=27, c_ld=27))
    # batch: outer x inner with distinct strides as attention lays heads out (a head is a column slice of a shared row); nb_in = 0
    # (treated as 1); one B for every batch (both strides 0)
    for vec in (True, False):
        v = "vec" if vec else "scalar"
        out.append(_g(f"batch-2x3-qk-{v}", 7, 7, 8, "k", "k", vec=vec, outer=2, inner=3, alpha=0.125))
        out.append(_g(f"batch-2x3-pv-{v}", 7, 8, 7, "k", "n", vec=vec, outer=2, inner=3))
        out.append(_g(f"batch-2x3-dk-{v}", 7, 8, 7, "m", "n", vec=vec, outer=2, inner=3, R="sep"))
        out.append(_g(f"batch-3x2-dv-{v}", 9, 12, 5, "m", "k", vec=vec, outer=3, inner=2, bias=True))
        out.append(_g(f"batch-nbin0-{v}", 33, 9, 17, vec=vec, outer=3, inner=1, nb_in0=True))
        out.append(_g(f"batch-B-shared-{v}", 9, 33, 17, "k", "n", vec=vec, outer=2, inner=2, b_shared=True, bias=True))
    out.append(_g("batch-5-two-tiles", 129, 5, 3, outer=5, inner=1))
    # nothing to do: returns 0 and writes nothing
    for name, val in (("M", 0), ("N", 0), ("batch", 0), ("M", -1), ("N", -3), ("batch", -2)):
        out.append(_g(f"degenerate-{name}{val}", 5, 6, 7, degenerate=(name, val)))
    return out


# the batch-invariance cases: batch b on its own has the bits it has inside the batched launch
INVARIANCE = ("gemm-batch-2x3-qk-vec", "gemm-batch-2x3-dk-scalar", "gemm-batch-2x3-pv-vec", "gemm-head6-pv")

LN_ROWS = (1, 3, 4, 5, 9)
LN_C = (1, 3, 4, 63, 64, 65, 68, 256, 260, 770)
LN_ADD = ("none", "a0", "a1", "both")


def _l(id, rows, C, **kw):
    return _case("ln", id, rows=rows, C=C, **kw)


def _ln_cases():
    out = []
    # C: 1 (zero variance, rstd = 1 / sqrt(eps)), 3, 63, 65 (scalar; 65: second trip of the scalar loop), 4, 64, 68, 256 (float4, one
    # trip), 260, 770 (float4 second trip; 770 % 4 = 2: scalar, 13 trips); rows: the 4-rows-per-block tail
    for i, C in enumerate(LN_C):
        for j in range(2):
            rows = LN_ROWS[(i + 3 * j) % 5]
            add = LN_ADD[(i + j) % 4]
            if C == 1 and add == "none":
                add = "a0"            # (dx is 0 exactly when C = 1: nothing to normalise an error by without an addend)
            out.append(_l(f"r{rows}-C{C}-{add}", rows, C, add=add))
    out.append(_l("r9-C772-both", 9, 772, add="both"))                    # float4, four trips, the last one partial
    # one misaligned operand with C % 4 == 0: the scalar path, still right
    for C in (64, 260):
        for mis in ("gamma", "beta", "x", "out", "dy", "dx", "add0", "add1"):
            out.append(_l(f"r5-C{C}-mis-{mis}", 5, C, add="both", mis=mis))
    # mean 100, spread 0.01: the two-pass variance
    for rows, C in ((3, 3), (5, 64), (4, 770), (3, 260)):
        out.append(_l(f"r{rows}-C{C}-mean100", rows, C, add="a1", big_mean=True))
    # dx aliasing an addend; `block`: the block backward's G, add1, G
    for rows, C in ((5, 260), (3, 65), (9, 64)):
        for alias in ("a0", "a1", "block"):
            out.append(_l(f"r{rows}-C{C}-alias-{alias}", rows, C, add="a0" if alias == "a0" else "a1" if alias == "a1" else "both", alias=alias))
    return out


SM_N = (1, 2, 3, 4, 5, 49, 197, 256, 257, 260, 263, 1027)
SM_ROWS = (1, 3, 5)
SM_KINDS = ("one", "big", "equal", "spike", "huge")


def _softmax_cases():
    out = []
    # N4 = N & ~3: 0 (1, 2, 3: tail only), one trip (4 .. 256), a second trip (257: N4 = 256 is still one; 260, 263, 1027), a tail after
    # it (263: 3, 1027: 3, 257: 1); ld = N rounded up to 4, and that + 8
    for i, N in enumerate(SM_N):
        for j, extra in enumerate((0, 8)):
            kind = SM_KINDS[(i + 2 * j) % 5]
            out.append(_case("softmax", f"N{N}-ld{_r4(N) + extra}-r{SM_ROWS[(i + j) % 3]}-{kind}", N=N, ld=_r4(N) + extra, rows=SM_ROWS[(i + j) % 3],
                             kind=kind, scale=(1.0, 0.125)[(i + j) % 2]))
    for N in (5, 263, 1027):
        for k, kind in enumerate(SM_KINDS):
            out.append(_case("softmax", f"N{N}-{kind}-all-kinds", N=N, ld=_r4(N) + 4, rows=5, kind=kind, scale=(0.125, 1.0)[k % 2]))
    return out


def _attn_cases():
    # (frames, T, heads, dh): dh = 6 drops the vector flags of q, k, v, out and dqkv by the batch stride; T = 4: ld = T; T = 129: two
    # score tiles with a one-row tail at dh = 8; T = 5 at dh = 8: every operand float4, probs with 3 padding columns
    return [_case("attn", f"f{f}-T{T}-h{h}-dh{dh}", frames=f, T=T, heads=h, dh=dh) for f, T, h, dh in
            ((2, 5, 3, 6), (1, 4, 2, 8), (1, 129, 1, 8), (2, 5, 2, 8), (1, 130, 2, 6))]


def _token_cases():
    out = []
    i = 0
    for patch in (4, 8, 16):
        for cin in (1, 3):
            for g in (1, 2, 3):
                acc, npre = i % 2, 1 + (i // 2) % 2
                out.append(_case("patchify", f"p{patch}-c{cin}-g{g}-acc{acc}", patch=patch, cin=cin, g=g, frames=1 + i % 2, acc=acc))
                out.append(_case("embed", f"p{patch}-c{cin}-g{g}-pre{npre}-acc{acc}", patch=patch, cin=cin, g=g, frames=1 + i % 2, acc=acc, npre=npre,
                                 ex=npre == 2 or i % 4 == 0, dim=(8, 12, 36)[i % 3], pos0=i % 3 != 1))
                i += 1
    return out


CASES = tuple(_gemm_cases() + _ln_cases() + _softmax_cases() + _attn_cases() + _token_cases())
BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES)


# ---------------------------------------------------------------------------------------------------------------------------
# GEMM: the descriptor of a case
# ---------------------------------------------------------------------------------------------------------------------------
def gemm_spec(kw):
    """Strides, offsets and batch levels of the case's operands, in floats: {a, b, c: {O, E, ld, bi, bo, off}, ...}.  An operand is
    stored as O rows of E contiguous floats at leading dimension ld; inner batches are column slices `bi` apart of one shared row."""
    M, N, K, vec = kw["M"], kw["N"], kw["K"], kw.get("vec", True)
    n_out, n_in = kw.get("outer", 1), kw.get("inner", 1)

    def op(name, O, E):
        bi = kw.get(name + "_bi", _r4(E) if vec else E) if n_in > 1 else 0
        width = (n_in - 1) * bi + E
        ld = kw.get(name + "_ld", _r4(width) + (0 if vec else 1))
        assert ld >= width, (name, ld, width)
        bo = O * ld + kw.get(name + "_box", 0) if n_out > 1 else 0
        return {"O": O, "E": E, "ld": ld, "bi": bi, "bo": bo, "off": kw.get(name + "_off", 0 if vec else 1)}

    s = {"a": op("a", M, K) if kw["la"] == "k" else op("a", K, M), "b": op("b", N, K) if kw["lb"] == "k" else op("b", K, N), "c": op("c", M, N)}
    if kw.get("b_shared"):
        s["b"]["bi"] = s["b"]["bo"] = 0
        s["b"]["ld"] = kw.get("b_ld", _r4(s["b"]["E"]) + (0 if vec else 1))
    s.update(n_out=n_out, n_in=n_in, batch=n_out * n_in, mode=EPI[kw.get("mode", "plain")], alpha=float(kw.get("alpha", 1.0)),
             bias_off=kw.get("bias_off", 0 if vec else 1) if kw.get("bias") else None, R=kw.get("R"))
    c_off = s["c"]["off"]
    s["r_off"] = kw.get("r_off", c_off)
    s["c2_off"] = kw.get("c2_off", c_off)
    s["h_off"] = kw.get("h_off", c_off)
    return s


def gemm_flags(kw):
    """(a_vec, b_vec, c_vec, bias_vec) as vit_gemm sets them (allocations are 16-byte aligned and FRONT % 4 == 0)."""
    s = gemm_spec(kw)

    def v(o):
        return o["off"] % 4 == 0 and o["ld"] % 4 == 0 and o["bo"] % 4 == 0 and o["bi"] % 4 == 0
    c = v(s["c"])
    if s["R"] == "sep":
        c = c and s["r_off"] % 4 == 0
    if s["mode"] == 1:
        c = c and s["c2_off"] % 4 == 0
    if s["mode"] == 2:
        c = c and s["h_off"] % 4 == 0
    return int(v(s["a"])), int(v(s["b"])), int(c), int(s["bias_off"] is None or s["bias_off"] % 4 == 0)


def _index(o, n_out, n_in, off=None, shared=False):
    """Flat positions (n_out, n_in, O, E) of an operand's elements in its allocation, and the allocation's size."""
    off = o["off"] if off is None else off
    a = torch.arange
    idx = (FRONT + off + a(n_out).view(-1, 1, 1, 1) * o["bo"] + a(n_in).view(1, -1, 1, 1) * o["bi"] + a(o["O"]).view(1, 1, -1, 1) * o["ld"]
           + a(o["E"]).view(1, 1, 1, -1))
    size = FRONT + off + (n_out - 1) * o["bo"] + (n_in - 1) * o["bi"] + o["O"] * o["ld"] + 129 * o["ld"] + 256
    return idx, size


# ---------------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------------
def _gen(case, salt=0):
    return torch.Generator().manual_seed(zlib.crc32(case.id.encode()) + salt)


@functools.lru_cache(maxsize=8)
def inputs(case: Case):
    """{name: float32 CPU tensor} in the operation's own shapes (no padding); read-only, shared by run and reference."""
    kw, g = case.kw, _gen(case)
    rn = lambda *s: torch.randn(*s, generator=g)
    if case.op == "gemm":
        s = gemm_spec(kw)
        B, M, N, K = s["batch"], kw["M"], kw["N"], kw["K"]
        inp = {"A": rn(B, M, K), "B": rn(1 if kw.get("b_shared") else B, K, N)}
        if kw.get("bias"):
            inp["bias"] = rn(N)
        if s["R"]:
            inp["R"] = rn(B, M, N)
        if s["mode"] == 2:
            H = torch.rand(B, M, N, generator=g) * 12 - 6
            H.view(-1)[::7] = 0.0
            inp["H"] = H
        return inp
    if case.op == "ln":
        rows, C = kw["rows"], kw["C"]
        x = 100 + 0.01 * rn(rows, C) if kw.get("big_mean") else rn(rows, C) * 1.5 + 0.3
        return {"x": x.contiguous(), "gamma": 1 + 0.3 * rn(C), "beta": 0.3 * rn(C), "dy": rn(rows, C), "add0": rn(rows, C), "add1": rn(rows, C)}
    if case.op == "softmax":
        rows, N, kind = kw["rows"], kw["N"], kw["kind"]
        x = rn(rows, N)
        if kind in ("big", "huge"):
            # every row scaled to +-80, and to +-300: exp(80) = 5.5e34 is still a float32, so a softmax without the max subtraction
            # survives `big` with a few digits lost; exp(300) is not, and `huge` is the row it cannot get right
            x = x * ((80 if kind == "big" else 300) / x.abs().max(1, keepdim=True).values.clamp_min(1e-3))
        elif kind == "equal":
            x = torch.full((rows, N), 0.7) * (1 + torch.arange(rows).view(-1, 1))
        elif kind == "spike":
            x = x.clamp(-3.5, 3.5)
            x[torch.arange(rows), torch.arange(rows) * 5 % N] = 104.0    # one entry >= 100 above the rest: they underflow to 0
        # the backward's probabilities are an INPUT of their own: the float32 rounding of the float64 softmax of the row at order one
        # (a one-hot P makes scale * P (d - sum d P) vanish and leaves nothing to normalise an error by)
        soft = rn(rows, N) if kind in ("big", "spike", "huge") else x
        return {"X": x.contiguous(), "Pin": torch.softmax(soft.double(), 1).float(), "dX": rn(rows, N)}
    if case.op == "attn":
        f, T, h, dh = kw["frames"], kw["T"], kw["heads"], kw["dh"]
        return {"qkv": rn(f, T, 3 * h * dh), "dout": rn(f, T, h * dh)}
    f, cin, g_, p = kw["frames"], kw["cin"], kw["g"], kw["patch"]
    img = rn(f, cin, g_ * p, g_ * p)
    if case.op == "patchify":
        return {"img": img, "dpatches": rn(f * g_ * g_, cin * p * p), "base": rn(f, cin, g_ * p, g_ * p)}
    dim, npre, T = kw["dim"], kw["npre"], kw["npre"] + g_ * g_
    pos = 0.5 * rn(T, dim)
    if kw["pos0"]:
        pos[:npre] = 0
    return {"img": img, "W": rn(dim, cin * p * p) / math.sqrt(cin * p * p), "b": 0.2 * rn(dim), "prefix": rn(npre, dim), "pos": pos,
            "dtokens": rn(f, T, dim), "base": rn(f, cin, g_ * p, g_ * p)}


# ---------------------------------------------------------------------------------------------------------------------------
# references: plain torch in `dt` (float64: the reference; float32: its own error e32)
# ---------------------------------------------------------------------------------------------------------------------------
def _gelu(x):
    return 0.5 * x * (1 + torch.erf(x * 0.7071067811865476))


def _gelu_grad(x):
    return 0.5 * (1 + torch.erf(x * 0.7071067811865476)) + x * torch.exp(-0.5 * x * x) * 0.3989422804014327


def _patch_rows(img, g, p):
    f, cin = img.shape[:2]
    return img.reshape(f, cin, g, p, g, p).permute(0, 2, 4, 1, 3, 5).reshape(f * g * g, cin * p * p)


def _unpatch(rows, f, cin, g, p):
    return rows.reshape(f, g, g, cin, p, p).permute(0, 3, 1, 4, 2, 5).reshape(f, cin, g * p, g * p)


def _slack(n):
    return ("exact", torch.full((n,), SENTINEL))


def _ref_gemm(case, inp, dt):
    kw, s = case.kw, gemm_spec(case.kw)
    out = {}
    sizes = _gemm_slack_sizes(kw)
    if kw.get("degenerate"):
        out["C"] = ("exact", torch.zeros(0))
        out["C_slack"] = _slack(sizes["C"])
        return out
    v = torch.matmul(inp["A"].to(dt), inp["B"].to(dt))
    if s["alpha"] != 1.0:
        v = torch.tensor(s["alpha"], dtype=torch.float32).to(dt) * v
    if "bias" in inp:
        v = v + inp["bias"].to(dt)
    if "R" in inp:
        v = v + inp["R"].to(dt)
    if s["mode"] == 2:
        v = v * _gelu_grad(inp["H"].to(dt))
    out["C"] = ("tensor", v)
    out["C_slack"] = _slack(sizes["C"])
    if s["mode"] == 1:
        out["C2"] = ("tensor", _gelu(v))
        out["C2_slack"] = _slack(sizes["C2"])
    return out


def _gemm_slack_sizes(kw):
    s = gemm_spec(kw)
    n = 0 if kw.get("degenerate") else s["batch"] * kw["M"] * kw["N"]
    return {"C": _index(s["c"], s["n_out"], s["n_in"])[1] - n, "C2": _index(s["c"], s["n_out"], s["n_in"], s["c2_off"])[1] - n}


def _ln_tail(C):
    return 8 * C + 256


def _ref_ln(case, inp, dt):
    kw = case.kw
    rows, C, add = kw["rows"], kw["C"], kw["add"]
    x, gamma, beta, dy = (inp[n].to(dt) for n in ("x", "gamma", "beta", "dy"))
    mu = x.mean(1, keepdim=True)
    var = ((x - mu) * (x - mu)).mean(1, keepdim=True)
    rstd = 1 / torch.sqrt(var + torch.tensor(LN_EPS, dtype=torch.float32).to(dt))
    xh = (x - mu) * rstd
    dyg = dy * gamma
    dx = rstd * (dyg - dyg.mean(1, keepdim=True) - xh * (dyg * xh).mean(1, keepdim=True))
    if add in ("a0", "both"):
        dx = inp["add0"].to(dt) + dx
    if add in ("a1", "both"):
        dx = dx + inp["add1"].to(dt)
    off = lambda n: 1 if kw.get("mis") == n else 0
    return {"out": ("tensor", xh * gamma + beta), "mean": ("tensor", mu.reshape(-1)), "rstd": ("tensor", rstd.reshape(-1)), "dx": ("tensor", dx),
            "out_slack": _slack(FRONT + off("out") + _ln_tail(C)), "dx_slack": _slack(FRONT + off("dx") + _ln_tail(C)),
            "mean_slack": _slack(FRONT + 64), "rstd_slack": _slack(FRONT + 64)}


def _ref_softmax(case, inp, dt):
    kw = case.kw
    rows, N, ld = kw["rows"], kw["N"], kw["ld"]
    x, d, p = inp["X"].to(dt), inp["dX"].to(dt), inp["Pin"].to(dt)
    e = torch.exp(x - x.max(1, keepdim=True).values)
    P_ = e / e.sum(1, keepdim=True)
    scale = torch.tensor(kw["scale"], dtype=torch.float32).to(dt)
    n_slack = FRONT + rows * (ld - N) + 8 * ld + 256
    out = {"P": ("tensor", P_), "P_slack": _slack(n_slack), "dX": ("tensor", scale * (p * (d - (d * p).sum(1, keepdim=True)))),
           "dX_slack": _slack(n_slack), "Pin_unchanged": ("exact", torch.ones(1, dtype=torch.int32))}
    if N == 1:                          # p = 1: d - sum d p is d - d, zero exactly, and there is nothing to normalise an error by
        out["dX"] = ("exact", torch.zeros(rows, 1))
    if kw["kind"] == "equal":
        out["P_uniform"] = ("exact", torch.full((rows, N), 1.0 / N, dtype=torch.float64).float())
    return out


def probs_ld(T):
    return _r4(T)


def _ref_attn(case, inp, dt):
    kw = case.kw
    f, T, h, dh = kw["frames"], kw["T"], kw["heads"], kw["dh"]
    ld = probs_ld(T)
    scale = torch.tensor(dh ** -0.5, dtype=torch.float32).to(dt)
    q, k, v = inp["qkv"].to(dt).reshape(f, T, 3, h, dh).permute(2, 0, 3, 1, 4)          # (f, h, T, dh) each
    do = inp["dout"].to(dt).reshape(f, T, h, dh).permute(0, 2, 1, 3)
    S = scale * torch.matmul(q, k.transpose(-1, -2))
    e = torch.exp(S - S.max(-1, keepdim=True).values)
    Pm = e / e.sum(-1, keepdim=True)
    o = torch.matmul(Pm, v)
    dP = torch.matmul(do, v.transpose(-1, -2))
    dS = scale * (Pm * (dP - (dP * Pm).sum(-1, keepdim=True)))
    dq, dk, dv = torch.matmul(dS, k), torch.matmul(dS.transpose(-1, -2), q), torch.matmul(Pm.transpose(-1, -2), do)
    dqkv = torch.stack([dq, dk, dv], 0).permute(1, 3, 0, 2, 4).reshape(f, T, 3 * h * dh)
    n_slack = FRONT + f * h * T * (ld - T) + 129 * ld + 256
    return {"probs": ("tensor", Pm), "probs_slack": _slack(n_slack), "out": ("tensor", o.permute(0, 2, 1, 3).reshape(f, T, h * dh)),
            "out_slack": _slack(FRONT + 129 * h * dh + 256), "dprobs": ("tensor", dS), "dprobs_slack": _slack(n_slack),
            "dqkv": ("tensor", dqkv), "dqkv_slack": _slack(FRONT + 129 * 3 * h * dh + 256)}


def _ref_patchify(case, inp, dt):
    kw = case.kw
    f, cin, g, p = kw["frames"], kw["cin"], kw["g"], kw["patch"]
    gimg = _unpatch(inp["dpatches"], f, cin, g, p)
    if kw["acc"]:
        gimg = (inp["base"].double() + gimg.double()).float()        # one float32 add, correctly rounded: exact as well
    KP = cin * p * p
    return {"patches": ("exact", _patch_rows(inp["img"], g, p).contiguous()), "patches_slack": _slack(FRONT + 129 * KP + 256),
            "gimg": ("exact", gimg.contiguous()), "gimg_slack": _slack(FRONT + 129 * g * p + 256)}


def _ref_embed(case, inp, dt):
    kw = case.kw
    f, cin, g, p, dim, npre = kw["frames"], kw["cin"], kw["g"], kw["patch"], kw["dim"], kw["npre"]
    KP, np_ = cin * p * p, g * g
    rows = _patch_rows(inp["img"], g, p)
    W = inp["W"].to(dt)
    emb = rows.to(dt) @ W.t() + inp["b"].to(dt)
    tok = torch.cat([inp["prefix"].to(dt).expand(f, npre, dim), emb.reshape(f, np_, dim)], 1) + inp["pos"].to(dt)
    dpatch = inp["dtokens"].to(dt)[:, npre:].reshape(f * np_, dim) @ W
    gimg = _unpatch(dpatch, f, cin, g, p)
    if kw["acc"]:
        gimg = inp["base"].to(dt) + gimg
    out = {"patches": ("exact", rows.contiguous()), "patches_slack": _slack(FRONT + 129 * KP + 256), "emb": ("tensor", emb),
           "emb_slack": _slack(FRONT + 129 * dim + 256), "tokens": ("tensor", tok), "tokens_slack": _slack(FRONT + 129 * dim + 256),
           "dpatches": ("tensor", dpatch), "dpatches_slack": _slack(FRONT + 129 * KP + 256), "gimg": ("tensor", gimg),
           "gimg_slack": _slack(FRONT + 129 * g * p + 256)}
    if kw["pos0"]:
        out["tokens_prefix"] = ("exact", inp["prefix"].expand(f, npre, dim).contiguous())
    return out


_REFS = {"gemm": _ref_gemm, "ln": _ref_ln, "softmax": _ref_softmax, "attn": _ref_attn, "patchify": _ref_patchify, "embed": _ref_embed}


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
        if not getattr(self.capi, "_xf_bound", False):
            lib.bind(self.capi, lib._XF_PROTOS if hasattr(self.capi, "i2v_xf_softmax_f32") else lib.XF_HOST_PROTOS)
            self.capi._xf_bound = True
        self.device_lib = hasattr(self.capi, "i2v_vit_layernorm_f32")

    def call(self, name, *args):
        lib.check(self.capi, getattr(self.capi, name)(*args, self.eng.stream()))

    def sync(self):
        if self.cuda:
            torch.cuda.synchronize()


class _Buf:
    """One allocation: `fill` everywhere, `data` scattered to the flat positions `idx` (None: the positions keep `fill`)."""

    def __init__(self, cx, size, idx, data, fill):
        host = torch.full((size,), fill, dtype=torch.float32)
        self.idx = idx.reshape(-1)
        assert self.idx.numel() == 0 or (int(self.idx.max()) < size and self.idx.unique().numel() == self.idx.numel())
        if data is not None:
            host[self.idx] = data.reshape(-1).float()
        self.cx, self.shape, self.size = cx, tuple(idx.shape), size
        self.dev = host.to(cx.eng.device) if cx.cuda else host
        assert self.dev.data_ptr() % 16 == 0

    def ptr(self, floats=0):
        return P(self.dev.data_ptr() + 4 * floats)

    def host(self):
        self.cx.sync()
        return self.dev.detach().cpu().clone()

    def collect(self, out, name, shape=None):
        buf = self.host()
        out[name] = buf[self.idx].reshape(shape if shape is not None else self.shape).contiguous()
        keep = torch.ones(self.size, dtype=torch.bool)
        keep[self.idx] = False
        out[name + "_slack"] = buf[keep]


def _flat(n, off=0):
    return FRONT + off + torch.arange(n)


def _inb(cx, t, off=0, tail=256):
    """A contiguous input `off` floats past FRONT, NaN around it."""
    return _Buf(cx, FRONT + off + t.numel() + tail, _flat(t.numel(), off), t, float("nan"))


def _outb(cx, n, off=0, tail=256, init=None):
    return _Buf(cx, FRONT + off + n + tail, _flat(n, off), init if init is not None else torch.full((n,), float("nan")), SENTINEL)


def gemm_desc(case, bufs, only=None):
    """The descriptor of the case over `bufs`; `only` = b: batch b on its own (batch = 1, the pointers moved to it, the strides kept)."""
    kw, s = case.kw, gemm_spec(case.kw)
    d = lib.XfGemmDesc()

    def base(name, o, off):
        shift = 0
        if only is not None:
            shift = (only // s["n_in"]) * o["bo"] + (only % s["n_in"]) * o["bi"]
        return bufs[name].ptr(FRONT + off + shift)
    a, b, c = s["a"], s["b"], s["c"]
    d.A, d.a_bo, d.a_bi = base("A", a, a["off"]), a["bo"], a["bi"]
    d.a_sm, d.a_sk = (a["ld"], 1) if kw["la"] == "k" else (1, a["ld"])
    d.B, d.b_bo, d.b_bi = base("B", b, b["off"]), b["bo"], b["bi"]
    d.b_sk, d.b_sn = (1, b["ld"]) if kw["lb"] == "k" else (b["ld"], 1)
    d.C, d.c_bo, d.c_bi, d.c_sm = base("C", c, c["off"]), c["bo"], c["bi"], c["ld"]
    d.bias = bufs["bias"].ptr(FRONT + s["bias_off"]) if "bias" in bufs else None
    d.R = None if not s["R"] else d.C if s["R"] == "inplace" else base("R", c, s["r_off"])
    d.C2 = base("C2", c, s["c2_off"]) if s["mode"] == 1 else None
    d.H = base("H", c, s["h_off"]) if s["mode"] == 2 else None
    d.M, d.N, d.K, d.batch, d.nb_in = kw["M"], kw["N"], kw["K"], s["batch"], 0 if kw.get("nb_in0") else s["n_in"]
    d.alpha, d.mode = s["alpha"], s["mode"]
    if only is not None:
        d.batch, d.nb_in = 1, 1
    if kw.get("degenerate"):
        setattr(d, *kw["degenerate"])
    return d


def _run_gemm(cx, case, inp, only=None):
    kw, s = case.kw, gemm_spec(case.kw)
    n_out, n_in, M, N, K = s["n_out"], s["n_in"], kw["M"], kw["N"], kw["K"]
    nan, B = float("nan"), s["batch"]
    A = inp["A"] if kw["la"] == "k" else inp["A"].transpose(1, 2)                # stored (O, E)
    Bm = inp["B"].transpose(1, 2) if kw["lb"] == "k" else inp["B"]
    ia, na = _index(s["a"], n_out, n_in)
    bufs = {"A": _Buf(cx, na, ia, A.reshape(n_out, n_in, *A.shape[1:]), nan)}
    if kw.get("b_shared"):
        ib, nb = _index(s["b"], 1, 1)
        bufs["B"] = _Buf(cx, nb, ib, Bm, nan)
    else:
        ib, nb = _index(s["b"], n_out, n_in)
        bufs["B"] = _Buf(cx, nb, ib, Bm.reshape(n_out, n_in, *Bm.shape[1:]), nan)
    ic, nc = _index(s["c"], n_out, n_in)
    if only is not None:
        ic = ic[only // n_in, only % n_in]
    dead = bool(kw.get("degenerate"))
    init = inp["R"] if s["R"] == "inplace" else torch.full((B, M, N), nan)
    if only is not None:
        init = init[only]
    bufs["C"] = _Buf(cx, nc, ic[..., :0] if dead else ic, None if dead else init, SENTINEL)
    if "bias" in inp:
        bufs["bias"] = _inb(cx, inp["bias"], s["bias_off"])
    if s["R"] == "sep":
        ir, nr = _index(s["c"], n_out, n_in, s["r_off"])
        bufs["R"] = _Buf(cx, nr, ir, inp["R"], nan)
    if s["mode"] == 1:
        i2, n2 = _index(s["c"], n_out, n_in, s["c2_off"])
        bufs["C2"] = _Buf(cx, n2, i2 if only is None else i2[only // n_in, only % n_in], init * nan, SENTINEL)
    if s["mode"] == 2:
        ih, nh = _index(s["c"], n_out, n_in, s["h_off"])
        bufs["H"] = _Buf(cx, nh, ih, inp["H"], nan)
    d = gemm_desc(case, bufs, only)
    cx.call("i2v_xf_gemm_f32", ctypes.byref(d))
    out = {}
    shape = (0,) if dead else (M, N) if only is not None else (B, M, N)
    bufs["C"].collect(out, "C", shape)
    if s["mode"] == 1:
        bufs["C2"].collect(out, "C2", shape)
    return out


def _run_ln(cx, case, inp):
    kw = case.kw
    rows, C, add, alias, mis = kw["rows"], kw["C"], kw["add"], kw.get("alias"), kw.get("mis")
    off = lambda n: 1 if mis == n else 0
    n, tail = rows * C, _ln_tail(C)
    x, gamma, beta, dy = (_inb(cx, inp[k], off(k), tail) for k in ("x", "gamma", "beta", "dy"))
    out_b = _outb(cx, n, off("out"), tail)
    mean, rstd = _outb(cx, rows, 0, 64), _outb(cx, rows, 0, 64)
    fwd, bwd = ("i2v_vit_layernorm_f32", "i2v_vit_layernorm_bwd_f32") if cx.device_lib else ("i2v_xf_layernorm_f32", "i2v_xf_layernorm_bwd_f32")
    cx.call(fwd, x.ptr(FRONT + off("x")), rows, C, gamma.ptr(FRONT + off("gamma")), beta.ptr(FRONT + off("beta")), LN_EPS,
            out_b.ptr(FRONT + off("out")), mean.ptr(FRONT), rstd.ptr(FRONT))
    # the backward takes the statistics this library saved; dx starts as NaN, or as the addend it aliases
    use0, use1 = add in ("a0", "both"), add in ("a1", "both")
    dx = _outb(cx, n, off("dx"), tail, init=inp["add0"] if alias in ("a0", "block") else inp["add1"] if alias == "a1" else None)
    dxp = dx.ptr(FRONT + off("dx"))
    a0 = a1 = None
    p0 = p1 = NULL
    if use0:
        if alias in ("a0", "block"):
            p0 = dxp
        else:
            a0 = _inb(cx, inp["add0"], off("add0"), tail)
            p0 = a0.ptr(FRONT + off("add0"))
    if use1:
        if alias == "a1":
            p1 = dxp
        else:
            a1 = _inb(cx, inp["add1"], off("add1"), tail)
            p1 = a1.ptr(FRONT + off("add1"))
    cx.call(bwd, dy.ptr(FRONT + off("dy")), x.ptr(FRONT + off("x")), mean.ptr(FRONT), rstd.ptr(FRONT), gamma.ptr(FRONT + off("gamma")), rows, C,
            p0, p1, dxp)
    out = {}
    out_b.collect(out, "out", (rows, C))
    mean.collect(out, "mean", (rows,))
    rstd.collect(out, "rstd", (rows,))
    dx.collect(out, "dx", (rows, C))
    del a0, a1
    return out


def _rows_index(rows, N, ld):
    return FRONT + torch.arange(rows).view(-1, 1) * ld + torch.arange(N).view(1, -1)


def _run_softmax(cx, case, inp):
    kw = case.kw
    rows, N, ld = kw["rows"], kw["N"], kw["ld"]
    idx, size = _rows_index(rows, N, ld), FRONT + rows * ld + 8 * ld + 256
    X = _Buf(cx, size, idx, inp["X"], SENTINEL)
    cx.call("i2v_xf_softmax_f32", X.ptr(FRONT), rows, N, ld)
    Pin = _Buf(cx, size, idx, inp["Pin"], SENTINEL)
    before = Pin.host()
    dX = _Buf(cx, size, idx, inp["dX"], SENTINEL)
    cx.call("i2v_xf_softmax_bwd_f32", dX.ptr(FRONT), Pin.ptr(FRONT), rows, N, ld, kw["scale"])
    out = {}
    X.collect(out, "P")
    dX.collect(out, "dX")
    out["Pin_unchanged"] = torch.tensor([int(same_bits(before, Pin.host()))], dtype=torch.int32)
    if kw["kind"] == "equal":
        out["P_uniform"] = out["P"].clone()
    return out


def _run_attn(cx, case, inp):
    kw = case.kw
    f, T, h, dh = kw["frames"], kw["T"], kw["heads"], kw["dh"]
    C, ld = h * dh, probs_ld(T)
    assert cx.capi.i2v_vit_probs_ld(T) == ld
    pidx = FRONT + (torch.arange(f * h * T).view(f, h, T, 1) * ld + torch.arange(T).view(1, 1, 1, -1))
    psize = FRONT + f * h * T * ld + 129 * ld + 256
    qkv, dout = _inb(cx, inp["qkv"], 0, 129 * 3 * C + 256), _inb(cx, inp["dout"], 0, 129 * C + 256)
    probs = _Buf(cx, psize, pidx, torch.full((f, h, T, T), float("nan")), SENTINEL)
    o = _outb(cx, f * T * C, 0, 129 * C + 256)
    cx.call("i2v_vit_attention_f32", qkv.ptr(FRONT), f, T, h, dh, dh ** -0.5, probs.ptr(FRONT), o.ptr(FRONT))
    dprobs = _Buf(cx, psize, pidx, torch.full((f, h, T, T), float("nan")), SENTINEL)
    dqkv = _outb(cx, f * T * 3 * C, 0, 129 * 3 * C + 256)
    cx.call("i2v_vit_attention_bwd_f32", qkv.ptr(FRONT), probs.ptr(FRONT), dout.ptr(FRONT), f, T, h, dh, dh ** -0.5, dprobs.ptr(FRONT),
            dqkv.ptr(FRONT))
    out = {}
    probs.collect(out, "probs")
    o.collect(out, "out", (f, T, C))
    dprobs.collect(out, "dprobs")
    dqkv.collect(out, "dqkv", (f, T, 3 * C))
    return out


def _run_patchify(cx, case, inp):
    kw = case.kw
    f, cin, g, p, acc = kw["frames"], kw["cin"], kw["g"], kw["patch"], kw["acc"]
    KP, n = cin * p * p, inp["img"].numel()
    img, dpat = _inb(cx, inp["img"], 0, 129 * g * p + 256), _inb(cx, inp["dpatches"], 0, 129 * KP + 256)
    pat = _outb(cx, n, 0, 129 * KP + 256)
    gimg = _outb(cx, n, 0, 129 * g * p + 256, init=inp["base"] if acc else None)
    cx.call("i2v_xf_patchify_f32", img.ptr(FRONT), pat.ptr(FRONT), f, cin, g, g, p, NULL, 0)
    cx.call("i2v_xf_patchify_f32", NULL, dpat.ptr(FRONT), f, cin, g, g, p, gimg.ptr(FRONT), acc)
    out = {}
    pat.collect(out, "patches", (f * g * g, KP))
    gimg.collect(out, "gimg", tuple(inp["img"].shape))
    return out


def _run_embed(cx, case, inp):
    kw = case.kw
    f, cin, g, p, dim, npre, acc = kw["frames"], kw["cin"], kw["g"], kw["patch"], kw["dim"], kw["npre"], kw["acc"]
    KP, np_, T = cin * p * p, g * g, kw["npre"] + g * g
    img = _inb(cx, inp["img"], 0, 129 * g * p + 256)
    W, b, prefix, pos = _inb(cx, inp["W"], 0, 129 * KP + 256), _inb(cx, inp["b"]), _inb(cx, inp["prefix"], 0, 129 * dim + 256), _inb(cx, inp["pos"], 0, 129 * dim + 256)
    dtok = _inb(cx, inp["dtokens"], 0, 129 * dim + 256)
    pat, emb, tok = _outb(cx, f * np_ * KP, 0, 129 * KP + 256), _outb(cx, f * np_ * dim, 0, 129 * dim + 256), _outb(cx, f * T * dim, 0, 129 * dim + 256)
    dpat = _outb(cx, f * np_ * KP, 0, 129 * KP + 256)
    gimg = _outb(cx, inp["img"].numel(), 0, 129 * g * p + 256, init=inp["base"] if acc else None)
    F_ = FRONT
    if kw["ex"]:
        cx.call("i2v_vit_embed_ex_f32", img.ptr(F_), f, cin, g, p, W.ptr(F_), b.ptr(F_), prefix.ptr(F_), npre, pos.ptr(F_), dim, pat.ptr(F_), emb.ptr(F_), tok.ptr(F_))
        cx.call("i2v_vit_embed_bwd_ex_f32", dtok.ptr(F_), f, cin, g, p, W.ptr(F_), dim, npre, dpat.ptr(F_), gimg.ptr(F_), acc)
    else:
        assert npre == 1
        cx.call("i2v_vit_embed_f32", img.ptr(F_), f, cin, g, p, W.ptr(F_), b.ptr(F_), prefix.ptr(F_), pos.ptr(F_), dim, pat.ptr(F_), emb.ptr(F_), tok.ptr(F_))
        cx.call("i2v_vit_embed_bwd_f32", dtok.ptr(F_), f, cin, g, p, W.ptr(F_), dim, dpat.ptr(F_), gimg.ptr(F_), acc)
    out = {}
    pat.collect(out, "patches", (f * np_, KP))
    emb.collect(out, "emb", (f * np_, dim))
    tok.collect(out, "tokens", (f, T, dim))
    dpat.collect(out, "dpatches", (f * np_, KP))
    gimg.collect(out, "gimg", tuple(inp["img"].shape))
    if kw["pos0"]:
        out["tokens_prefix"] = out["tokens"][:, :npre].contiguous()
    return out


_RUNS = {"gemm": _run_gemm, "ln": _run_ln, "softmax": _run_softmax, "attn": _run_attn, "patchify": _run_patchify, "embed": _run_embed}


def run(engine, case: Case):
    """The case through the C entries of `engine.capi`: {name: CPU tensor} over the names of `reference(case)`."""
    return _RUNS[case.op](_Ctx(engine), case, inputs(case))


def run_batch_alone(engine, case: Case, b):
    """Batch `b` of a GEMM case as a launch of its own: {"C": (M, N), "C_slack"} (and C2)."""
    return _run_gemm(_Ctx(engine), case, inputs(case), only=b)


# ---------------------------------------------------------------------------------------------------------------------------
# refusals: (label, the name the message starts with, thunk returning the status); `keep` holds the buffers
# ---------------------------------------------------------------------------------------------------------------------------
def gemm_refusals(engine):
    cx = _Ctx(engine)
    case = BY_ID["gemm-flags-all-set"]
    inp = inputs(case)
    s = gemm_spec(case.kw)
    keep = {"A": _Buf(cx, *reversed(_index(s["a"], 1, 1)), inp["A"], 0.0), "B": _Buf(cx, *reversed(_index(s["b"], 1, 1)), inp["B"].transpose(1, 2), 0.0),
            "C": _Buf(cx, *reversed(_index(s["c"], 1, 1)), None, SENTINEL), "bias": _inb(cx, inp["bias"]),
            "R": _Buf(cx, *reversed(_index(s["c"], 1, 1)), inp["R"], 0.0)}

    def thunk(**edits):
        def go():
            d = gemm_desc(case, keep)
            for k, v in edits.items():
                setattr(d, k, v)
            return cx.capi.i2v_xf_gemm_f32(ctypes.byref(d), cx.eng.stream())
        return go
    thunks = [("A contiguous along neither M nor K", "vit_gemm", thunk(a_sm=20, a_sk=2)),
              ("B contiguous along neither K nor N", "vit_gemm", thunk(b_sk=2, b_sn=20)),
              ("GELU without C2", "vit_gemm", thunk(mode=1)),
              ("GELU backward without H", "vit_gemm", thunk(mode=2)),
              ("K = 0", "vit_gemm", thunk(K=0)), ("K = -4", "vit_gemm", thunk(K=-4)),
              ("batch = 65536", "vit_gemm", thunk(batch=65536)),
              ("null descriptor", "i2v_xf_gemm_f32", lambda: cx.capi.i2v_xf_gemm_f32(None, cx.eng.stream()))]

    def untouched():
        out = {}
        keep["C"].collect(out, "C")
        return bool((out["C"] == SENTINEL).all()) and bool((out["C_slack"] == SENTINEL).all())
    return thunks, untouched, keep


def device_refusals(engine):
    """The softmax and token-assembly refusals (device library only)."""
    cx = _Ctx(engine)
    s = cx.eng.stream
    z = lambda n: torch.zeros(n + 8, device=cx.eng.device)
    X, Pb = z(64), z(64)
    ptr = lambda t, off=0: P(t.data_ptr() + 4 * off)
    sm, smb = cx.capi.i2v_xf_softmax_f32, cx.capi.i2v_xf_softmax_bwd_f32
    thunks = [("softmax ld % 4", "vit_softmax", lambda: sm(ptr(X), 2, 5, 6, s())),
              ("softmax ld < N", "vit_softmax", lambda: sm(ptr(X), 2, 9, 8, s())),
              ("softmax X misaligned", "vit_softmax", lambda: sm(ptr(X, 1), 2, 5, 8, s())),
              ("softmax_bwd ld % 4", "vit_softmax_bwd", lambda: smb(ptr(X), ptr(Pb), 2, 5, 7, 1.0, s())),
              ("softmax_bwd ld < N", "vit_softmax_bwd", lambda: smb(ptr(X), ptr(Pb), 2, 9, 8, 1.0, s())),
              ("softmax_bwd dX misaligned", "vit_softmax_bwd", lambda: smb(ptr(X, 1), ptr(Pb), 2, 5, 8, 1.0, s())),
              ("softmax_bwd P misaligned", "vit_softmax_bwd", lambda: smb(ptr(X), ptr(Pb, 2), 2, 5, 8, 1.0, s()))]
    # token assembly: frames 1, in_chans 1, g 2; every buffer large enough for the launches that run before the refusal
    big = 4096
    img, W, b, pre, pos, pat, emb, tok, dtok, gimg = (z(big) for _ in range(10))
    E, EB = cx.capi.i2v_vit_embed_ex_f32, cx.capi.i2v_vit_embed_bwd_ex_f32

    def embed(patch=4, dim=8, npre=1, g=2, img_off=0, tok_off=0, pat_off=0):
        return lambda: E(ptr(img, img_off), 1, 1, g, patch, ptr(W), ptr(b), ptr(pre), npre, ptr(pos), dim, ptr(pat, pat_off), ptr(emb), ptr(tok, tok_off), s())

    def embed_bwd(patch=4, dim=8, npre=1, g=2, gimg_off=0, pat_off=0):
        return lambda: EB(ptr(dtok), 1, 1, g, patch, ptr(W), dim, npre, ptr(pat, pat_off), ptr(gimg, gimg_off), 0, s())
    thunks += [("embed patch % 4", "vit_patchify", embed(patch=6)), ("embed dim % 4", "vit_assemble", embed(dim=6)),
               ("embed image misaligned", "vit_patchify", embed(img_off=1)), ("embed patches misaligned", "vit_patchify", embed(pat_off=1)),
               ("embed tokens misaligned", "vit_assemble", embed(tok_off=1)),
               ("embed n_prefix 0", "i2v_vit_embed", embed(npre=0)), ("embed n_prefix >= T", "vit_assemble", embed(g=0, npre=1)),
               ("embed_bwd n_prefix 0", "i2v_vit_embed_bwd", embed_bwd(npre=0)), ("embed_bwd patch % 4", "vit_patchify", embed_bwd(patch=6)),
               ("embed_bwd image misaligned", "vit_patchify", embed_bwd(gimg_off=1))]
    return thunks, (X, Pb, img, W, b, pre, pos, pat, emb, tok, dtok, gimg)
