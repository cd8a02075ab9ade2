"""TEST INFRASTRUCTURE: the case table of the two fused attention launches that have a softmax of their own -- `cait_attention(_bwd)`
(csrc/i2v_cait.hip: talking heads, every CaiT block) and `convit_attention(_bwd)` (csrc/i2v_convit.hip: gated positional attention, every
ConViT block; ungated behind the join) -- and of the three small launches next to them: `cait_add_pos` (the stem of every CaiT, ConViT and
XCiT surrogate), `convit_join_cls` and `convit_join_cls_bwd`.  All five have a scalar twin in the host simulation (csrc/i2v_cait_host.h,
csrc/i2v_convit_host.h): tests/test_attn_edge_cpu.py runs the table there, tests/test_gpu_attn_edge.py on the device.  The buffer helpers
are those of tests/xf_cases.py, imported.

`run(engine, case)` calls the C entries (include/i2v_cait.h, include/i2v_convit.h) through `engine.capi` and returns {name: CPU tensor};
`reference(case)` returns {name: (kind, tensor)} over the SAME names.  The references are `tests/cait_reference.talking_heads` and
`tests/convit_reference.blend_attention` in float64 under `torch.autograd.grad`.

Kinds and bounds (`check`):
  planes   the error is taken per slice -- for `probs` one (frame, head, row) over the keys, for `out`, `dq`, `dk`, `dv` one (frame, token,
           head) of dh values -- as max|got - want| over the slice divided by the largest |want| of the slice's (frame, head) plane; the
           case's error is its worst slice, held to max(2e-6, 4 e32) (2e-6: xf_cases.FLOOR; 4: DESIGN.md section 14).  A wrong tail row or
           a wrong last key of one head is not divided by everything that is right.  A plane whose reference is exactly zero (T = 1: dq
           and dk; q = 0: dk; c_h = 0: dq and dk of head h; `spike`: dq and dk) must be exactly zero.
  exact    equal bits: the slack around every output, the pad columns T .. ld of `probs` and of both scratch arrays, the three small
           launches (one rounded add per element, or a copy), `dS_zero` (the planes of the score gradient that must be exactly zero).
e32 is the larger of two errors against float64 under the same measure -- the reference evaluated in float32 by plain torch on the CPU,
and the scalar host twin through the host simulation -- committed as tests/golden/attn_edge_fp32_cpu_errors.json
(tests/make_attn_edge_fixtures.py).  Nothing in a bound comes from the device.

Buffers (xf_cases._Buf).  Every operand lies FRONT = 128 floats into a larger flat allocation with a tail of 64 rows + 256 floats behind
it.  Everything of an OUTPUT allocation that is not an addressed element -- the pad columns T .. ld of probs, dS and Pm included -- is
SENTINEL and must come back bit for bit; its addressed elements start as NaN.  Everything of an INPUT allocation that is not an addressed
element is NaN -- the pad columns of the table included, and those of the probabilities the backward reads, which are handed over in a
fresh allocation: a stray read poisons a checked output.

Branch arithmetic (re-derive the comments at the cases when any of it changes):
  both forwards / row-tile backwards: one workgroup of 4 waves per tile of 16 query rows (and frame; ConViT: and head); Tp = T rounded up to
    16, LDS rows of Tp + 4 floats.  CaiT holds all H heads' tiles: H 16 (Tp + 4) 4 bytes, instantiated for HM = 4, 8, 16 heads (H <= HM:
    `h < H` guards in head_mix / mix_lds); ConViT holds one: 16 (Tp + 4) 4 bytes.  Past 64 KiB `raise_lds` raises the kernel's limit, and
    past 160 KiB the call is refused: CaiT serves H (Tp + 4) <= 2560, ConViT Tp + 4 <= 2560 (T <= 2544).
  scores: a wave per (head, 16-key tile); the head width walked in chunks of 16, lane quad g = lane / 16 loading floats 4 g .. 4 g + 3 of
    the chunk: at dh 4 only g == 0 is live, at dh 20 the second chunk has one live quad.
  softmax / row sums: a wave per row, lane l on keys l, l + 64, ...: a second trip from T = 65.
  products over the keys (out, dq): a wave per (head, 16-column tile), ND = ceil(dh / 16) tiles per head: H ND wave tasks in CaiT (8 at
    H 2, dh 64; 10 at dh 80), ND in ConViT (5 at dh 80: the second trip of `t += 4`); `dok` is false for the columns past dh (dh 20: 12 of
    16 lanes of the second tile).  Key-tile backward: 2 H ND (CaiT) or 2 ND (ConViT: 10 at dh 80) wave tasks.
  cait_add_pos / convit_join_cls(_bwd): one thread per float4, min(ceil(quads / 256), 65536) blocks -- the grid-stride second trip starts
    above 16.7 M quads (64 M floats), left to code reading.

`bl`: the bias of the first head mix is constant over the keys of a row and cancels in the softmax, so NO output depends on it and no
test can see a wrong `bl` -- the `bl-large` case checks the other direction: with bl = 50 N(0, 1) no output may move beyond its bound.
"""
import functools
import zlib

import torch

from i2v_amd import lib
from tests import cait_reference as car
from tests import convit_reference as cvr
from tests.xf_cases import FLOOR, FRONT, NULL, SENTINEL, Case, P, _Buf, _Ctx as _XfCtx, _inb, _outb, bound, same_bits

CAIT_KINDS = ("dense", "identity", "huge", "spike", "equal", "bl-large")
CONVIT_KINDS = ("gated", "ungated", "huge", "spike", "equal", "c0", "c1z", "zrows")
VALUE_OUTPUTS = ("probs", "out", "dq", "dk", "dv")
LDS_DEFAULT, LDS_MAX = 64 * 1024, 160 * 1024


def _a(op, F, T, H, dh, kind):
    return Case(f"{op}-f{F}-T{T}-h{H}-dh{dh}-{kind}", op, tuple(sorted(dict(F=F, T=T, H=H, dh=dh, kind=kind).items())))


def _s(op, F, T, C):
    return Case(f"{op}-f{F}-T{T}-C{C}", op, tuple(sorted(dict(F=F, T=T, C=C).items())))


# ---------------------------------------------------------------------------------------------------------------------------
# the table
# ---------------------------------------------------------------------------------------------------------------------------
CAIT_CASES = (
    _a("cait", 1, 1, 1, 4, "dense"),             # the smallest: P exactly 1.0, dq and dk exactly 0
    _a("cait", 1, 15, 2, 8, "dense"),            # one row short of the tile
    _a("cait", 1, 16, 2, 8, "dense"),            # the tile
    _a("cait", 1, 17, 2, 8, "dense"),            # a one-row, one-key tail tile
    _a("cait", 1, 17, 2, 8, "identity"),
    _a("cait", 1, 17, 2, 8, "huge"),
    _a("cait", 1, 17, 2, 8, "spike"),
    _a("cait", 1, 17, 2, 8, "equal"),
    _a("cait", 1, 17, 2, 8, "bl-large"),
    _a("cait", 3, 17, 2, 8, "dense"),            # frame offsets
    _a("cait", 1, 63, 3, 20, "dense"),           # dh 20: a partial second chunk; H 3 < HM in <4>
    _a("cait", 1, 64, 3, 20, "dense"),
    _a("cait", 1, 65, 3, 20, "dense"),           # the lane loops' second trip, by one key
    _a("cait", 1, 65, 3, 20, "identity"),
    _a("cait", 1, 65, 3, 20, "huge"),
    _a("cait", 1, 65, 3, 20, "spike"),
    _a("cait", 1, 129, 4, 4, "dense"),           # dh 4: only the g == 0 quad of a chunk is live
    _a("cait", 2, 33, 5, 12, "dense"),           # <8> with H < HM
    _a("cait", 2, 33, 5, 12, "identity"),
    _a("cait", 2, 33, 5, 12, "huge"),
    _a("cait", 1, 17, 9, 4, "dense"),            # <16>, its smallest
    _a("cait", 1, 144, 16, 4, "dense"),          # <16>, its largest: 151 552 B, raise_lds on <16>
    _a("cait", 1, 240, 4, 8, "dense"),           # 62 464 B: below raise_lds on <4>
    _a("cait", 1, 256, 4, 8, "dense"),           # 66 560 B: above it
    _a("cait", 1, 17, 2, 64, "dense"),           # H ND = 8 wave tasks
    _a("cait", 1, 17, 2, 80, "dense"),           # H ND = 10: the third trip of `t += 4`
)
CONVIT_CASES = (
    _a("convit", 1, 1, 1, 4, "gated"),           # the smallest
    _a("convit", 1, 15, 2, 8, "gated"),
    _a("convit", 1, 16, 2, 8, "gated"),
    _a("convit", 1, 17, 2, 8, "gated"),
    _a("convit", 1, 17, 2, 8, "ungated"),
    _a("convit", 1, 17, 2, 8, "huge"),
    _a("convit", 1, 17, 2, 8, "spike"),
    _a("convit", 1, 17, 2, 8, "equal"),
    _a("convit", 1, 17, 2, 8, "c0"),
    _a("convit", 1, 17, 2, 8, "c1z"),
    _a("convit", 1, 17, 2, 8, "zrows"),
    _a("convit", 3, 17, 2, 8, "gated"),          # frame offsets
    _a("convit", 3, 17, 2, 8, "ungated"),
    _a("convit", 1, 17, 1, 4, "gated"),          # dh 4, one head
    _a("convit", 1, 17, 2, 80, "gated"),         # ND = 5: the second trip of the column-tile loop; 10 wave tasks in the key-tile launch
    _a("convit", 1, 63, 3, 20, "gated"),
    _a("convit", 1, 64, 3, 20, "gated"),
    _a("convit", 1, 65, 3, 20, "gated"),
    _a("convit", 1, 65, 3, 20, "ungated"),
    _a("convit", 1, 65, 3, 20, "huge"),
    _a("convit", 1, 65, 3, 20, "spike"),
    _a("convit", 1, 65, 3, 20, "c1z"),
    _a("convit", 2, 33, 3, 12, "c0"),
    _a("convit", 2, 33, 5, 12, "ungated"),
    _a("convit", 1, 1008, 1, 4, "ungated"),      # 64 768 B: below raise_lds
    _a("convit", 1, 1009, 1, 4, "gated"),        # 65 792 B: above it; ld 1012
)
POS_CASES = tuple(_s("pos", F, T, C) for C in (4, 8, 68) for T in (1, 3) for F in (1, 3))
JOIN_CASES = tuple(_s("join", F, T, C) for C in (4, 8, 68) for T in (1, 3) for F in (1, 3))
ATTN_CASES = CAIT_CASES + CONVIT_CASES
CASES = ATTN_CASES + POS_CASES + JOIN_CASES
BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES)
FRAME_INVARIANCE = tuple(c.id for c in ATTN_CASES if c.kw["F"] > 1)
# (CaiT `identity`, the ungated ConViT case on the same shape): the same fma chains and the same butterfly, so the same values
IDENTITY_PAIRS = tuple((f"cait-{s}-identity", f"convit-{s}-ungated") for s in ("f1-T17-h2-dh8", "f1-T65-h3-dh20", "f2-T33-h5-dh12"))
# (c = 1 with a zero table, the ungated case on the same shape): fma(1, p, 0) has p's bits
C1Z_PAIRS = tuple((f"convit-{s}-c1z", f"convit-{s}-ungated") for s in ("f1-T17-h2-dh8", "f1-T65-h3-dh20"))
ONE_HEAD = ("convit-f1-T65-h3-dh20-gated", "convit-f2-T33-h3-dh12-c0", "convit-f3-T17-h2-dh8-ungated")


def probs_ld(T):
    return (T + 3) // 4 * 4


def lds_bytes(case: Case):
    kw = case.kw
    return (kw["H"] if case.op == "cait" else 1) * 16 * ((kw["T"] + 15) // 16 * 16 + 4) * 4


def c0_head(kw):
    return kw["H"] - 1


# ---------------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------------
def _shape_seed(kw):
    """One seed per shape: a CaiT case and the ConViT case of the same shape share qkv and dout (the exact pair checks need it)."""
    return zlib.crc32(f"f{kw['F']}-T{kw['T']}-h{kw['H']}-dh{kw['dh']}".encode())


def _hot_qkv(rn, F, T, H, dh, kind):
    """qkv of the `huge` and `spike` kinds.  Directions e0, e1 of the head width carry the structure, the other dh - 2 are N(0, 1).
    huge   q = +-20 sqrt(dh) e0 by row parity, k = (10 + 0.1 N(0, 1)) e0: scale q k = +-(200 + 2 N(0, 1)) -- even rows have maxima beyond
           +100, odd rows all logits below -100.
    spike  q = 10 sqrt(dh) e0 (even rows) or e1 (odd rows); key T - 1 = (4, -8), key 0 = (-8, 4), every other key (-8, -8) in (e0, e1):
           an even row sees +40 at its last key and -80 elsewhere, an odd row +40 at key 0.  The gap of 120 survives any mix with
           positive weights and a diagonal of one, and no logit reaches exp's overflow: the softmax is one-hot with or without the max."""
    qkv = rn(F, T, 3, H, dh)
    q, k = qkv[:, :, 0], qkv[:, :, 1]
    even = (torch.arange(T) % 2 == 0).view(1, T, 1)
    s = dh ** 0.5
    if kind == "huge":
        q[..., 0] = torch.where(even, 20.0 * s, -20.0 * s)
        k[..., 0] = 10 + 0.1 * rn(F, T, H)
    else:
        q[..., 0] = torch.where(even, 10.0 * s, 0.0)
        q[..., 1] = torch.where(even, 0.0, 10.0 * s)
        k[..., 0], k[..., 1] = -8.0, -8.0
        k[:, T - 1, :, 0] = 4.0
        k[:, 0, :, 1] = 4.0
    return qkv.reshape(F, T, 3 * H * dh)


@functools.lru_cache(maxsize=None)
def inputs(case: Case):
    """{name: float32 CPU tensor} in the operation's own shapes (no padding); read-only, shared by run and reference."""
    kw = case.kw
    if case.op in ("pos", "join"):
        g = torch.Generator().manual_seed(zlib.crc32(case.id.encode()))
        rn = lambda *s: torch.randn(*s, generator=g)
        F, T, C = kw["F"], kw["T"], kw["C"]
        if case.op == "pos":
            return {"x": rn(F, T, C), "pos": rn(T, C)}
        return {"x": rn(F, T, C), "cls": rn(C), "dout": rn(F, T + 1, C), "add": rn(F, T, C)}
    F, T, H, dh, kind = kw["F"], kw["T"], kw["H"], kw["dh"], kw["kind"]
    g = torch.Generator().manual_seed(_shape_seed(kw))
    rn = lambda *s: torch.randn(*s, generator=g)
    qkv, dout = rn(F, T, 3 * H * dh), rn(F, T, H * dh)
    g = torch.Generator().manual_seed(zlib.crc32(case.id.encode()))
    if kind in ("huge", "spike"):
        qkv = _hot_qkv(rn, F, T, H, dh, kind)
    elif kind == "equal":
        qkv = qkv.clone()
        qkv.view(F, T, 3, H * dh)[:, :, 0] = 0.0
    inp = {"qkv": qkv.contiguous(), "dout": dout}
    if case.op == "cait":
        eye = torch.eye(H)
        if kind == "identity":
            inp.update(wl=eye, bl=torch.zeros(H), ww=eye.clone(), bw=torch.zeros(H))
        else:
            # dense: full random mixes with negative entries (P' leaves [0, 1]); huge, spike, equal: a positive first mix with a diagonal
            # above one, so that the sign and the gap of the structured logits survive it
            wl = 0.7 * rn(H, H) if kind in ("dense", "bl-large") else eye + 0.25 * torch.rand(H, H, generator=g)
            inp.update(wl=wl, bl=(50.0 if kind == "bl-large" else 0.3) * rn(H), ww=0.7 * rn(H, H), bw=0.2 * rn(H))
        return inp
    if kind != "ungated":
        c = 0.1 + 0.8 * torch.rand(H, generator=g)
        table = torch.rand(H, T, T, generator=g) * (2.0 / T)
        if kind == "c0":
            c[c0_head(kw)] = 0.0
        elif kind == "c1z":
            c, table = torch.ones(H), torch.zeros(H, T, T)
        elif kind == "zrows":
            table[:, ::3] = 0.0                      # rows 0, 3, ..., of every head: the last row of T = 17 is not among them
        inp.update(c=c, table=table)
    return inp


# ---------------------------------------------------------------------------------------------------------------------------
# references: plain torch in `dt`.  `cait` and `convit` are the functions under reference (the CPU test passes wrong variants)
# ---------------------------------------------------------------------------------------------------------------------------
def _slack(n):
    return ("exact", torch.full((n,), SENTINEL))


def _tail(row):
    return 64 * row + 256


def _scale(dh, dt):
    return torch.tensor(dh ** -0.5, dtype=torch.float32).to(dt)


def _heads_first(t, H):
    """(F, T, H dh) -> (F, H, T, dh)"""
    return t.reshape(t.shape[0], t.shape[1], H, -1).permute(0, 2, 1, 3)


def zero_ds_planes(case: Case):
    """(F, H) bool: the (frame, head) planes of the score gradient that are zero by construction -- T = 1 (P = 1: dP - dP), `spike`
    (P one-hot), and head `c0_head` of the `c0` kind (c dP = 0)."""
    kw = case.kw
    z = torch.zeros(kw["F"], kw["H"], dtype=torch.bool)
    if kw["T"] == 1 or kw["kind"] == "spike":
        z[:] = True
    if kw["kind"] == "c0":
        z[:, c0_head(kw)] = True
    return z


def logits(case: Case):
    """The float64 logits the softmax of the case sees, (F, H, T, T): after the first head mix for CaiT."""
    kw, inp = case.kw, inputs(case)
    F, T, H, dh = kw["F"], kw["T"], kw["H"], kw["dh"]
    q, k, _ = inp["qkv"].double().reshape(F, T, 3, H, dh).permute(2, 0, 3, 1, 4)
    a = (q * _scale(dh, torch.float64)) @ k.transpose(-2, -1)
    if case.op == "cait":
        a = torch.nn.functional.linear(a.permute(0, 2, 3, 1), inp["wl"].double(), inp["bl"].double()).permute(0, 3, 1, 2)
    return a


def evaluate(case: Case, dt=torch.float64, cait=car.talking_heads, convit=cvr.blend_attention):
    kw, inp = case.kw, inputs(case)
    if case.op == "pos":
        # one float32 add per element, correctly rounded: `dt` plays no part
        F, T, C = kw["F"], kw["T"], kw["C"]
        return {"x": ("exact", (inp["x"].double() + inp["pos"].double()).float()), "x_slack": _slack(FRONT + _tail(C))}
    if case.op == "join":
        F, T, C = kw["F"], kw["T"], kw["C"]
        out = torch.cat([inp["cls"].expand(F, 1, C), inp["x"]], 1).contiguous()
        dx = inp["dout"][:, 1:].contiguous()
        return {"out": ("exact", out), "out_slack": _slack(FRONT + _tail(C)), "dx": ("exact", dx), "dx_slack": _slack(FRONT + _tail(C)),
                "dx_add": ("exact", (dx.double() + inp["add"].double()).float()), "dx_add_slack": _slack(FRONT + _tail(C))}
    F, T, H, dh = kw["F"], kw["T"], kw["H"], kw["dh"]
    C, ld = H * dh, probs_ld(T)
    qkv = inp["qkv"].to(dt).requires_grad_(True)
    if case.op == "cait":
        out, p = cait(qkv, H, _scale(dh, dt), *(inp[n].to(dt) for n in ("wl", "bl", "ww", "bw")))
    else:
        gated = "c" in inp
        out, p = convit(qkv, H, _scale(dh, dt), inp["c"].to(dt) if gated else None, inp["table"].to(dt) if gated else None)
    dq, dk, dv = (_heads_first(t, H).contiguous() for t in torch.autograd.grad(out, qkv, inp["dout"].to(dt))[0].reshape(F, T, 3, C).unbind(2))
    if kw["kind"] == "spike":
        # float64's exp(-120) = 8e-53 is not yet zero where float32's is: what is left of dS (below the smallest float32, asserted in
        # tests/test_attn_edge_cpu.py) is rounded to the zero a float32 softmax must give
        assert float(dq.abs().max()) < 1e-38 and float(dk.abs().max()) < 1e-38
        dq, dk = torch.zeros_like(dq), torch.zeros_like(dk)
    n_pad = F * H * T * (ld - T) + FRONT + _tail(ld)
    ref = {"probs": ("planes", p.detach()), "probs_slack": _slack(n_pad), "out": ("planes", _heads_first(out.detach(), H).contiguous()),
           "out_slack": _slack(FRONT + _tail(C)), "dq": ("planes", dq), "dk": ("planes", dk), "dv": ("planes", dv),
           "dqkv_slack": _slack(FRONT + _tail(3 * C)), "dS_slack": _slack(n_pad),
           "dS_zero": ("exact", zero_ds_planes(case).to(torch.int32))}
    if case.op == "cait":
        ref["Pm_slack"] = _slack(n_pad)
    return ref


@functools.lru_cache(maxsize=None)
def reference(case: Case):
    return evaluate(case)


def plane_errors(got, want):
    """(errors, zero): per (frame, head) plane of (F, H, ...) tensors max|got - want| / max|want| -- the worst slice of the plane, every
    slice being normalised by the plane's largest |want| --, inf where got is not finite; `zero`: the planes whose reference is exactly
    zero, whose error is 0 where got is exactly zero as well and inf where it is not."""
    assert got.shape == want.shape, (tuple(got.shape), tuple(want.shape))
    g, w = got.double().flatten(2), want.double().flatten(2)
    scale = w.abs().amax(2)
    zero = scale == 0
    err = (g - w).abs().amax(2) / torch.where(zero, torch.ones_like(scale), scale)
    err = torch.where(zero, torch.where((g == 0).all(2), 0.0, float("inf")).to(err.dtype), err)
    return torch.where(torch.isfinite(g).all(2), err, torch.full_like(err, float("inf"))), zero


def error(got, want):
    return float(plane_errors(got, want)[0].max())


def fp32_errors(case: Case):
    """{output: error of the float32 CPU evaluation of the reference against its float64 evaluation} for the `planes` outputs."""
    r64, r32 = reference(case), evaluate(case, torch.float32)
    return {name: error(r32[name][1], want) for name, (kind, want) in r64.items() if kind == "planes"}


def as_got(evaluated):
    """What a kernel computing `evaluated` exactly would hand back: float32 tensors by name."""
    return {name: (t.clone() if t.dtype == torch.int32 else t.to(torch.float32, copy=True)) for name, (_, t) in evaluated.items()}


def check(case: Case, got, e32, report=None):
    """Hold every output of `got` to its bound; `e32`: this case's entry of the committed fixture ({} for the small launches).  Returns
    {output: error}."""
    ref = reference(case)
    assert set(got) == set(ref), (case.id, sorted(got), sorted(ref))
    assert set(e32) == {n for n, (k, _) in ref.items() if k == "planes"}, (case.id, sorted(e32))
    errs = {}
    for name, (kind, want) in ref.items():
        g = got[name]
        if kind == "exact":
            assert g.dtype == want.dtype and same_bits(g, want), (
                f"{case.id}: {name} differs from the exact reference at "
                f"{int((g.contiguous().view(torch.int32) != want.contiguous().view(torch.int32)).sum()) if g.shape == want.shape else 'every'} of {want.numel()} element(s)")
            continue
        per, zero = plane_errors(g, want)
        assert not bool(zero.all()) or name in ("dq", "dk"), (case.id, name)          # only a gradient may have nothing to measure
        assert bool((per[zero] == 0).all()), f"{case.id}: {name} is not exactly zero in {int((per[zero] != 0).sum())} plane(s) whose reference is"
        errs[name] = float(per.max())
        if report is not None:
            report(f"{case.id:34s} {name:5s} error {errs[name]:.3g}  bound {bound(e32[name]):.3g}  (e32 {e32[name]:.3g})")
    for name, err in errs.items():
        assert err <= bound(e32[name]), f"{case.id}: {name} error {err:.3g} > bound {bound(e32[name]):.3g} = max({FLOOR:g}, 4 * {e32[name]:.3g})"
    return errs


# ---------------------------------------------------------------------------------------------------------------------------
# running a case through the C entries
# ---------------------------------------------------------------------------------------------------------------------------
class _Ctx(_XfCtx):
    def __init__(self, eng):
        super().__init__(eng)
        if not getattr(self.capi, "_attn_edge_bound", False):
            lib.bind(self.capi, lib._CAIT_PROTOS)
            lib.bind(self.capi, lib._CONVIT_PROTOS)
            self.capi._attn_edge_bound = True


def _probs_buf(cx, F, H, T, data, fill):
    ld = probs_ld(T)
    idx = FRONT + (torch.arange(F * H * T).view(F, H, T, 1) * ld + torch.arange(T).view(1, 1, 1, -1))
    return _Buf(cx, FRONT + F * H * T * ld + _tail(ld), idx, data, fill)


def _table_buf(cx, table):
    H, T = table.shape[:2]
    ld = probs_ld(T)
    idx = FRONT + (torch.arange(H * T).view(H, T, 1) * ld + torch.arange(T).view(1, 1, -1))
    return _Buf(cx, FRONT + H * T * ld + _tail(ld), idx, table, float("nan"))


def _run_attn(cx, case, inp, frames=None, head=None):
    """`frames` = k: the first k frames as a call of their own; `head` = h (ConViT): head h as a 1-head call on its columns."""
    kw = case.kw
    F, T, H, dh = kw["F"] if frames is None else frames, kw["T"], kw["H"], kw["dh"]
    qkv, dout = inp["qkv"][:F], inp["dout"][:F]
    c, table = inp.get("c"), inp.get("table")
    if head is not None:
        assert case.op == "convit"
        qkv = qkv.reshape(F, T, 3, H, dh)[:, :, :, head].reshape(F, T, 3 * dh)
        dout = dout.reshape(F, T, H, dh)[:, :, head].reshape(F, T, dh)
        c, table = (None, None) if c is None else (c[head:head + 1], table[head:head + 1])
        H = 1
    C, scale, F_ = H * dh, dh ** -0.5, FRONT
    nan = float("nan")
    qb, db = _inb(cx, qkv, 0, _tail(3 * C)), _inb(cx, dout, 0, _tail(C))
    probs = _probs_buf(cx, F, H, T, torch.full((F, H, T, T), nan), SENTINEL)
    o, dqkv = _outb(cx, F * T * C, 0, _tail(C)), _outb(cx, F * T * 3 * C, 0, _tail(3 * C))
    dS = _probs_buf(cx, F, H, T, torch.full((F, H, T, T), nan), SENTINEL)
    out = {}
    if case.op == "cait":
        wl, bl, ww, bw = (_inb(cx, inp[n]) for n in ("wl", "bl", "ww", "bw"))
        cx.call("i2v_cait_attention_f32", qb.ptr(F_), F, T, H, dh, scale, wl.ptr(F_), bl.ptr(F_), ww.ptr(F_), bw.ptr(F_), probs.ptr(F_), o.ptr(F_))
        probs.collect(out, "probs")
        pin = _probs_buf(cx, F, H, T, out["probs"], nan)               # the backward's input: NaN in the pad columns
        Pm = _probs_buf(cx, F, H, T, torch.full((F, H, T, T), nan), SENTINEL)
        cx.call("i2v_cait_attention_bwd_f32", qb.ptr(F_), pin.ptr(F_), db.ptr(F_), F, T, H, dh, scale, wl.ptr(F_), ww.ptr(F_), bw.ptr(F_),
                dS.ptr(F_), Pm.ptr(F_), dqkv.ptr(F_))
        Pm.collect(out, "Pm")
        del out["Pm"]
    else:
        cb = _inb(cx, c) if c is not None else None
        tb = _table_buf(cx, table) if table is not None else None
        cp, tp = (cb.ptr(F_), tb.ptr(F_)) if cb is not None else (NULL, NULL)
        cx.call("i2v_convit_attention_f32", qb.ptr(F_), F, T, H, dh, scale, cp, tp, probs.ptr(F_), o.ptr(F_))
        probs.collect(out, "probs")
        pin = _probs_buf(cx, F, H, T, out["probs"], nan)
        cx.call("i2v_convit_attention_bwd_f32", qb.ptr(F_), pin.ptr(F_), db.ptr(F_), F, T, H, dh, scale, cp, tp, dS.ptr(F_), dqkv.ptr(F_))
    o.collect(out, "out", (F, T, C))
    out["out"] = _heads_first(out["out"], H).contiguous()
    dqkv.collect(out, "dqkv", (F, T, 3, C))
    out["dq"], out["dk"], out["dv"] = (_heads_first(t, H).contiguous() for t in out.pop("dqkv").unbind(2))
    dS.collect(out, "dS")
    ds = out.pop("dS")
    out["dS_zero"] = (ds == 0).flatten(2).all(2).to(torch.int32)
    if head is None and frames is None:
        out["dS_zero"] = out["dS_zero"] * zero_ds_planes(case).to(torch.int32)         # only the planes that must be zero are asserted
    return out


def _run_pos(cx, case, inp):
    kw = case.kw
    F, T, C = kw["F"], kw["T"], kw["C"]
    x, pos = _outb(cx, F * T * C, 0, _tail(C), init=inp["x"]), _inb(cx, inp["pos"], 0, _tail(C))
    cx.call("i2v_cait_add_pos_f32", x.ptr(FRONT), pos.ptr(FRONT), F, T, C)
    out = {}
    x.collect(out, "x", (F, T, C))
    return out


def _run_join(cx, case, inp):
    kw = case.kw
    F, T, C, F_ = kw["F"], kw["T"], kw["C"], FRONT
    x, cls, dout, add = _inb(cx, inp["x"], 0, _tail(C)), _inb(cx, inp["cls"]), _inb(cx, inp["dout"], 0, _tail(C)), _inb(cx, inp["add"], 0, _tail(C))
    o, dx, dxa = _outb(cx, F * (T + 1) * C, 0, _tail(C)), _outb(cx, F * T * C, 0, _tail(C)), _outb(cx, F * T * C, 0, _tail(C))
    cx.call("i2v_convit_join_cls_f32", x.ptr(F_), cls.ptr(F_), o.ptr(F_), F, T, C)
    cx.call("i2v_convit_join_cls_bwd_f32", dout.ptr(F_), NULL, dx.ptr(F_), F, T, C)
    cx.call("i2v_convit_join_cls_bwd_f32", dout.ptr(F_), add.ptr(F_), dxa.ptr(F_), F, T, C)
    out = {}
    o.collect(out, "out", (F, T + 1, C))
    dx.collect(out, "dx", (F, T, C))
    dxa.collect(out, "dx_add", (F, T, C))
    return out


def run(engine, case: Case, **how):
    """The case through the C entries of `engine.capi`: {name: CPU tensor} over the names of `reference(case)`.  Attention cases take
    frames = k (the first k frames as a call of their own) and, ConViT, head = h (head h as a 1-head call on its columns)."""
    cx = _Ctx(engine)
    if case.op in ("cait", "convit"):
        return _run_attn(cx, case, inputs(case), **how)
    return (_run_pos if case.op == "pos" else _run_join)(cx, case, inputs(case))


# ---------------------------------------------------------------------------------------------------------------------------
# refusals: (label, the name the message starts with, thunk returning the status); `untouched()`: every output sentinel is in place
# ---------------------------------------------------------------------------------------------------------------------------
def small_refusals(engine):
    """The three small launches: C % 4 != 0, a misaligned pointer, a null pointer, each operand in turn."""
    cx = _Ctx(engine)
    capi, s = cx.capi, cx.eng.stream
    F, T, C = 2, 3, 8
    dev = cx.eng.device
    zeros = lambda n: torch.zeros(n + 8, device=dev)
    sents = lambda n: torch.full((n + 8,), SENTINEL, device=dev)
    x, pos, cls, dout, add = zeros(F * T * C), zeros(T * C), zeros(C), zeros(F * (T + 1) * C), zeros(F * T * C)
    xs, out, dx = sents(F * T * C), sents(F * (T + 1) * C), sents(F * T * C)
    p = lambda t, off=0: P(t.data_ptr() + 4 * off)

    def ap(x=p(xs), pos=p(pos), F=F, T=T, C=C):
        return lambda: capi.i2v_cait_add_pos_f32(x, pos, F, T, C, s())

    def jo(x=p(x), cls=p(cls), out=p(out), F=F, T=T, C=C):
        return lambda: capi.i2v_convit_join_cls_f32(x, cls, out, F, T, C, s())

    def jb(dout=p(dout), add=p(add), dx=p(dx), F=F, T=T, C=C):
        return lambda: capi.i2v_convit_join_cls_bwd_f32(dout, add, dx, F, T, C, s())
    thunks = []
    for who, mk, ptrs, optional in (("cait_add_pos", ap, {"x": xs, "pos": pos}, ()), ("convit_join_cls", jo, {"x": x, "cls": cls, "out": out}, ()),
                                    ("convit_join_cls_bwd", jb, {"dout": dout, "add": add, "dx": dx}, ("add",))):
        thunks += [(f"null {k}", who, mk(**{k: NULL})) for k in ptrs if k not in optional]
        thunks += [(f"misaligned {k}", who, mk(**{k: p(t, 1)})) for k, t in ptrs.items()]
        thunks += [(f"misaligned {k} by 8 bytes", who, mk(**{k: p(t, 2)})) for k, t in ptrs.items()]
        thunks += [("C % 4", who, mk(C=6)), ("C = 0", who, mk(C=0)), ("T = 0", who, mk(T=0)), ("F = 0", who, mk(F=0)), ("F < 0", who, mk(F=-1))]
    thunks += [("2^31 elements", "convit_join_cls", jo(F=65536, T=127, C=256)), ("2^31 elements", "convit_join_cls_bwd", jb(F=65536, T=127, C=256))]

    def untouched():
        cx.sync()
        return all(bool((t == SENTINEL).all()) for t in (xs, out, dx))
    return thunks, untouched, (x, pos, cls, dout, add, xs, out, dx)


def boundary_calls(engine, op, T, H, dh=4):
    """One forward and one backward call at (1, T, H, dh) on zero operands with SENTINEL outputs: (forward status, backward status,
    touched: whether any output element left SENTINEL behind).  For the LDS refusal boundaries."""
    cx = _Ctx(engine)
    capi, s, dev = cx.capi, cx.eng.stream, cx.eng.device
    C, ld = H * dh, probs_ld(T)
    zeros = lambda n: torch.zeros(n + 8, device=dev)
    sents = lambda n: torch.full((n + 8,), SENTINEL, device=dev)
    qkv, dout, probs_in, w = zeros(T * 3 * C), zeros(T * C), zeros(H * T * ld), zeros(H * H + H)
    probs, o, dS, Pm, dqkv = sents(H * T * ld), sents(T * C), sents(H * T * ld), sents(H * T * ld), sents(T * 3 * C)
    p = lambda t: P(t.data_ptr())
    if op == "cait":
        fwd = capi.i2v_cait_attention_f32(p(qkv), 1, T, H, dh, 0.5, p(w), p(w), p(w), p(w), p(probs), p(o), s())
        bwd = capi.i2v_cait_attention_bwd_f32(p(qkv), p(probs_in), p(dout), 1, T, H, dh, 0.5, p(w), p(w), p(w), p(dS), p(Pm), p(dqkv), s())
    else:
        fwd = capi.i2v_convit_attention_f32(p(qkv), 1, T, H, dh, 0.5, NULL, NULL, p(probs), p(o), s())
        bwd = capi.i2v_convit_attention_bwd_f32(p(qkv), p(probs_in), p(dout), 1, T, H, dh, 0.5, NULL, NULL, p(dS), p(dqkv), s())
    cx.sync()
    touched = [n for n, t in (("probs", probs), ("out", o), ("dS", dS), ("dqkv", dqkv)) if not bool((t == SENTINEL).all())]
    return fwd, bwd, touched
