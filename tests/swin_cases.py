"""TEST INFRASTRUCTURE: the case table of the two launches of csrc/i2v_swin.hip that three families run on -- `swin_window_attention(_bwd)`
(every Swin block, and every Twins-SVT window block through `twins_window_attention`, which calls it at shift 0 with a zero table) and
`swin_merge_gather` / `swin_merge_scatter` (Swin, ConvNeXt, Twins) --, with input generators and a reference per case.  Neither launch
has a scalar twin in the host simulation: tests/test_gpu_swin_kernels.py runs the table on the device, tests/test_swin_kernels_cpu.py
checks on the CPU that the table, the reference and `check` can tell a wrong kernel from a right one.  The buffer helpers are those of
tests/xf_cases.py, imported.

`run(engine, case)` calls the C entries (include/i2v_swin.h, include/i2v_twins.h) through `engine.capi` and returns {name: CPU tensor};
`reference(case)` returns {name: (kind, tensor)} over the SAME names.

Kinds and bounds (`check`):
  blocks   the error is taken per (frame, window, head) block, partitioned as the kernel partitions its work: `got` and `want` are rolled
           by -shift, cut into windows and split into heads; within a block max|got - want| / max|want|; the case's error is its worst
           block, held to max(2e-6, 4 e32) (2e-6: tests/loop_cases.py's `tensor` floor; 4: DESIGN.md section 14).  An error confined to
           the masked corner window, or to one head, is not averaged away.  out, dq, dk and dv are four outputs, each on its own.
  exact    equal bits: patch merging (a permutation; with accumulate one correctly rounded add per element), the slack around every output.
e32 is the same measure on the float32 CPU evaluation of the reference against its float64 evaluation, committed as
tests/golden/swin_kernel_fp32_cpu_errors.json (tests/make_swin_kernel_fixtures.py).  Nothing in a bound comes from the device.

Buffers (xf_cases._Buf).  Every operand lies FRONT = 128 floats into a larger flat allocation with a tail of 64 rows + 256 floats (a row
per lane of a wave) behind it.  Everything of an OUTPUT allocation that is not an addressed element is SENTINEL and must come back bit
for bit (`out_slack`, `dqkv_slack`, ...); its addressed elements start as NaN (as the addend where the scatter accumulates).  Everything
of an INPUT allocation that is not an addressed element is NaN: a stray read poisons a checked output.

Branch arithmetic of csrc/i2v_swin.hip (re-derive the comments at the cases when any of it changes):
  swin_attn_fwd_kernel / swin_attn_bwd_kernel: one WAVE per problem, nprob = frames * (H / ws) * (W / ws) * heads problems; FWD_WAVES = 4
    per block forward, BWD_WAVES = 2 backward, ceil(nprob / WAVES) blocks.  A wave with p >= nprob (the spare waves of the last block:
    nprob % 4 != 0 forward, nprob odd backward) recomputes problem nprob - 1 and stores nothing (`live`).
    win_problem: h = p % heads, window w = (p / heads) % nwin, frame = p / heads / nwin, nwin = (H / ws) (W / ws), wy = w / (W / ws),
    wx = w % (W / ws): H and W enter separately, here, in win_token (token row oy * W + ox with oy = (y + shift) mod H, ox = (x + shift)
    mod W, one conditional subtraction each) and in shift_region.
    T = ws^2 tokens: 49 of a wave's 64 lanes at ws 7, 16 at ws 4 (head width 32 and 16); a lane past T repeats row T - 1 and stores nothing.
    The table is read as table[e * heads + h], e < (2 ws - 1)^2, by scalar loads: the head count is its stride, its base needs no alignment.
    Bias of (i, j): Bs[bi - bj], bi = (i / ws + ws - 1)(2 ws - 1) + i % ws + ws - 1, bj = (j / ws)(2 ws - 1) + j % ws.
    Mask, shift != 0 only: region(y, H) * 3 + region(x, W) with region(y, H) = y < H - ws ? 0 : y < H - shift ? 1 : 2 on ROLLED coordinates;
    a pair in different regions gets -100 ADDED to its score (timm's semantics: the key is not excluded; exp(-100) = 3.7e-44 of the row's
    largest term at order-one logits, but a masked key 100 above the rest still wins -- the `hot` cases).  Shift 1 puts one row / column
    in region 2, shift ws - 1 one in region 1.
    The entry serves (ws, dh) = (7, 32) and (4, 16), a grid of whole windows, 0 <= shift < ws, shift != 0 only where H > ws and W > ws,
    nprob <= 2^31 - 1, and 16-byte aligned qkv, out / dout, dqkv.
  swin_merge_kernel: one thread per float4 of the FINE tensor, min(ceil(quads / 256), 65536) blocks of 256: above 65536 * 256 = 16 777 216
    quads the grid-stride loop takes a second trip.  fine (f, y, x, c) <-> merged row (f, y / 2, x / 2), quarter (y & 1) + 2 (x & 1).
    `i2v_swin_merge_bwd_f32` with accumulate passes `add == dx`: the in-place form is the only accumulating form the C ABI has.
"""
import functools
import time
import zlib

import torch

from tests import swin_reference as sr
from tests.xf_cases import FLOOR, FRONT, NULL, SENTINEL, Case, P, _Ctx, _inb, _outb, bound, same_bits

QKV_SCALE, TABLE_SCALE, HOT = 1.5, 0.7, 8.0            # the magnitudes of tests/test_gpu_swin.py; `hot`: qkv times 8
MERGE_CAP = 65536 * 256                                  # quads one trip of the merge grid covers


def _dh(ws):
    return {7: 32, 4: 16}[ws]


def _w(frames, H, W, ws, shift, heads, kind="plain"):
    id = f"win-f{frames}-{H}x{W}-ws{ws}-s{shift}-h{heads}" + ("" if kind == "plain" else "-" + kind)
    return Case(id, "win", tuple(sorted(dict(frames=frames, H=H, W=W, ws=ws, shift=shift, heads=heads, kind=kind).items())))


def _m(frames, H, W, C):
    return Case(f"merge-f{frames}-{H}x{W}-C{C}", "merge", tuple(sorted(dict(frames=frames, H=H, W=W, C=C).items())))


# ---------------------------------------------------------------------------------------------------------------------------
# the table
# ---------------------------------------------------------------------------------------------------------------------------
WIN_CASES = (
    _w(1, 7, 7, 7, 0, 1),               # nprob 1: three spare waves forward, one backward
    _w(1, 7, 7, 7, 0, 3),               # nprob 3: odd; one spare wave forward and backward
    _w(1, 7, 14, 7, 0, 5),              # 1 x 2 windows, nprob 10: two spare waves forward in the third block
    _w(1, 14, 21, 7, 3, 1),             # 2 x 3 windows: all nine mask regions, H < W, nprob 6
    _w(2, 21, 14, 7, 1, 2),             # shift 1 (one row / column in region 2), H > W
    _w(1, 21, 14, 7, 6, 3),             # shift ws - 1 (one row / column in region 1), nprob 18
    _w(3, 14, 14, 7, 3, 7),             # odd head count: the table's stride; nprob 84
    _w(1, 14, 14, 7, 3, 2, "hot"),      # qkv x 8: adding -100 and excluding the key differ (the condition of test_swin_kernels_cpu.py)
    _w(2, 14, 14, 7, 0, 2, "notable"),  # zero table: the Twins route at ws 7
    _w(1, 4, 4, 4, 0, 1),               # nprob 1 at T = 16: 48 lanes repeat row 15
    _w(1, 8, 12, 4, 1, 3),              # rectangular, shift 1
    _w(2, 12, 8, 4, 3, 1),              # shift ws - 1
    _w(1, 8, 8, 4, 2, 5),               # nprob 20, five heads
    _w(1, 8, 8, 4, 2, 5, "hot"),
    _w(5, 4, 8, 4, 0, 1),               # five frames, nprob 10
)
MERGE_CASES = (
    _m(1, 2, 2, 4),                     # one cell, one quad per token: four threads
    _m(2, 2, 6, 4),                     # H != W, two frames
    _m(3, 6, 4, 20),                    # H > W, five quads per token (c4n no power of two)
    _m(1, 14, 10, 96),                  # 3360 quads: 14 blocks, the last of 32 threads
    _m(2, 4, 2, 8),
)
# (1, 2, 4, 8388676): 16 777 352 quads, 136 past the cap -- the second trip of the grid-stride loop, by a count that is no multiple of 256
MERGE_BIG = (1, 2, 4, 8388676)
CASES = WIN_CASES + MERGE_CASES
BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES)
HOT_CASES = tuple(c for c in WIN_CASES if c.kw["kind"] == "hot")
FRAME_INVARIANCE = ("win-f3-14x14-ws7-s3-h7", "win-f5-4x8-ws4-s0-h1")
NOTABLE = "win-f2-14x14-ws7-s0-h2-notable"
WIN_OUTPUTS = ("out", "dq", "dk", "dv")


def nprob(kw):
    return kw["frames"] * (kw["H"] // kw["ws"]) * (kw["W"] // kw["ws"]) * kw["heads"]


# ---------------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def inputs(case: Case):
    """{name: float32 CPU tensor} in the operation's own shapes; read-only, shared by run and reference."""
    kw, g = case.kw, torch.Generator().manual_seed(zlib.crc32(case.id.encode()))
    rn = lambda *s: torch.randn(*s, generator=g)
    if case.op == "win":
        f, T, C, ws = kw["frames"], kw["H"] * kw["W"], kw["heads"] * _dh(kw["ws"]), kw["ws"]
        qkv = QKV_SCALE * rn(f, T, 3 * C) * (HOT if kw["kind"] == "hot" else 1.0)
        table = TABLE_SCALE * rn((2 * ws - 1) ** 2, kw["heads"])
        if kw["kind"] == "notable":
            table = torch.zeros_like(table)
        return {"qkv": qkv, "table": table, "dout": rn(f, T, C)}
    f, H, W, C = kw["frames"], kw["H"], kw["W"], kw["C"]
    return {"x": rn(f, H * W, C), "dmerged": rn(f, H * W // 4, 4 * C), "base": rn(f, H * W, C)}


# ---------------------------------------------------------------------------------------------------------------------------
# references: plain torch in `dt`.  `attention` and `gather` are the functions under reference (the CPU test passes wrong variants)
# ---------------------------------------------------------------------------------------------------------------------------
def _slack(n):
    return ("exact", torch.full((n,), SENTINEL))


def _tail(row):
    return 64 * row + 256


def evaluate(case: Case, dt=torch.float64, attention=sr.window_attention, gather=sr.patch_merge_gather):
    kw, inp = case.kw, inputs(case)
    if case.op == "win":
        f, H, W, C = kw["frames"], kw["H"], kw["W"], kw["heads"] * _dh(kw["ws"])
        qkv = inp["qkv"].to(dt).requires_grad_(True)
        out = attention(qkv, H, W, kw["ws"], kw["shift"], kw["heads"], inp["table"].to(dt))
        dq, dk, dv = torch.autograd.grad(out, qkv, inp["dout"].to(dt))[0].reshape(f, H * W, 3, C).unbind(2)
        return {"out": ("blocks", out.detach()), "dq": ("blocks", dq.contiguous()), "dk": ("blocks", dk.contiguous()), "dv": ("blocks", dv.contiguous()),
                "out_slack": _slack(FRONT + _tail(C)), "dqkv_slack": _slack(FRONT + _tail(3 * C))}
    # merging is exact in float32: `dt` plays no part
    H, W, C = kw["H"], kw["W"], kw["C"]
    x = inp["x"].clone().requires_grad_(True)
    m = gather(x, H, W)
    dx = torch.autograd.grad(m, x, inp["dmerged"])[0]
    return {"merged": ("exact", m.detach().contiguous()), "merged_slack": _slack(FRONT + _tail(4 * C)),
            "dx": ("exact", dx.contiguous()), "dx_slack": _slack(FRONT + _tail(C)),
            "dx_acc": ("exact", (inp["base"] + dx).contiguous()), "dx_acc_slack": _slack(FRONT + _tail(C))}


@functools.lru_cache(maxsize=None)
def reference(case: Case):
    return evaluate(case)


def blocks(t, kw):
    """(frames, H * W, heads * dh) -> (frames * windows * heads, ws^2 * dh): one row per problem of the kernel."""
    H, W, ws, heads = kw["H"], kw["W"], kw["ws"], kw["heads"]
    g = t.reshape(t.shape[0], H, W, -1)
    if kw["shift"]:
        g = torch.roll(g, shifts=(-kw["shift"], -kw["shift"]), dims=(1, 2))
    w = sr.window_partition(g, ws)                                                   # (f * windows, ws^2, C)
    return w.reshape(w.shape[0], ws * ws, heads, -1).permute(0, 2, 1, 3).reshape(w.shape[0] * heads, -1)


def error(got, want, kw):
    """The error of one `blocks` output: the worst (frame, window, head) block of max|got - want| / max|want| within the block."""
    got, want = got.double(), want.double()
    assert got.shape == want.shape, (tuple(got.shape), tuple(want.shape))
    if not bool(torch.isfinite(got).all()):
        return float("inf")
    g, w = blocks(got, kw), blocks(want, kw)
    scale = w.abs().max(1).values
    assert float(scale.min()) > 0
    return float(((g - w).abs().max(1).values / scale).max())


def fp32_errors(case: Case):
    """{output: error of the float32 CPU evaluation of the reference against its float64 evaluation} for the `blocks` outputs."""
    r64, r32 = reference(case), evaluate(case, torch.float32)
    return {name: error(r32[name][1], want, case.kw) for name, (kind, want) in r64.items() if kind == "blocks"}


def as_got(evaluated):
    """What a kernel computing `evaluated` exactly would hand back: float32 tensors by name."""
    return {name: t.to(torch.float32, copy=True) for name, (_, t) in evaluated.items()}


def check(case: Case, got, e32, report=None):
    """Hold every output of `got` to its bound; `e32`: this case's entry of the committed fixture ({} for merging).  Returns {output: error}."""
    ref = reference(case)
    assert set(got) == set(ref), (case.id, sorted(got), sorted(ref))
    assert set(e32) == {n for n, (k, _) in ref.items() if k == "blocks"}, (case.id, sorted(e32))
    errs = {}
    for name, (kind, want) in ref.items():
        g = got[name]
        if kind == "exact":
            assert g.dtype == want.dtype and same_bits(g, want), (
                f"{case.id}: {name} differs from the exact reference at "
                f"{int((g.contiguous().view(torch.int32) != want.contiguous().view(torch.int32)).sum()) if g.shape == want.shape else 'every'} of {want.numel()} element(s)")
            continue
        errs[name] = error(g, want, case.kw)
        if report is not None:
            report(f"{case.id:34s} {name:4s} error {errs[name]:.3g}  bound {bound(e32[name]):.3g}  (e32 {e32[name]:.3g})")
    for name, err in errs.items():
        assert err <= bound(e32[name]), f"{case.id}: {name} error {err:.3g} > bound {bound(e32[name]):.3g} = max({FLOOR:g}, 4 * {e32[name]:.3g})"
    return errs


# ---------------------------------------------------------------------------------------------------------------------------
# running a case through the C entries
# ---------------------------------------------------------------------------------------------------------------------------
def _run_win(cx, case, inp, frames=None, table_off=0, route="swin"):
    kw = case.kw
    H, W, ws, shift, heads = kw["H"], kw["W"], kw["ws"], kw["shift"], kw["heads"]
    f, T, dh = kw["frames"] if frames is None else frames, H * W, _dh(ws)
    C = heads * dh
    qkv, dout = _inb(cx, inp["qkv"][:f], 0, _tail(3 * C)), _inb(cx, inp["dout"][:f], 0, _tail(C))
    table = _inb(cx, inp["table"], table_off)
    o, dqkv = _outb(cx, f * T * C, 0, _tail(C)), _outb(cx, f * T * 3 * C, 0, _tail(3 * C))
    F_ = FRONT
    if route == "swin":
        cx.call("i2v_swin_window_attention_f32", qkv.ptr(F_), f, H, W, ws, shift, heads, dh, table.ptr(F_ + table_off), o.ptr(F_))
        cx.call("i2v_swin_window_attention_bwd_f32", qkv.ptr(F_), dout.ptr(F_), f, H, W, ws, shift, heads, dh, table.ptr(F_ + table_off), dqkv.ptr(F_))
    else:
        assert shift == 0 and not bool(inp["table"].any())
        cx.call("i2v_twins_window_attention_f32", qkv.ptr(F_), f, H, W, ws, heads, dh, table.ptr(F_ + table_off), o.ptr(F_))
        cx.call("i2v_twins_window_attention_bwd_f32", qkv.ptr(F_), dout.ptr(F_), f, H, W, ws, heads, dh, table.ptr(F_ + table_off), dqkv.ptr(F_))
    out = {}
    o.collect(out, "out", (f, T, C))
    dqkv.collect(out, "dqkv", (f, T, 3, C))
    out["dq"], out["dk"], out["dv"] = (t.contiguous() for t in out.pop("dqkv").unbind(2))
    return out


def _run_merge(cx, case, inp):
    kw = case.kw
    f, H, W, C = kw["frames"], kw["H"], kw["W"], kw["C"]
    n = f * H * W * C
    x, dm = _inb(cx, inp["x"], 0, _tail(C)), _inb(cx, inp["dmerged"], 0, _tail(4 * C))
    merged, dx, dxa = _outb(cx, n, 0, _tail(4 * C)), _outb(cx, n, 0, _tail(C)), _outb(cx, n, 0, _tail(C), init=inp["base"])
    F_ = FRONT
    cx.call("i2v_swin_merge_f32", x.ptr(F_), f, H, W, C, merged.ptr(F_))
    cx.call("i2v_swin_merge_bwd_f32", dm.ptr(F_), f, H, W, C, dx.ptr(F_), 0)
    cx.call("i2v_swin_merge_bwd_f32", dm.ptr(F_), f, H, W, C, dxa.ptr(F_), 1)         # add == dx inside the entry
    out = {}
    merged.collect(out, "merged", (f, H * W // 4, 4 * C))
    dx.collect(out, "dx", (f, H * W, C))
    dxa.collect(out, "dx_acc", (f, H * W, C))
    return out


def run(engine, case: Case, **how):
    """The case through the C entries of `engine.capi`: {name: CPU tensor} over the names of `reference(case)`.  Window cases take
    frames = k (the first k frames as a call of their own), table_off = 1 (the table one float off 16-byte alignment), route = "twins"."""
    return (_run_win if case.op == "win" else _run_merge)(_Ctx(engine), case, inputs(case), **how)


def run_merge_big(engine, scatter=True):
    """MERGE_BIG on the device: element i of the input holds the int32 i (viewed as float32), so the copy is bitwise and every element
    names where it came from.  The gather is compared with `sr.patch_merge_gather` of the same integers; the scatter (accumulate 0) of
    the gathered tensor is the inverse permutation and must give the integers back.  Compared on the device as int32, slack included.
    Returns (mismatches, seconds of the launches)."""
    cx = _Ctx(engine)
    f, H, W, C = MERGE_BIG
    n, dev = f * H * W * C, engine.device
    assert n // 4 > MERGE_CAP and (n // 4 - MERGE_CAP) % 256 != 0
    sent = torch.tensor([SENTINEL]).view(torch.int32).item()

    def alloc(fill):
        t = torch.full((FRONT + n + 256,), sent, dtype=torch.int32, device=dev)
        if fill is not None:
            t[FRONT:FRONT + n] = fill
        return t
    x = alloc(torch.arange(n, dtype=torch.int32, device=dev))
    merged, back = alloc(-1), alloc(-1) if scatter else None
    ptr = lambda t: P(t.data_ptr() + 4 * FRONT)
    cx.sync()
    t0 = time.perf_counter()
    cx.call("i2v_swin_merge_f32", ptr(x), f, H, W, C, ptr(merged))
    if scatter:
        cx.call("i2v_swin_merge_bwd_f32", ptr(merged), f, H, W, C, ptr(back), 0)
    cx.sync()
    seconds = time.perf_counter() - t0
    want = sr.patch_merge_gather(x[FRONT:FRONT + n].view(f, H * W, C), H, W).reshape(-1)
    bad = {"merged": int((merged[FRONT:FRONT + n] != want).sum())}
    del want
    for name, t in (("merged", merged), ("back", back)):
        if t is not None:
            bad[name + "_slack"] = int((t[:FRONT] != sent).sum()) + int((t[FRONT + n:] != sent).sum())
    if scatter:
        bad["back"] = int((back != x).sum())
    return bad, seconds


# ---------------------------------------------------------------------------------------------------------------------------
# refusals: (label, the name the message starts with, thunk returning the status); `untouched()`: every output sentinel is in place
# ---------------------------------------------------------------------------------------------------------------------------
def refusals(engine):
    cx = _Ctx(engine)
    capi, s = cx.capi, cx.eng.stream
    F, H, W, ws, shift, heads, dh = 1, 14, 14, 7, 3, 2, 32              # an ordinary shape: each thunk spoils one argument of it
    C, T = heads * dh, H * W
    zeros = lambda n: torch.zeros(n + 8, device=cx.eng.device)
    sents = lambda n: torch.full((n + 8,), SENTINEL, device=cx.eng.device)
    qkv, dout, table = zeros(F * T * 3 * C), zeros(F * T * C), zeros(169 * heads)
    out, dqkv = sents(F * T * C), sents(F * T * 3 * C)
    mx, mdm, mout, mdx = zeros(4 * 4 * 8), zeros(4 * 4 * 8), sents(4 * 4 * 8), sents(4 * 4 * 8)
    p = lambda t, off=0: P(t.data_ptr() + 4 * off)
    fw, bw = capi.i2v_swin_window_attention_f32, capi.i2v_swin_window_attention_bwd_f32
    ga, sc = capi.i2v_swin_merge_f32, capi.i2v_swin_merge_bwd_f32

    def fwd(q=p(qkv), t=p(table), o=p(out), F=F, H=H, W=W, ws=ws, shift=shift, heads=heads, dh=dh):
        return lambda: fw(q, F, H, W, ws, shift, heads, dh, t, o, s())

    def bwd(q=p(qkv), d=p(dout), t=p(table), g=p(dqkv), F=F, H=H, W=W, ws=ws, shift=shift, heads=heads, dh=dh):
        return lambda: bw(q, d, F, H, W, ws, shift, heads, dh, t, g, s())

    def gather(x=p(mx), o=p(mout), H=4, W=4, C=8):
        return lambda: ga(x, 1, H, W, C, o, s())

    def scatter(d=p(mdm), o=p(mdx), H=4, W=4, C=8, acc=0):
        return lambda: sc(d, 1, H, W, C, o, acc, s())
    thunks = []
    for who, mk, ptrs in (("swin_window_attention", fwd, {"q": qkv, "t": table, "o": out}),
                          ("swin_window_attention_bwd", bwd, {"q": qkv, "d": dout, "t": table, "g": dqkv})):
        thunks += [(f"null {k}", who, mk(**{k: NULL})) for k in ptrs]
        thunks += [(f"misaligned {k}", who, mk(**{k: p(t, 1)})) for k, t in ptrs.items() if k != "t"]
        thunks += [("H % ws", who, mk(H=10)), ("W % ws", who, mk(W=10)), ("shift = ws", who, mk(shift=ws)), ("shift < 0", who, mk(shift=-1)),
                   ("shift with H = ws", who, mk(H=7)), ("shift with W = ws", who, mk(W=7)),
                   ("ws 7 with dh 16", who, mk(dh=16)), ("ws 4 with dh 32", who, mk(H=8, W=8, ws=4, shift=2)),
                   ("ws 6", who, mk(H=12, W=12, ws=6)), ("ws 4 with dh 16 at shift ws", who, mk(H=8, W=8, ws=4, dh=16, shift=4)),
                   ("2^31 problems", who, mk(F=65536, H=112, W=112, shift=0, heads=128))]     # 65536 * 256 * 128 = 2^31; nothing is launched
    for who, mk, ptrs in (("swin_merge_gather", gather, {"x": mx, "o": mout}), ("swin_merge_scatter", scatter, {"d": mdm, "o": mdx})):
        thunks += [(f"null {k}", who, mk(**{k: NULL})) for k in ptrs]
        thunks += [(f"misaligned {k}", who, mk(**{k: p(t, 1)})) for k, t in ptrs.items()]
        thunks += [("odd H", who, mk(H=3)), ("odd W", who, mk(W=3)), ("C % 4", who, mk(C=6))]
    thunks.append(("misaligned dx, accumulating", "swin_merge_scatter", scatter(o=p(mdx, 2), acc=1)))

    def untouched():
        cx.sync()
        return all(bool((t == SENTINEL).all()) for t in (out, dqkv, mout, mdx))
    return thunks, untouched, (qkv, dout, table, out, dqkv, mx, mdm, mout, mdx)
