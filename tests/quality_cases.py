"""What the tests of the quality launches and the 8-bit export share (include/i2v_quality.h): the case table, the
float64 reference, the wrong references, the run of a case through the C entries between padding, and the bounds.

REFERENCE.  `ssim_ref` is Wang et al.'s SSIM as the header states it, separable, in the dtype it is given (float64: the reference;
float32: the run whose error against float64 is recorded in tests/golden/quality_fp32_cpu_errors.json by tests/make_quality_fixtures.py).
`ssim_direct` is the same definition as a direct 121-tap double loop in Python floats; the tests pin `ssim_ref` on the smallest planes
with it.  SSE and max are plain float64 sums of the level differences.

BOUNDS (the project's convention, tests/conv_aux_cases.py): against float64 the SSIM of a frame within max(2e-6, 4 x e32) absolute,
the f32 mode's SSE within max(2e-6, 4 x e32) relative, where e32 is the recorded error of the float32 CPU run on the same case; the u8
mode's SSE and max exact; the f32 mode's max within one fp32 ulp of 255.  A case without a recorded error fails (KeyError).

PADDING.  `run_case` lays both operands into larger allocations: float operands between NaN, byte operands between 0xA5 bytes, `out` and
`scratch` between SENTINEL doubles that must come back bit for bit.  `offset` moves an operand off its natural alignment: one byte (u8),
one element (f32, off the 16 bytes a vector load would want).

SHAPES.  The tile is TR x TC valid positions (asserted against `Engine.clip_quality_tile()`); a frame of h x w has (h - 10) x (w - 10).
One window; one extra row / column; a long row; widths 13, 14, 15 (3 w mod 4 = 3, 2, 1: every skew of a byte row); one fewer, equal and
one more than a tile's positions in each direction; two tiles plus one in both; 224 x 224; frames 1, 2, 5; two clips of 1 and 3 frames;
70 000 frames of 11 x 11 in one call (past a 65 535 grid, and past the launch's own 65 536 workgroups: the item loop runs)."""
import ctypes as C
import json
import os
from collections import namedtuple

import numpy as np
import torch

from i2v_amd import lib as _lib

TR, TC = 16, 32
SENTINEL = -123.25
PAD_BYTE = 0xA5
FRONT = 64                      # elements of padding ahead of an operand (a multiple of 16 bytes in every dtype)
FLOOR = 2e-6
ULP_255 = float(np.spacing(np.float32(255.0)))
MEAN = [float(np.float32(v)) for v in (0.485, 0.456, 0.406)]
STD = [float(np.float32(v)) for v in (0.229, 0.224, 0.225)]
C1, C2 = (0.01 * 255) ** 2, (0.03 * 255) ** 2
FP32_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "quality_fp32_cpu_errors.json")

Case = namedtuple("Case", "name mode clips t h w content offset reps")


def _c(mode, h, w, content="noise", clips=1, t=1, offset=0, reps=1):
    name = f"{mode}-{clips}x{t}x{h}x{w}-{content}" + (f"-off{offset}" if offset else "") + (f"-x{reps}" if reps > 1 else "")
    return Case(name, mode, clips, t, h, w, content, offset, reps)


def _cases():
    out = []
    shapes = [(11, 11), (11, 12), (12, 11), (11, 75), (27, 13), (12, 14), (12, 15)]
    shapes += [(TR + 10 + d, 13) for d in (-1, 0, 1)] + [(12, TC + 10 + d) for d in (-1, 0, 1)] + [(2 * TR + 11, 2 * TC + 11)]
    for mode in ("u8", "f32"):
        out += [_c(mode, h, w) for h, w in shapes]
        out.append(_c(mode, 224, 224))
        for content in ("noise", "same", "const-2-12", "const-100-110", "const-0-255", "checker", "flat250"):
            out.append(_c(mode, TR + 11, TC + 15, content))
        out.append(_c(mode, 27, 13, offset=1))
        out.append(_c(mode, TR + 11, TC + 15, offset=1))
    out += [_c("u8", 27, 45, clips=2), _c("u8", 27, 45, clips=5), _c("f32", 27, 45, clips=2, t=1), _c("f32", 27, 45, clips=2, t=3)]
    out.append(_c("u8", 11, 11, clips=7, reps=10000))               # 70 000 frames, about 25 MB: 7 distinct frames, repeated
    return list({c.name: c for c in out}.values())                   # (27 x 13 is also one more than a tile's rows)


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}
SMALLEST = [c for c in CASES if c.h * c.w <= 132 and c.content == "noise" and c.reps == 1]      # pinned by the direct loop


def frames_of(case):
    """The case's two operands as uint8 frames (n, h, w, 3), n = clips * t (before `reps`): seeded, the second within +-16 of the first."""
    n, h, w = case.clips * case.t, case.h, case.w
    gen = torch.Generator().manual_seed(1000 + 7 * h + w + n)
    kind = case.content
    if kind in ("noise", "same"):
        a = torch.randint(0, 256, (n, h, w, 3), generator=gen, dtype=torch.int32)
        b = a if kind == "same" else (a + torch.randint(-16, 17, a.shape, generator=gen, dtype=torch.int32)).clamp(0, 255)
    elif kind.startswith("const"):
        va, vb = (int(v) for v in kind.split("-")[1:])
        a, b = torch.full((n, h, w, 3), va, dtype=torch.int32), torch.full((n, h, w, 3), vb, dtype=torch.int32)
    elif kind == "checker":
        yy, xx = torch.meshgrid(torch.arange(h), torch.arange(w), indexing="ij")
        a = (((yy + xx) % 2) * 255).to(torch.int32).view(1, h, w, 1).expand(n, h, w, 3)
        b = 255 - a
    elif kind == "flat250":         # the cancellation case: means of 250 against variances below 1
        a = 250 + torch.randint(-1, 2, (n, h, w, 3), generator=gen, dtype=torch.int32)
        b = 250 + torch.randint(-1, 2, (n, h, w, 3), generator=gen, dtype=torch.int32)
    else:
        raise KeyError(kind)
    return a.to(torch.uint8).contiguous(), b.to(torch.uint8).contiguous()


def normalise(u8):
    """frames (b, t, h, w, 3) uint8 -> the clip (b, 3, t, h, w) float32 as `i2v_clip_from_u8_f32` forms it: two correctly rounded fp32
    divisions and one subtraction."""
    x = u8.permute(0, 4, 1, 2, 3).to(torch.float32) / 255.0
    mean = torch.tensor(MEAN, dtype=torch.float32).view(1, 3, 1, 1, 1)
    std = torch.tensor(STD, dtype=torch.float32).view(1, 3, 1, 1, 1)
    return ((x - mean) / std).contiguous()


def operands(case):
    """(a, b) as the entry takes them, before `reps`: uint8 (n, h, w, 3), or float32 (clips, 3, t, h, w) -- the normalised frames, the
    second operand moved off the 8-bit grid by a seeded fraction of a level so that nothing of the f32 mode rests on round numbers."""
    a, b = frames_of(case)
    if case.mode == "u8":
        return a, b
    shape = (case.clips, case.t, case.h, case.w, 3)
    xa, xb = normalise(a.view(shape)), normalise(b.view(shape))
    if case.content in ("noise", "flat250"):
        gen = torch.Generator().manual_seed(77 + case.h + case.w)
        std = torch.tensor(STD, dtype=torch.float32).view(1, 3, 1, 1, 1)
        xb = (xb + (torch.rand(xb.shape, generator=gen) - 0.5) / (255.0 * std)).contiguous()
    return xa, xb


def levels(case, x, dtype=torch.float64):
    """An operand as levels (n, 3, h, w) in `dtype`: the bytes, or 255 (x std + mean) of the fp32 clip."""
    if case.mode == "u8":
        return x.permute(0, 3, 1, 2).to(dtype)
    mean = torch.tensor(MEAN, dtype=dtype).view(1, 3, 1, 1, 1)
    std = torch.tensor(STD, dtype=dtype).view(1, 3, 1, 1, 1)
    lv = 255.0 * (x.to(dtype) * std + mean)
    return lv.permute(0, 2, 1, 3, 4).reshape(-1, 3, case.h, case.w)


# ---- the reference --------------------------------------------------------------------------------------------------------------------
def taps(sigma=1.5, dtype=torch.float64, box=False):
    k = torch.arange(11, dtype=torch.float64) - 5.0
    g = torch.ones(11, dtype=torch.float64) if box else torch.exp(-k * k / (2.0 * sigma * sigma))
    return (g / g.sum()).to(dtype)


def _filter(x, g, same=False):
    if same:
        x = torch.nn.functional.pad(x, (5, 5, 5, 5))
    oh, ow = x.shape[-2] - 10, x.shape[-1] - 10
    rows = sum(g[k] * x[..., :, k:k + ow] for k in range(11))
    return sum(g[k] * rows[..., k:k + oh, :] for k in range(11))


def ssim_ref(la, lb, dtype=torch.float64, sigma=1.5, box=False, same=False, k2=0.03, data_range=255.0, gray=False):
    """Mean SSIM per frame of levels (n, 3, h, w), in `dtype`; the keywords are the wrong references.  The moments are taken of
    level - 127.5, as the definition has it: in float64 that changes nothing, in float32 it is the run whose error is recorded."""
    la, lb = la.to(dtype), lb.to(dtype)
    if gray:
        la, lb = la.mean(1, keepdim=True), lb.mean(1, keepdim=True)
    g = taps(sigma, dtype, box)
    c1, c2 = (0.01 * data_range) ** 2, (k2 * data_range) ** 2
    va, vb = la - 127.5, lb - 127.5
    ma, mb = _filter(va, g, same), _filter(vb, g, same)
    saa, sbb, sab = _filter(va * va, g, same) - ma * ma, _filter(vb * vb, g, same) - mb * mb, _filter(va * vb, g, same) - ma * mb
    Ma, Mb = ma + 127.5, mb + 127.5
    s = ((2 * (Ma * Mb) + c1) * (2 * sab + c2)) / (((Ma * Ma + Mb * Mb) + c1) * ((saa + sbb) + c2))
    return s.mean(dim=(1, 2, 3)).to(torch.float64)


def ssim_direct(la, lb):
    """The definition as a direct 121-tap double loop over every valid position, uncentred, in Python floats: (n,) values."""
    g = [float(v) for v in taps()]
    n, _, h, w = la.shape
    A, B = la.tolist(), lb.tolist()
    out = []
    for f in range(n):
        total = 0.0
        for c in range(3):
            for y in range(h - 10):
                for x in range(w - 10):
                    ma = mb = maa = mbb = mab = 0.0
                    for i in range(11):
                        for j in range(11):
                            wgt, a, b = g[i] * g[j], A[f][c][y + i][x + j], B[f][c][y + i][x + j]
                            ma += wgt * a; mb += wgt * b; maa += wgt * a * a; mbb += wgt * b * b; mab += wgt * a * b
                    saa, sbb, sab = maa - ma * ma, mbb - mb * mb, mab - ma * mb
                    total += (2 * ma * mb + C1) * (2 * sab + C2) / ((ma * ma + mb * mb + C1) * (saa + sbb + C2))
        out.append(total / (3 * (h - 10) * (w - 10)))
    return torch.tensor(out, dtype=torch.float64)


def reference(case, a, b, dtype=torch.float64, **wrong):
    """(n, 3) float64 rows of (SSE, max, SSIM) of the case's operands (before `reps`), computed in `dtype`."""
    la, lb = levels(case, a, dtype), levels(case, b, dtype)
    d = la - lb
    sse = (d * d).sum(dim=(1, 2, 3)).to(torch.float64)
    mx = d.abs().amax(dim=(1, 2, 3)).to(torch.float64)
    return torch.stack((sse, mx, ssim_ref(la, lb, dtype, **wrong)), dim=1)


WRONG = {   # name -> (the reference's keywords, contents whose SSIM it must miss, contents it cannot change)
    "same-padding": (dict(same=True), ("noise", "const-2-12", "const-100-110", "checker"), ("same",)),
    "box-window": (dict(box=True), ("noise", "flat250"), ("same", "const-2-12", "const-100-110", "const-0-255")),
    "sigma-1.0": (dict(sigma=1.0), ("noise", "flat250"), ("same", "const-2-12", "const-100-110", "const-0-255")),
    "K2-0.02": (dict(k2=0.02), ("noise", "flat250"), ("same", "const-2-12", "const-100-110", "const-0-255")),
    "channels-averaged": (dict(gray=True), ("noise", "flat250"), ("same", "const-2-12", "const-100-110", "const-0-255", "checker")),
    "data-range-1": (dict(data_range=1.0), ("noise", "flat250", "const-2-12"), ("same",)),
}


# ---- the bounds -----------------------------------------------------------------------------------------------------------------------
def fp32_errors():
    return json.load(open(FP32_PATH))


def bound(e32):
    return max(FLOOR, 4.0 * e32)


def check(case, got, want, fp32):
    """`got` (n, 3) against the float64 `want`, at the bounds of this module; every figure is printed before it is held."""
    e = fp32[case.name]                                             # a case without a recorded error fails here
    ssim_err = float((got[:, 2] - want[:, 2]).abs().max())
    sse_rel = float(((got[:, 0] - want[:, 0]).abs() / want[:, 0].clamp_min(1e-300)).max()) if float(want[:, 0].max()) > 0 else float(got[:, 0].abs().max())
    max_err = float((got[:, 1] - want[:, 1]).abs().max())
    print(f"{case.name}: ssim err {ssim_err:.3e} (fp32 CPU {e['ssim']:.3e}) sse rel {sse_rel:.3e} (fp32 CPU {e['sse']:.3e}) max err {max_err:.3e}")
    assert ssim_err <= bound(e["ssim"]), (case.name, ssim_err, e["ssim"])
    if case.mode == "u8":
        assert torch.equal(got[:, :2], want[:, :2]), case.name
    else:
        assert sse_rel <= bound(e["sse"]), (case.name, sse_rel, e["sse"])
        assert max_err <= ULP_255, (case.name, max_err)


# ---- a case through the C entries, between padding ------------------------------------------------------------------------------------
def _padded(t, offset, fill, to_dev):
    """`t` laid at element FRONT + offset of a larger flat allocation filled with `fill`: (the allocation, the view's pointer)."""
    flat = torch.full((FRONT + offset + t.numel() + FRONT,), fill, dtype=t.dtype)
    flat[FRONT + offset:FRONT + offset + t.numel()] = t.reshape(-1)
    dev = to_dev(flat)
    return dev, C.c_void_p(dev.data_ptr() + (FRONT + offset) * t.element_size())


def run_case(eng, case, a, b, to_dev=lambda t: t, sync=lambda: None, scratch_bytes=None):
    """The case's operands through `i2v_clip_quality_u8` / `_f32` of `eng`, everything between padding: (n * reps, 3) float64 on the
    host.  Holds the padding of `out` and `scratch` to its bits afterwards."""
    capi = _lib.bind(eng.capi, _lib._QUALITY_PROTOS)
    if case.reps > 1:
        a, b = a.repeat(case.reps, 1, 1, 1), b.repeat(case.reps, 1, 1, 1)
    n = case.clips * case.t * case.reps
    fill = PAD_BYTE if case.mode == "u8" else float("nan")
    abuf, pa = _padded(a, case.offset, fill, to_dev)
    bbuf, pb = _padded(b, case.offset, fill, to_dev)
    need = int(capi.i2v_clip_quality_scratch_bytes(n, case.h, case.w))
    assert need == n * (-(-(case.h - 10) // TR)) * (-(-(case.w - 10) // TC)) * 24
    out = to_dev(torch.full((FRONT + 3 * n + FRONT,), SENTINEL, dtype=torch.float64))
    scratch = to_dev(torch.full((FRONT + need // 8 + FRONT,), SENTINEL, dtype=torch.float64))
    po, ps = C.c_void_p(out.data_ptr() + 8 * FRONT), C.c_void_p(scratch.data_ptr() + 8 * FRONT)
    nb = need if scratch_bytes is None else scratch_bytes
    if case.mode == "u8":
        rc = capi.i2v_clip_quality_u8(pa, pb, po, n, case.h, case.w, ps, nb, eng.stream())
    else:
        rc = capi.i2v_clip_quality_f32(pa, pb, po, case.clips, case.t, case.h, case.w, ps, nb, eng.stream())
    _lib.check(capi, rc)
    sync()
    out, scratch = out.cpu(), scratch.cpu()
    for buf, k in ((out, 3 * n), (scratch, need // 8)):
        assert torch.equal(buf[:FRONT], torch.full((FRONT,), SENTINEL, dtype=torch.float64)), case.name
        assert torch.equal(buf[FRONT + k:], torch.full((FRONT,), SENTINEL, dtype=torch.float64)), case.name
    del abuf, bbuf
    return out[FRONT:FRONT + 3 * n].view(n, 3).clone()


def run_export(eng, video, ref=None, levels=-1, offset=0, to_dev=lambda t: t, sync=lambda: None):
    """`i2v_clip_to_u8` of `eng` on video (b, 3, t, h, w) between padding, the frames written `offset` bytes off their natural
    alignment between 0xA5 bytes that must come back: (b, t, h, w, 3) uint8 on the host."""
    capi = _lib.bind(eng.capi, _lib._QUALITY_PROTOS)
    b, _, t, h, w = video.shape
    n = b * t * h * w * 3
    vbuf, pv = _padded(video, 0, float("nan"), to_dev)
    rbuf, pr = _padded(ref, offset, PAD_BYTE, to_dev) if ref is not None else (None, None)
    out = to_dev(torch.full((FRONT + offset + n + FRONT,), PAD_BYTE, dtype=torch.uint8))
    _lib.check(capi, capi.i2v_clip_to_u8(pv, pr, levels, C.c_void_p(out.data_ptr() + FRONT + offset), b, t, h, w, eng.stream()))
    sync()
    out = out.cpu()
    assert bool((out[:FRONT + offset] == PAD_BYTE).all()) and bool((out[FRONT + offset + n:] == PAD_BYTE).all())
    del vbuf, rbuf
    return out[FRONT + offset:FRONT + offset + n].view(b, t, h, w, 3).clone()
