// Internal interface of the 8-bit export and the quality launches (i2v_quality.hip; without -DI2V_HAVE_QUALITY the same as scalar host
// code, i2v_quality_host.h) to their C entries (i2v_quality.cpp).  This header IS the definition of the arithmetic: the constants, the
// tile, the owner of every pixel and the order of every sum.  Device and host twin are held to each other bit for bit.
#pragma once
#ifdef __HIP__
#include <hip/hip_runtime.h>
#else
#include "i2v_hip_stub.h"     // (no HIP: the host simulation's build)
#endif
#include <stddef.h>
#include <stdint.h>

// A tile is QL_TR x QL_TC positions of the VALID SSIM map of one frame, all three channels; it stages (QL_TR + 10) x (QL_TC + 10)
// pixels.  One workgroup of QL_THREADS threads works a tile off; a workgroup loops over (frame, tile) items.
enum { QL_TAPS = 11, QL_HALO = QL_TAPS - 1, QL_TR = 16, QL_TC = 32, QL_IR = QL_TR + QL_HALO, QL_IC = QL_TC + QL_HALO, QL_THREADS = 256,
       QL_YB = 2,                      // consecutive valid rows one thread finishes in the vertical pass
       QL_FIN_THREADS = 64, QL_MAX_GRID = 65536 };

// exp(-(k - 5)^2 / (2 * 1.5^2)) / their sum, in float64, rounded to fp32
#define QL_TAP_LITERALS 0.00102838012f, 0.00759875821f, 0.0360007733f, 0.109360687f, 0.213005543f, 0.266011715f, 0.213005543f, 0.109360687f, \
                        0.0360007733f, 0.00759875821f, 0.00102838012f
#define QL_C1 6.5025                   // (0.01 * 255)^2
#define QL_C2 58.5225                  // (0.03 * 255)^2
#define QL_CENTRE 127.5f
#define QL_MEAN_LITERALS 0.485f, 0.456f, 0.406f      // the loader's constants (i2v_kernels.hip)
#define QL_STD_LITERALS 0.229f, 0.224f, 0.225f

// ---- the definition -------------------------------------------------------------------------------------------------------------------
// Level of an element: u8 mode the byte; f32 mode 255.f * fmaf(x, std[c], mean[c]), neither rounded nor clamped.  v = level - 127.5f.
// Difference of a pixel: u8 mode the integer a - b; f32 mode, in double, d = (255.0 * (double)std[c]) * ((double)xa - (double)xb).
//
// Tile (ty, tx) of a frame, oh = h - 10, ow = w - 10 valid rows / columns, nty = ceil(oh / 16), ntx = ceil(ow / 32): stages the pixels
// (16 ty + r, 32 tx + q), r < 26, q < 42, as fp32 v; a pixel outside the frame is staged as 0 and reaches no valid position.  The tile
// OWNS the staged pixels inside the frame with (r < 16 or ty = nty - 1) and (q < 32 or tx = ntx - 1): every pixel has one owner.
// The window sums and the formula are DOUBLE arithmetic on the fp32 v and the fp32 taps (fp32 sums of x^2 - mu^2 lose the variance of a
// bright flat region to rounding; a double costs this launch little):
//   per channel c = 0, 1, 2:
//     horizontal  H_m[r][x] for r < 26, x < 32, m in (a, b, aa, bb, ab): the fma chain from 0 over k = 0 .. 10 of
//                 (double)tap[k] * s_m[r][x + k], s_a = (double)va, s_b = (double)vb, s_aa = s_a s_a, s_bb = s_b s_b, s_ab = s_a s_b
//                 (exact in double)
//     vertical    M_m[y][x] for y < 16, x < 32: the fma chain from 0 over k = 0 .. 10 of (double)tap[k] * H_m[y + k][x]
//     formula     ssim_value() below on the five M; a position with 16 ty + y >= oh or 32 tx + x >= ow counts as nothing
// Thread t of the 256 takes, for the SSIM sum, the positions x = t % 32, y = 2 (t / 32) + j, j = 0, 1, of channel 0, then 1, then 2,
// and adds each valid value to its sum in that order.  For SSE and max it takes the owned (pixel, channel) elements
//   u8 mode   e = t, t + 256, ... < 26 * 42 * 3, e = (r * 42 + q) * 3 + c: the integer square added to a 32-bit sum, the integer max;
//   f32 mode  channel 0, then 1, then 2, within a channel e = t, t + 256, ... < 26 * 42, e = r * 42 + q: d * d, rounded, added to a
//             double sum in that order, |d| to a double max.
// The 256 thread values (doubles: sum, max, sum) are then folded in place for s = 128, 64, .. 1: p[t] = p[t] + p[t + s] (max: the
// larger) for t < s; p[0] is the tile's partial, written as three doubles to scratch[(frame * nty * ntx + ty * ntx + tx) * 3].
// Second launch, per frame, 64 threads: thread t folds the partials of the tiles t, t + 64, ... in that order from 0, the 64 values are
// folded as above for s = 32 .. 1; out[frame] = (SSE, max, SSIM sum / (double)(3 * oh * ow)).
// Nothing depends on the number of frames in the call nor on which workgroup works which item off.
#ifdef __HIP__
#define QL_HD __host__ __device__
#else
#define QL_HD
#endif
QL_HD inline double ssim_value(double ma, double mb, double maa, double mbb, double mab) {
    // ma, mb: the means of v (centred); the variances do not move with the centre, the means get it back
    const double Ma = ma + (double)QL_CENTRE, Mb = mb + (double)QL_CENTRE;
    const double pa = ma * ma, pb = mb * mb, pab = ma * mb;
    const double saa = maa - pa, sbb = mbb - pb, sab = mab - pab;
    const double Pab = Ma * Mb, Paa = Ma * Ma, Pbb = Mb * Mb;
    const double t1 = 2.0 * Pab + QL_C1, t3 = (Paa + Pbb) + QL_C1;       // identical operands: Pab = Paa = Pbb, 2 p = p + p exactly
    const double t2 = 2.0 * sab + QL_C2, t4 = (saa + sbb) + QL_C2;
    const double num = t1 * t2, den = t3 * t4;
    return num / den;                                                     // correctly rounded: x / x = 1
}

struct QlClips {                      // one call of either mode
    const void *a, *b;
    double* out;
    double* scratch;
    int64_t frames;                   // f32 mode: clips * t
    int32_t t, h, w, u8;              // t: frames per clip (f32 mode: the channel planes of a clip are t h w apart; u8 mode: unused)
};
inline int64_t ql_tiles(int h, int w) { return (int64_t)((h - QL_HALO + QL_TR - 1) / QL_TR) * ((w - QL_HALO + QL_TC - 1) / QL_TC); }
inline size_t ql_scratch_bytes(int64_t frames, int h, int w) { return (size_t)(frames * ql_tiles(h, w)) * 3 * sizeof(double); }
int ql_clip_quality(const QlClips& p, hipStream_t s);           // two launches

// normalised clip (b, 3, t, h, w) -> frames (b, t, h, w, 3): q = rintf(255.f * min(max(fmaf(x, std[c], mean[c]), 0), 1)), round half to
// even, a NaN as 0; with ref: then min(max(q, max(ref - levels, 0)), min(ref + levels, 255))
struct QlExport {
    const float* video;
    const uint8_t* ref;
    uint8_t* frames;
    int32_t levels, b, t, h, w;
};
int ql_clip_to_u8(const QlExport& p, hipStream_t s);            // one launch

// What both forms refuse, with the text.  Returns the message or null.
inline const char* ql_quality_refusal(const QlClips& p, size_t scratch_bytes) {
    if (!p.a || !p.b || !p.out || !p.scratch) return "null argument";
    if (p.frames <= 0 || p.t <= 0) return "clips and frames must be positive";
    if (p.h < QL_TAPS || p.w < QL_TAPS) return "a frame smaller than the 11 x 11 window";
    if ((int64_t)p.h * p.w * 3 >= (1ll << 31)) return "more than 2^31 elements in a frame";
    if (p.frames * ql_tiles(p.h, p.w) >= (1ll << 40)) return "more than 2^40 tiles";
    if (scratch_bytes < ql_scratch_bytes(p.frames, p.h, p.w)) return "scratch smaller than i2v_clip_quality_scratch_bytes";
    if (((uintptr_t)p.out | (uintptr_t)p.scratch) & 7) return "out and scratch must be 8-byte aligned";
    if (!p.u8 && (((uintptr_t)p.a | (uintptr_t)p.b) & 3)) return "4-byte alignment needed";
    return nullptr;
}

inline const char* ql_export_refusal(const QlExport& p) {
    if (!p.video || !p.frames) return "null argument";
    if (p.b <= 0 || p.t <= 0 || p.h <= 0 || p.w <= 0) return "clips, frames, height and width must be positive";
    if (p.ref && p.levels < 0) return "a negative budget in levels";
    if ((uintptr_t)p.video & 3) return "4-byte alignment needed";
    return nullptr;
}
