// Internal interface of the PiT launches (i2v_pit.hip; without -DI2V_HAVE_PIT the same as scalar host code, i2v_pit_host.h) to their
// planner (i2v_pit.cpp).  The linear layers, the LayerNorm pair and the token assembly are the shared ones (i2v_vit_kernels.h).
#pragma once
#ifdef __HIP__
#include <hip/hip_runtime.h>
#else
#include "i2v_hip_stub.h"     // (no HIP: the host simulation's build)
#endif
#include <stdint.h>

enum { PIT_MAX_DH = 64, PIT_QT = 64, PIT_KT = 64 };      // widest head; queries a workgroup owns; keys staged in LDS at a time

// Streaming attention on qkv (F, T, 3 H dh): q of head h at column h dh, k at H dh + h dh, v at 2 H dh + h dh.  T is unbounded: K and V
// pass through LDS in tiles of PIT_KT keys under an online softmax.  Per frame and head:
//   forward   S = scale q k^T | P = softmax over the keys | out = P v, out (F, T, H dh); lse = rowmax + log(denominator), (F, H, T)
//   backward  from dout (F, T, H dh), out and lse:  delta = rowsum(dout o out), (F, H, T), a scratch the first launch fills |
//             P = exp(S - lse) | dP = dout v^T | dS = scale P (dP - delta) | dq = dS k | dk = dS^T q | dv = P^T dout, into dqkv as qkv
struct PitAttn {
    const float* qkv;
    int32_t F, T, H, dh;
    float scale;
    float *out, *lse;                  // forward: written.  backward: read
    const float* dout;                 // backward
    float *delta, *dqkv;
};
int pit_attention(const PitAttn& p, hipStream_t s);             // one launch
int pit_attention_bwd(const PitAttn& p, hipStream_t s);         // three: delta, dq by query tile, dk / dv by key tile

// The pooling convolution of `transformers.{s}.pool.conv`: Conv2d(C, 2 C, kernel 3, stride 2, padding 1, groups = C) on token-major rows.
// Frame f's grid row (iy, ix) of x is at x + f xs + (iy g + ix) C  (xs: the frame stride in floats, the pointer already moved past the
// prefix rows), of y at y + f ys + (oy go + ox) 2 C, go = (g - 1) / 2 + 1.  Output channel o reads input channel o / 2.
//   forward   y[o] = bias[o] + sum over the taps (ky, kx) in increasing order of w[o][3 ky + kx] x[2 oy - 1 + ky][2 ox - 1 + kx][o / 2]
//   backward  dx[c] = sum over ky, kx, then o = 2 c, 2 c + 1, of w[o][3 ky + kx] dy[(iy + 1 - ky) / 2][(ix + 1 - kx) / 2][o]
//             (gather form: one owner per input element; taps whose output row or column is odd, or outside, take no part)
struct PitPool {
    const float *x, *w, *b;            // backward: x is dy, b unused
    float* y;                          // backward: dx
    int32_t F, g, C;                   // g and C of the INPUT side in both directions
    int32_t accumulate;                // backward: dx = dx + that sum (the sum formed first)
    int64_t xs, ys;                    // frame strides of the input-side and the output-side stream, in floats
};
int pit_pool(const PitPool& p, hipStream_t s);
int pit_pool_bwd(const PitPool& p, hipStream_t s);

// Overlapping patches: image (F, Cin, side, side) <-> rows (F g^2, Cin p^2), g = (side - p) / s + 1, column (c p + dy) p + dx of row
// (f, py, px) = pixel (py s + dy, px s + dx) of channel c.  The scatter is the transpose in gather form: a pixel sums its patches in
// increasing (py, px) order from 0; accumulate adds that sum to gx.
struct PitPatch {
    const float* src;
    float* dst;
    int32_t F, Cin, side, p, s, accumulate;
};
int pit_patch_gather(const PitPatch& p, hipStream_t s);
int pit_patch_scatter(const PitPatch& p, hipStream_t s);

// What both forms of the launches refuse, with the text.  Returns the message or null.
inline const char* pit_attn_refusal(const PitAttn& p, bool bwd) {
    if (!p.qkv || !p.out || !p.lse || (bwd && (!p.dout || !p.delta || !p.dqkv))) return "null argument";
    if (p.F <= 0 || p.T <= 0 || p.H <= 0 || p.dh <= 0) return "frames, tokens, heads and head width must be positive";
    if (p.dh % 4 != 0) return "the head width must be a multiple of 4";
    if (p.dh > PIT_MAX_DH) return "a head wider than 64";
    if (p.F > 65535 || p.H > 65535 || ((int64_t)p.T + PIT_QT - 1) / PIT_QT > 65535) return "a grid dimension over 65535 (frames, heads or token tiles)";
    if ((int64_t)p.F * p.T * 3 * p.H * p.dh >= (1ll << 31)) return "more than 2^31 elements";
    uintptr_t al = (uintptr_t)p.qkv | (uintptr_t)p.out | (uintptr_t)p.lse;
    if (bwd) al |= (uintptr_t)p.dout | (uintptr_t)p.delta | (uintptr_t)p.dqkv;
    if (al & 15) return "16-byte alignment needed";
    return nullptr;
}

inline const char* pit_pool_refusal(const PitPool& p) {
    if (!p.x || !p.w || !p.y) return "null argument";
    if (p.F <= 0 || p.g <= 0 || p.C <= 0) return "frames, grid and channels must be positive";
    const int64_t go = (p.g - 1) / 2 + 1;
    if (p.xs < (int64_t)p.g * p.g * p.C || p.ys < go * go * 2 * p.C) return "a frame stride shorter than the frame's grid rows";
    if ((p.F - 1) * p.xs + (int64_t)p.g * p.g * p.C >= (1ll << 31) || (p.F - 1) * p.ys + go * go * 2 * p.C >= (1ll << 31)) return "more than 2^31 elements";
    if (((uintptr_t)p.x | (uintptr_t)p.w | (uintptr_t)p.b | (uintptr_t)p.y) & 3) return "4-byte alignment needed";
    return nullptr;
}

inline const char* pit_patch_refusal(const PitPatch& p) {
    if (!p.src || !p.dst) return "null argument";
    if (p.F <= 0 || p.Cin <= 0 || p.side <= 0 || p.p <= 0 || p.s <= 0) return "frames, channels, side, patch and stride must be positive";
    if (p.p > p.side || (p.side - p.p) % p.s != 0) return "the patches at this stride do not tile the frame";
    if (p.s > p.p) return "a stride over the patch side leaves pixels uncovered";
    const int64_t g = (p.side - p.p) / p.s + 1;
    if ((int64_t)p.F * g * g * p.Cin * p.p * p.p >= (1ll << 31) || (int64_t)p.F * p.Cin * p.side * p.side >= (1ll << 31)) return "more than 2^31 elements";
    if (((uintptr_t)p.src | (uintptr_t)p.dst) & 3) return "4-byte alignment needed";
    return nullptr;
}
