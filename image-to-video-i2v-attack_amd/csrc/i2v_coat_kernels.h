// Internal interface of the CoaT launches (i2v_coat.hip; without -DI2V_HAVE_COAT the same as scalar host code, i2v_coat_host.h) to
// their planner (i2v_coat.cpp).  The linear layers, the LayerNorm pair and the token assembly are the shared ones (i2v_vit_kernels.h).
#pragma once
#ifdef __HIP__
#include <hip/hip_runtime.h>
#else
#include "i2v_hip_stub.h"     // (no HIP: the host simulation's build)
#endif
#include <stdint.h>

enum { COAT_MAX_DH = 64, COAT_TT = 64, COAT_GW = 64 };      // widest head; tokens of a tile; columns a head group covers at most

// Factorized attention on qkv (F, T, 3 H dh): q of head h at column h dh, k at H dh + h dh, v at 2 H dh + h dh.  Per frame and head:
//   forward   Ks = softmax of k over the TOKENS, per column | G = Ks^T v (dh, dh) | out = scale q G + q o E, out and E (F, T, H dh)
//             saved: gram (F, H, dh, dh) = G, kstat (F, H, 2, dh) = the column maximum of k, then the log of the column sum of exp(k - max)
//   backward  from dout: dG = scale q^T dout (written to the scratch dgram) | c[a] = sum over b of G[a][b] dG[a][b] |
//             Ks = exp((k - max) - logsum) | dq = scale dout G^T + dout o E | dE = dout o q | dv = Ks dG | dk = Ks o (v dG^T - c)
// A head group is the run of max(1, 64 / dh) whole heads: the unit one workgroup of a reduce launch owns.
struct CoatAttn {
    const float *qkv, *E;
    int32_t F, T, H, dh;
    float scale;
    float *gram, *kstat;               // forward: written.  backward: read
    float* out;                        // forward
    const float* dout;                 // backward
    float *dgram, *dqkv, *dE;
};
int coat_attention(const CoatAttn& p, hipStream_t s);           // two launches: reduce, apply
int coat_attention_bwd(const CoatAttn& p, hipStream_t s);       // two launches: reduce, apply

// Token-major depthwise convolution whose window depends on the channel.  Frame f's row t of x is at x + (f (prefix + g^2) + t) xrs,
// of y at y + (f (prefix + g^2) + t) yrs; rows 0 .. prefix-1 of a frame are the prefix tokens, the rest the g x g plane.  Channels
// 0 .. n3-1 take w3 (9, n3), n3 .. n3+n5-1 take w5 (25, n5), the rest w7 (49, C-n3-n5): filters tap-major, "same" zero padding.
//   forward   y[c] = (residual: x[c] +) (b[c] + the taps (ky, kx) in increasing order, a tap on the padding taking no part); prefix
//             rows of y: x's (residual) or 0
//   backward  x is dy and y is dx: dx[c] = (residual: dy[c] +) the sum from 0 over (ky, kx) in increasing order of
//             w[ky][kx][c] dy[py + K/2 - ky][px + K/2 - kx][c] (gather form: one owner per element); prefix rows: dy's (residual) or 0;
//             written, or added to dx with `accumulate` (a prefix row of zeros is then not touched)
struct CoatDw {
    const float *x, *w3, *w5, *w7, *b; // a filter of a window with no channels may be null; b may be null
    float* y;
    int32_t F, g, C, n3, n5, prefix, residual, accumulate;
    int64_t xrs, yrs;                  // row strides in floats
};
int coat_dwmix(const CoatDw& p, hipStream_t s);
int coat_dwmix_bwd(const CoatDw& p, hipStream_t s);

// The s x s cells of a token-major plane behind `prefix` rows: stream (F, prefix + g^2, C) <-> rows (F (g / s)^2, s^2 C), column
// (dy s + dx) C + c of row (f, oy, ox) = channel c of plane position (oy s + dy, ox s + dx); s = 1 strips the prefix rows.  The scatter
// is the inverse (every plane element has one cell): written with the prefix rows 0, or added with `accumulate`, the prefix rows untouched.
struct CoatCells {
    const float* src;
    float* dst;
    int32_t F, g, C, s, prefix, accumulate;
};
int coat_cell_gather(const CoatCells& p, hipStream_t s);
int coat_cell_scatter(const CoatCells& p, hipStream_t s);

// What both forms of the launches refuse, with the text.  Returns the message or null.
inline const char* coat_attn_refusal(const CoatAttn& p, bool bwd) {
    if (!p.qkv || !p.E || !p.gram || !p.kstat || (!bwd && !p.out) || (bwd && (!p.dout || !p.dgram || !p.dqkv || !p.dE))) return "null argument";
    if (p.F <= 0 || p.T <= 0 || p.H <= 0 || p.dh <= 0) return "frames, tokens, heads and head width must be positive";
    if (p.dh % 4 != 0) return "the head width must be a multiple of 4";
    if (p.dh > COAT_MAX_DH) return "a head wider than 64";
    if (p.F > 65535 || p.H > 65535 || ((int64_t)p.T + COAT_TT - 1) / COAT_TT > 65535) return "a grid dimension over 65535 (frames, heads or token tiles)";
    if ((int64_t)p.F * p.T * 3 * p.H * p.dh >= (1ll << 31)) return "more than 2^31 elements";
    uintptr_t al = (uintptr_t)p.qkv | (uintptr_t)p.E | (uintptr_t)p.gram | (uintptr_t)p.kstat;
    al |= bwd ? (uintptr_t)p.dout | (uintptr_t)p.dgram | (uintptr_t)p.dqkv | (uintptr_t)p.dE : (uintptr_t)p.out;
    if (al & 15) return "16-byte alignment needed";
    return nullptr;
}

inline const char* coat_dw_refusal(const CoatDw& p) {
    if (p.F <= 0 || p.g <= 0 || p.C <= 0) return "frames, grid and channels must be positive";
    if (p.n3 < 0 || p.n5 < 0 || p.prefix < 0 || p.n3 + p.n5 > p.C) return "the window groups do not partition the channels";
    const int n7 = p.C - p.n3 - p.n5;
    if (p.n3 % 4 || p.n5 % 4 || n7 % 4) return "a group width must be a multiple of 4";
    if (!p.x || !p.y || (p.n3 && !p.w3) || (p.n5 && !p.w5) || (n7 && !p.w7)) return "null argument";
    if (p.xrs < p.C || p.yrs < p.C || p.xrs % 4 || p.yrs % 4) return "a row stride shorter than the channels or no multiple of 4";
    const int64_t rows = (int64_t)p.F * (p.prefix + (int64_t)p.g * p.g);
    if (p.F > 65535 || p.g > 65535) return "a grid dimension over 65535 (frames or plane side)";
    if (rows * p.xrs >= (1ll << 31) || rows * p.yrs >= (1ll << 31)) return "more than 2^31 elements";
    if (((uintptr_t)p.x | (uintptr_t)p.y | (uintptr_t)p.w3 | (uintptr_t)p.w5 | (uintptr_t)p.w7 | (uintptr_t)p.b) & 15) return "16-byte alignment needed";
    return nullptr;
}

inline const char* coat_cells_refusal(const CoatCells& p) {
    if (!p.src || !p.dst) return "null argument";
    if (p.F <= 0 || p.g <= 0 || p.C <= 0 || p.s <= 0 || p.prefix < 0) return "frames, grid, channels and cell side must be positive";
    if (p.g % p.s != 0) return "the cells do not tile the plane";
    if (p.C % 4 != 0) return "the channels must be a multiple of 4";
    if ((int64_t)p.F * (p.prefix + (int64_t)p.g * p.g) * p.C >= (1ll << 31)) return "more than 2^31 elements";
    if (((uintptr_t)p.src | (uintptr_t)p.dst) & 15) return "16-byte alignment needed";
    return nullptr;
}
