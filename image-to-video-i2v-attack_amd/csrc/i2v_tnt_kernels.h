// Internal interface of the TNT launches (i2v_tnt.hip; without -DI2V_HAVE_TNT the same as scalar host code, i2v_tnt_host.h) to their
// planner (i2v_tnt.cpp).  The linear layers, the LayerNorm pair and the token assembly are the shared ones (i2v_vit_kernels.h).
#pragma once
#ifdef __HIP__
#include <hip/hip_runtime.h>
#else
#include "i2v_hip_stub.h"     // (no HIP: the host simulation's build)
#endif
#include <stdint.h>

enum { TNT_MAX_T = 16, TNT_MAX_DH = 16, TNT_MAX_H = 8, TNT_THREADS = 256, TNT_LDS_BYTES = 65536 };

// Attention over many short sequences on qkv (S, T, 3 H dh): q of head h at column h dh, k at H dh + h dh, v at 2 H dh + h dh.
// Per sequence, head and query row i, every sum an fmaf chain from 0 in increasing index:
//   forward   s[j] = (q_i . k_j) scale | m = max s | e[j] = exp(s[j] - m) | l = e[0] + e[1] + ... | P[j] = e[j] / l |
//             out_i[d] = sum over j of P[j] v_j[d], out (S, T, H dh)
//   backward  from dout (S, T, H dh), P recomputed as above:  dP[j] = dout_i . v_j | delta = sum over j of P[j] dP[j] |
//             dS[j] = P[j] (dP[j] - delta) | the row owns dq_i[d] = (sum over j of dS[j] k_j[d]) scale; the key j owns
//             dk_j[d] = (sum over i of dS[i][j] q_i[d]) scale and dv_j[d] = sum over i of P[i][j] dout_i[d]; dqkv laid out as qkv.
// A workgroup owns tnt_group(T, H, dh) whole sequences; a sequence never leaves its workgroup and no sum crosses sequences.
struct TntAttn {
    const float* qkv;
    int64_t S;
    int32_t T, H, dh;
    float scale;
    float* out;                        // forward
    const float* dout;                 // backward
    float* dqkv;
};
int tnt_attention(const TntAttn& p, hipStream_t s);             // one launch
int tnt_attention_bwd(const TntAttn& p, hipStream_t s);         // one launch

// LDS floats a workgroup of n sequences stages in the backward (the larger of the two passes): qkv, dout, and (m, l, delta) per row
inline int64_t tnt_lds_floats(int n, int T, int H, int dh) { return (int64_t)n * T * (4 * H * dh + 3 * H); }

// Sequences per workgroup, forward and backward alike: one (sequence, head, row) per thread, as many whole sequences as 256 threads
// and 64 KB of LDS take
inline int tnt_group(int T, int H, int dh) {
    int n = TNT_THREADS / (H * T);
    while (n > 1 && tnt_lds_floats(n, T, H, dh) * 4 > TNT_LDS_BYTES) --n;
    return n < 1 ? 1 : n;
}

// The pixel embedding's rows: frame (F, Cin, side, side) <-> rows (F g^2 16, Kp), g = side / 16, Kp = Cin 49 rounded up to 4.
// Row ((f g + py) g + px) 16 + 4 i + j is the window of the 7 x 7, stride 4, padding 3 convolution at output (4 py + i, 4 px + j);
// column c 49 + ky 7 + kx = frame[f][c][4 oy + ky - 3][4 ox + kx - 3], 0 outside the frame and in the padding columns.
//   scatter   the transpose in gather form: pixel (f, c, y, x) sums rows[.][c 49 + ky 7 + kx] over the at most 2 x 2 outputs (oy, ox)
//             whose window holds it, from 0, oy then ox increasing; written, or added once to dx with `accumulate`
struct TntPixels {
    const float* src;
    float* dst;
    int32_t F, Cin, side, accumulate;
};
constexpr int tnt_pixel_cols(int Cin) { return (Cin * 49 + 3) / 4 * 4; }
int tnt_pixel_gather(const TntPixels& p, hipStream_t s);
int tnt_pixel_scatter(const TntPixels& p, hipStream_t s);

// x (rows, C) += table (period, C) at row r % period: the pixel position table (period 16); with period = rows, one array onto another
int tnt_row_add(float* x, const float* table, int64_t rows, int C, int64_t period, hipStream_t s);

// What both forms of the launches refuse, with the text.  Returns the message or null.
inline const char* tnt_attn_refusal(const TntAttn& p, bool bwd) {
    if (!p.qkv || (bwd ? (!p.dout || !p.dqkv) : !p.out)) return "null argument";
    if (p.S <= 0 || p.T <= 0 || p.H <= 0 || p.dh <= 0) return "sequences, tokens, heads and head width must be positive";
    if (p.T > TNT_MAX_T) return "more than 16 tokens: a thread holds one row of the score matrix in registers";
    if (p.dh > TNT_MAX_DH) return "a head wider than 16";
    if (p.H > TNT_MAX_H) return "more than 8 heads";
    if ((p.H * p.dh) % 4 != 0) return "heads x head width must be a multiple of 4";
    if (p.S * p.T * 3 * p.H * p.dh >= (1ll << 31)) return "more than 2^31 elements";
    const uintptr_t al = (uintptr_t)p.qkv | (uintptr_t)(bwd ? p.dout : p.out) | (uintptr_t)(bwd ? p.dqkv : p.out);
    if (al & 15) return "16-byte alignment needed";
    return nullptr;
}

inline const char* tnt_pixels_refusal(const TntPixels& p) {
    if (!p.src || !p.dst) return "null argument";
    if (p.F <= 0 || p.Cin <= 0 || p.side <= 0) return "frames, channels and frame side must be positive";
    if (p.side % 16 != 0) return "the frame side must be a multiple of 16";
    const int64_t rows = (int64_t)p.F * (p.side / 4) * (p.side / 4);
    if (rows * tnt_pixel_cols(p.Cin) >= (1ll << 31) || (int64_t)p.F * p.Cin * p.side * p.side >= (1ll << 31)) return "more than 2^31 elements";
    if (((uintptr_t)p.src | (uintptr_t)p.dst) & 15) return "16-byte alignment needed";
    return nullptr;
}

inline const char* tnt_row_add_refusal(const float* x, const float* table, int64_t rows, int C, int64_t period) {
    if (!x || !table) return "null argument";
    if (rows <= 0 || C <= 0 || period <= 0 || rows % period != 0) return "rows, width and period must be positive and the period must divide the rows";
    if (C % 4 != 0) return "the width must be a multiple of 4";
    if (rows * C >= (1ll << 31)) return "more than 2^31 elements";
    if (((uintptr_t)x | (uintptr_t)table) & 15) return "16-byte alignment needed";
    return nullptr;
}
