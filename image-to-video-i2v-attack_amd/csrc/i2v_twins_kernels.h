// Internal interface of the Twins launches (i2v_twins.hip; without -DI2V_HAVE_TWINS the same as scalar host code, i2v_twins_host.h) to
// their planner (i2v_twins.cpp).  The linear layers, the LayerNorm pair, patchify and the 2 x 2 merge pair are the shared ones
// (i2v_vit_kernels.h, i2v_swin_kernels.h); the depthwise 3 x 3 of the position encoding is XCiT's (i2v_xcit_kernels.h).
#pragma once
#ifdef __HIP__
#include <hip/hip_runtime.h>
#else
#include "i2v_hip_stub.h"     // (no HIP: the host simulation's build)
#endif
#include <stdint.h>

enum { TWINS_MAX_TK = 64, TWINS_MAX_DH = 64 };      // one head's whole K and V live in one workgroup's LDS

// Sub-sampled (rectangular) attention: q (F, Tq, H dh), kv (F, Tk, 2 H dh) with k of head h at column h dh and v at H dh + h dh.
// Per frame and head:
//   forward   S = scale q k^T (Tq, Tk) | P = softmax over the keys | out = P v, out (F, Tq, H dh)
//   backward  from dout (F, Tq, H dh), P recomputed:  dP = dout v^T | dS = scale P (dP - rowsum(dP P)) | dq = dS k (F, Tq, H dh) |
//             dk = dS^T q, dv = P^T dout into dkv (F, Tk, 2 H dh)
struct TwinsAttn {
    const float *q, *kv;
    int32_t F, Tq, Tk, H, dh;
    float scale;
    float* out;                        // forward
    const float* dout;                 // backward
    float *dq, *dkv;
};
int twins_attention(const TwinsAttn& p, hipStream_t s);           // one launch
int twins_attention_bwd(const TwinsAttn& p, hipStream_t s);       // two launches: dq by query tile, then dk / dv by (frame, head)

// The s x s block gather of a token-major plane and its adjoint, s in {2, 4, 8}; H and W multiples of s, C a multiple of 4.
//   gather   rows (F H/s W/s, s s C): rows[(f, oy, ox)][(dy s + dx) C + c] = x(f, s oy + dy, s ox + dx, c)
//   scatter  the inverse permutation: dx(f, y, x, c) (+)= drows[...]; `accumulate` adds to what dx holds
int twins_block_gather(const float* x, float* rows, int F, int H, int W, int C, int sr, hipStream_t s);
int twins_block_scatter(const float* drows, float* dx, int F, int H, int W, int C, int sr, int accumulate, hipStream_t s);

// Window attention without shift and without a bias table on qkv (F, H W, 3 heads dh): Twins-SVT's locally-grouped attention.  On the
// device this is swin_window_attention(_bwd) at shift 0 with `zero_table` ((2 ws - 1)^2 heads zeros, which that launch requires); the
// host form does not read the table.
int twins_window_attention(const float* qkv, int F, int H, int W, int ws, int heads, int dh, const float* zero_table, float* out, hipStream_t s);
int twins_window_attention_bwd(const float* qkv, const float* dout, int F, int H, int W, int ws, int heads, int dh, const float* zero_table,
                               float* dqkv, hipStream_t s);

// What both forms of the launches refuse, with the text.  Returns the message or null.
inline const char* twins_attn_refusal(const TwinsAttn& p, bool bwd) {
    const int64_t C = (int64_t)p.H * p.dh;
    if (!p.q || !p.kv || (bwd ? (!p.dout || !p.dq || !p.dkv) : !p.out)) return "null argument";
    if (p.F <= 0 || p.Tq <= 0 || p.Tk <= 0 || p.H <= 0 || p.dh <= 0) return "frames, queries, keys, heads and head width must be positive";
    if (p.dh % 4 != 0) return "the head width must be a multiple of 4";
    if (p.dh > TWINS_MAX_DH) return "a head wider than 64: one head's K and V do not fit the staged tile";
    if (p.Tk > TWINS_MAX_TK) return "more than 64 keys: one head's whole K and V are staged in one workgroup's LDS";
    if ((int64_t)p.F * p.Tq * C >= (1ll << 31) || (int64_t)p.F * p.Tk * 2 * C >= (1ll << 31)) return "more than 2^31 elements";
    if (p.F > 65535 || p.H > 65535) return "a grid dimension over 65535 (frames or heads)";
    const uintptr_t al = (uintptr_t)p.q | (uintptr_t)p.kv | (uintptr_t)(bwd ? p.dout : p.out) | (uintptr_t)(bwd ? p.dq : p.out) |
                         (uintptr_t)(bwd ? p.dkv : p.out);
    if (al & 15) return "16-byte alignment needed";
    return nullptr;
}

inline const char* twins_block_refusal(const void* a, const void* b, int F, int H, int W, int C, int sr) {
    if (!a || !b) return "null argument";
    if (F <= 0 || H <= 0 || W <= 0 || C <= 0) return "frames, plane and channels must be positive";
    if (sr != 2 && sr != 4 && sr != 8) return "the block side must be 2, 4 or 8";
    if (H % sr != 0 || W % sr != 0) return "the plane must be a whole number of blocks";
    if (C % 4 != 0) return "the channel count must be a multiple of 4";
    if ((int64_t)F * H * W * C >= (1ll << 31)) return "more than 2^31 elements";
    if (a == b) return "the two arrays must not overlap";
    if (((uintptr_t)a | (uintptr_t)b) & 15) return "16-byte alignment needed";
    return nullptr;
}

inline const char* twins_window_refusal(const void* a, const void* b, const void* c, int F, int H, int W, int ws, int heads, int dh) {
    if (!a || !b || !c) return "null argument";
    if (F <= 0 || heads <= 0 || H <= 0 || W <= 0 || H % ws != 0 || W % ws != 0 || !((ws == 7 && dh == 32) || (ws == 4 && dh == 16)))
        return "window 7 with head width 32 or window 4 with head width 16, on a grid of whole windows";
    if ((int64_t)F * H * W * 3 * heads * dh >= (1ll << 31)) return "more than 2^31 elements";
    if (((uintptr_t)a | (uintptr_t)b | (uintptr_t)c) & 15) return "16-byte alignment needed";
    return nullptr;
}
