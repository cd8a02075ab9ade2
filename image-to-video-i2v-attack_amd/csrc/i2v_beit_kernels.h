// Internal interface of the BEiT launches (i2v_beit.hip; without -DI2V_HAVE_BEIT the same as scalar host code, i2v_beit_host.h) to
// their planner (i2v_beit.cpp).  The linear layers, the LayerNorm pair and patchify are the shared ones (i2v_vit_kernels.h).
#pragma once
#ifdef __HIP__
#include <hip/hip_runtime.h>
#else
#include "i2v_hip_stub.h"     // (no HIP: the host simulation's build)
#endif
#include <stdint.h>

enum { BEIT_MAX_T = 208, BEIT_MAX_DH = 64 };      // one head's whole K and V (13 tiles of 16 rows, 64 wide) live in one workgroup's LDS

// Biased global attention on qkv (F, T, 3 H dh): q of head h at column h dh, k at H dh + h dh, v at 2 H dh + h dh.  Per frame and head:
//   forward   S = scale q k^T + bias_h (T, T) | P = softmax over the keys | out = P v, out (F, T, H dh)
//   backward  from dout (F, T, H dh), P recomputed:  dP = dout v^T | dS = scale P (dP - rowsum(dP P)) | dq = dS k | dk = dS^T q |
//             dv = P^T dout, into dqkv laid out as qkv.  No gradient for the bias.
// bias: (H, T, T) with row stride T, or null (plain attention).
struct BeitAttn {
    const float *qkv, *bias;
    int32_t F, T, H, dh;
    float scale;
    float* out;                        // forward
    const float* dout;                 // backward
    float* dqkv;
};
int beit_attention(const BeitAttn& p, hipStream_t s);             // one launch
int beit_attention_bwd(const BeitAttn& p, hipStream_t s);         // two launches: dq by (frame, head), then dk / dv by (frame, head)

// The launch of the shared-launch route of the planner (I2V_BEIT_ATTN=0) that the shared interface does not carry:
//   beit_bias_add   S (F, H, T, ld) += bias (H, T, ld), ld % 4 == 0: every element, the padding columns included
int beit_bias_add(float* S, const float* bias, int F, int64_t per_frame, hipStream_t s);

// What both forms of the attention launches refuse, with the text.  Returns the message or null.
inline const char* beit_attn_refusal(const BeitAttn& p, bool bwd) {
    if (!p.qkv || (bwd ? (!p.dout || !p.dqkv) : !p.out)) return "null argument";
    if (p.F <= 0 || p.T <= 0 || p.H <= 0 || p.dh <= 0) return "frames, tokens, heads and head width must be positive";
    if (p.dh % 4 != 0) return "the head width must be a multiple of 4";
    if (p.dh > BEIT_MAX_DH) return "a head wider than 64: one head's K and V do not fit the staged tile";
    if (p.T > BEIT_MAX_T) return "more than 208 tokens: one head's whole K and V are staged in one workgroup's LDS";
    if (p.F > 65535 || p.H > 65535) return "a grid dimension over 65535 (frames or heads)";
    if ((int64_t)p.F * p.T * 3 * p.H * p.dh >= (1ll << 31) || (int64_t)p.H * p.T * p.T >= (1ll << 31)) return "more than 2^31 elements";
    const uintptr_t al = (uintptr_t)p.qkv | (uintptr_t)p.bias | (uintptr_t)(bwd ? p.dout : p.out) | (uintptr_t)(bwd ? p.dqkv : p.out);
    if (al & 15) return "16-byte alignment needed";
    return nullptr;
}

inline const char* beit_bias_add_refusal(const float* S, const float* bias, int F, int64_t per_frame) {
    if (!S || !bias) return "null argument";
    if (F <= 0 || per_frame <= 0 || per_frame % 4 != 0) return "frames must be positive and a frame's scores a positive multiple of 4 floats";
    if ((int64_t)F * per_frame >= (1ll << 40)) return "more than 2^40 elements";
    if (((uintptr_t)S | (uintptr_t)bias) & 15) return "16-byte alignment needed";
    return nullptr;
}
