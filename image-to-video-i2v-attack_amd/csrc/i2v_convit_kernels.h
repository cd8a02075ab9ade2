// Internal interface of the ConViT launches (i2v_convit.hip; without -DI2V_HAVE_CONVIT the same as scalar host code, i2v_convit_host.h)
// to their planner (i2v_convit.cpp).  The linear layers, the LayerNorm pair and the patchify kernel are the ViT ones (i2v_vit_kernels.h).
#pragma once
#ifdef __HIP__
#include <hip/hip_runtime.h>
#else
#include "i2v_hip_stub.h"     // (no HIP: the host simulation's build)
#endif
#include <stdint.h>

enum { CONVIT_TILE = 16, CONVIT_LDS_MAX = 160 * 1024 };

// Gated positional self-attention over qkv (F, T, 3 H dh), token-major as the ViT entry takes it: q of head h at column h dh, k at
// H dh + h dh, v at 2 H dh + h dh.  c: (H), table: (H, T, ld) with ld = convit_probs_ld(T), non-negative; both null: plain attention.
//   forward   S_h = (scale q_h) k_h^T | Ppatch_h = softmax over keys | P_h = fma(c_h, Ppatch_h, table_h) (P_h = Ppatch_h without a table)
//             | out_h = P_h v_h.  P: (F, H, T, ld) receives Ppatch; out: (F, T, H dh).  Nothing is divided: the caller's table and c make
//             the rows of P sum to one (ConvitSpec.native_arrays), and the entry takes any non-negative table.
//   backward  dqkv (F, T, 3 H dh) from dout (F, T, H dh), qkv and P; dS is scratch of P's size (the gradient of S, written by the
//             row-tile launch and read by the key-tile launch).  dS = Ppatch * (c dP - sum_j c dP Ppatch), dP = dout v^T.
struct ConvitAttn {
    const float* qkv;
    int32_t F, T, H, dh;
    float scale;
    const float *c, *table;
    float *P, *out;                    // forward: written; backward: P read
    const float* dout;                 // backward
    float *dS, *dqkv;
};

constexpr int convit_probs_ld(int T) { return (T + 3) / 4 * 4; }
// LDS bytes of one workgroup: one score tile of 16 rows by (T rounded up to 16, plus 4) keys
constexpr int64_t convit_lds_bytes(int T) { return (int64_t)CONVIT_TILE * ((T + 15) / 16 * 16 + 4) * 4; }

int convit_attention(const ConvitAttn& p, hipStream_t s);
int convit_attention_bwd(const ConvitAttn& p, hipStream_t s);
// out (F, T + 1, C) = [cls (C); x (F, T, C)]
int convit_join_cls(const float* x, const float* cls, float* out, int F, int T, int C, hipStream_t s);
// dx (F, T, C) = rows 1 .. T of dout (F, T + 1, C) (+ add (F, T, C)): the class token is a weight and gets no gradient
int convit_join_cls_bwd(const float* dout, const float* add, float* dx, int F, int T, int C, hipStream_t s);

// What both forms of the launches refuse, with the text.  Returns the message or null.
inline const char* convit_attn_refusal(const ConvitAttn& p, bool bwd) {
    const int64_t C = (int64_t)p.H * p.dh;
    if (!p.qkv || !p.P || (bwd ? (!p.dout || !p.dS || !p.dqkv) : !p.out)) return "null argument";
    if ((p.c == nullptr) != (p.table == nullptr)) return "c and table go together: both given (gated positional attention) or both null (plain attention)";
    if (p.F <= 0 || p.T <= 0 || p.H <= 0 || p.dh <= 0) return "frames, tokens, heads and head width must be positive";
    if (p.dh % 4 != 0) return "the head width must be a multiple of 4";
    if (convit_lds_bytes(p.T) > CONVIT_LDS_MAX) return "more keys than the LDS budget holds (16 rows x keys floats within 160 KiB)";
    if ((int64_t)p.F * p.T * 3 * C >= (1ll << 31) || (int64_t)p.F * p.H * p.T * convit_probs_ld(p.T) >= (1ll << 31)) return "more than 2^31 elements";
    if (p.F > 65535 || p.H > 65535 || (p.T + CONVIT_TILE - 1) / CONVIT_TILE > 65535)
        return "a grid dimension over 65535 (frames, heads, or tiles of 16 tokens)";
    const uintptr_t al = (uintptr_t)p.qkv | (uintptr_t)p.P | (uintptr_t)p.table | (uintptr_t)(bwd ? p.dout : p.out) |
                         (uintptr_t)(bwd ? p.dqkv : p.out) | (uintptr_t)(bwd ? p.dS : p.P);
    if (al & 15) return "16-byte alignment needed";
    return nullptr;
}
