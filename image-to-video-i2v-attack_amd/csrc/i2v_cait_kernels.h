// Internal interface of the CaiT launches (i2v_cait.hip; without -DI2V_HAVE_CAIT the same three as scalar host code, i2v_cait_host.h)
// to their planner (i2v_cait.cpp).  The linear layers, the LayerNorm pair and the patchify kernel are the ViT ones (i2v_vit_kernels.h).
#pragma once
#ifdef __HIP__
#include <hip/hip_runtime.h>
#else
#include "i2v_hip_stub.h"     // (no HIP: the host simulation's build)
#endif
#include <stdint.h>

enum { CAIT_TILE = 16, CAIT_MAX_HEADS = 16, CAIT_LDS_MAX = 160 * 1024 };

// Talking-heads attention over qkv (F, T, 3 H dh), token-major as the ViT entry takes it: q of head h at column h dh, k at H dh + h dh,
// v at 2 H dh + h dh.  wl, ww: (H, H) row-major [g][h] (attn.proj_l.weight, attn.proj_w.weight); bl, bw: (H).
//   forward   S_h = (scale q_h) k_h^T | S'_g = sum_h wl[g][h] S_h + bl[g] | P_g = softmax over keys | P'_g = sum_h ww[g][h] P_h + bw[g] |
//             out_g = P'_g v_g.  P: (F, H, T, ld), ld = cait_probs_ld(T), post-softmax and pre-mix; out: (F, T, H dh).
//   backward  dqkv (F, T, 3 H dh) from dout (F, T, H dh), qkv and P; dS and Pm are scratch of P's size (the gradient of S and the mixed
//             probabilities P', written by the row-tile launch and read by the key-tile launch).
struct CaitAttn {
    const float* qkv;
    int32_t F, T, H, dh;
    float scale;
    const float *wl, *bl, *ww, *bw;
    float *P, *out;                    // forward: written; backward: P read
    const float* dout;                 // backward
    float *dS, *Pm, *dqkv;
};

constexpr int cait_probs_ld(int T) { return (T + 3) / 4 * 4; }
// LDS bytes of one workgroup: H score tiles of 16 rows by (T rounded up to 16, plus 4) keys
constexpr int64_t cait_lds_bytes(int T, int H) { return (int64_t)H * CAIT_TILE * ((T + 15) / 16 * 16 + 4) * 4; }

int cait_attention(const CaitAttn& p, hipStream_t s);
int cait_attention_bwd(const CaitAttn& p, hipStream_t s);
// x (F, T, C) += pos (T, C)
int cait_add_pos(float* x, const float* pos, int F, int T, int C, hipStream_t s);

// What both forms of the launches refuse, with the text: null or misaligned arrays, a head width that is no multiple of 4, more heads than
// the LDS holds, more than 2^31 elements, a grid dimension over 65 535.  Returns the message or null.
inline const char* cait_attn_refusal(const CaitAttn& p, bool bwd) {
    const int64_t C = (int64_t)p.H * p.dh;
    if (!p.qkv || !p.wl || !p.ww || !p.bw || !p.P || (bwd ? (!p.dout || !p.dS || !p.Pm || !p.dqkv) : (!p.bl || !p.out))) return "null argument";
    if (p.F <= 0 || p.T <= 0 || p.H <= 0 || p.dh <= 0) return "frames, tokens, heads and head width must be positive";
    if (p.dh % 4 != 0) return "the head width must be a multiple of 4";
    if (p.H > CAIT_MAX_HEADS || cait_lds_bytes(p.T, p.H) > CAIT_LDS_MAX)
        return "more heads than the LDS budget holds (heads x 16 rows x keys floats within 160 KiB, at most 16 heads)";
    if ((int64_t)p.F * p.T * 3 * C >= (1ll << 31) || (int64_t)p.F * p.H * p.T * cait_probs_ld(p.T) >= (1ll << 31)) return "more than 2^31 elements";
    if (p.F > 65535 || (p.T + CAIT_TILE - 1) / CAIT_TILE > 65535) return "a grid dimension over 65535 (frames, or tiles of 16 tokens)";
    const uintptr_t al = (uintptr_t)p.qkv | (uintptr_t)p.P | (uintptr_t)(bwd ? p.dout : p.out) | (uintptr_t)(bwd ? p.dqkv : p.out) |
                         (uintptr_t)(bwd ? p.dS : p.P) | (uintptr_t)(bwd ? p.Pm : p.P);
    if (al & 15) return "16-byte alignment needed";
    return nullptr;
}
