// Internal interface of the XCiT launches (i2v_xcit.hip; without -DI2V_HAVE_XCIT the same as scalar host code, i2v_xcit_host.h) to their
// planner (i2v_xcit.cpp).  The linear layers and the LayerNorm pair are the ViT ones (i2v_vit_kernels.h).
#pragma once
#ifdef __HIP__
#include <hip/hip_runtime.h>
#else
#include "i2v_hip_stub.h"     // (no HIP: the host simulation's build)
#endif
#include <stdint.h>

enum { XCIT_MAX_DH = 64 };      // widest head: the dh x dh matrices of one head live in one workgroup's LDS and MFMA accumulators

// Cross-covariance attention over qkv (F, T, 3 H dh), token-major as the ViT entry takes it: q of head h at column h dh, k at H dh + h dh,
// v at 2 H dh + h dh.  Per frame and head, with nq[i] = max(||q[:, i]||_2, 1e-12) over the T tokens and nk[j] likewise:
//   forward   Gh[i][j] = (sum_t q[t][i] k[t][j]) / nq[i] / nk[j] | A = softmax over j of temperature[h] * Gh | out[t][i] = sum_j A[i][j] v[t][j]
//             gram: (F, H, dh + 2, dh) receives Gh in rows 0 .. dh - 1, nq in row dh and nk in row dh + 1; probs: (F, H, dh, dh) receives
//             A; out: (F, T, H dh).
//   backward  dqkv (F, T, 3 H dh) from dout (F, T, H dh), qkv, gram and probs:  dA = dout^T v | dS = A (dA - rowsum(dA A)) | dG =
//             temperature dS | r[i] = sum_j dG[i][j] Gh[i][j], c[j] = sum_i dG[i][j] Gh[i][j] | dv = dout A |
//             dq[t][i] = (sum_j k[t][j] dG[i][j] / nk[j] - q[t][i] r[i] / nq[i]) / nq[i] | dk[t][j] = (sum_i q[t][i] dG[i][j] / nq[i] -
//             k[t][j] c[j] / nk[j]) / nk[j].
struct XcitAttn {
    const float* qkv;
    int32_t F, T, H, dh;
    const float* temperature;          // (H)
    float *gram, *probs, *out;         // forward: written; backward: gram and probs read
    const float* dout;                 // backward
    float* dqkv;
};

constexpr float XCIT_NORM_EPS = 1e-12f;
constexpr int xcit_dp(int dh) { return (dh + 15) / 16 * 16; }      // the head width as the MFMA tiles see it

int xcit_attention(const XcitAttn& p, hipStream_t s);
int xcit_attention_bwd(const XcitAttn& p, hipStream_t s);

// Token-major depthwise 3 x 3, pad 1, stride 1, on x (N, H, W, C) with the filter as w (9, C), tap = 3 ky + kx:
//   z(p) = ta ? ta[c] * gelu(x(p)) + ts[c] : x(p) for p in the plane, 0 outside it
//   y = sum_taps w[tap][c] z(p + tap) (+ b[c]) (+ add) ; then y *= ma[c] * gelu'(mu) where ma is given
// add, mu and y are (N, H, W, C); y must not overlap x.  add may be y.
struct XcitDw3 {
    const float *x, *w, *b;            // b may be null
    const float *ta, *ts;              // the input transform, both or neither
    const float* add;                  // may be null
    const float *ma, *mu;              // the output multiply, both or neither
    float* y;
    int32_t N, H, W, C;
};
int xcit_dw3(const XcitDw3& p, hipStream_t s);

// The stem's 3 x 3 / stride 2 / pad 1 convolutions as a gather and a product.  Ho = (H + 1) / 2, Wo = (W + 1) / 2.
//   gather   rows (F Ho Wo, 9 C): rows[(f, oy, ox)][tap C + c] = src(f, 2 oy - 1 + ky, 2 ox - 1 + kx, c), 0 outside the plane
//   scatter  its transpose, in gather form: dst(f, y, x, c) = (sum over the taps and output positions that read (y, x), ky then kx
//            increasing) drows[...] (* gelu'(pre(f, y, x, c))); one owner per element of dst
// src / dst are token-major (F, H, W, C), or with `nchw` the image layout (F, C, H, W); pre is token-major.  `accumulate` adds to dst.
int xcit_stem_gather(const float* src, float* rows, int F, int H, int W, int C, int nchw, hipStream_t s);
int xcit_stem_scatter(const float* drows, const float* pre, float* dst, int F, int H, int W, int C, int nchw, int accumulate, hipStream_t s);

// What both forms of the launches refuse, with the text.  Returns the message or null.
inline const char* xcit_attn_refusal(const XcitAttn& p, bool bwd) {
    const int64_t C = (int64_t)p.H * p.dh;
    if (!p.qkv || !p.temperature || !p.gram || !p.probs || (bwd ? (!p.dout || !p.dqkv) : !p.out)) return "null argument";
    if (p.F <= 0 || p.T <= 0 || p.H <= 0 || p.dh <= 0) return "frames, tokens, heads and head width must be positive";
    if (p.dh % 4 != 0) return "the head width must be a multiple of 4";
    if (p.dh > XCIT_MAX_DH) return "a head wider than 64: its dh x dh matrices do not fit one workgroup's LDS and register budget";
    if ((int64_t)p.F * p.T * 3 * C >= (1ll << 31) || (int64_t)p.F * p.H * (p.dh + 2) * p.dh >= (1ll << 31)) return "more than 2^31 elements";
    if (p.F > 65535 || p.H > 65535) return "a grid dimension over 65535 (frames or heads)";
    const uintptr_t al = (uintptr_t)p.qkv | (uintptr_t)p.gram | (uintptr_t)p.probs | (uintptr_t)(bwd ? p.dout : p.out) |
                         (uintptr_t)(bwd ? p.dqkv : p.out);
    if (al & 15) return "16-byte alignment needed";
    return nullptr;
}

inline const char* xcit_dw3_refusal(const XcitDw3& p) {
    if (!p.x || !p.w || !p.y) return "null argument";
    if ((p.ta == nullptr) != (p.ts == nullptr)) return "the input transform takes both of its arrays or neither";
    if ((p.ma == nullptr) != (p.mu == nullptr)) return "the output multiply takes both of its arrays or neither";
    if (p.N <= 0 || p.H <= 0 || p.W <= 0 || p.C <= 0) return "frames, plane and channels must be positive";
    if (p.C % 4 != 0) return "the channel count must be a multiple of 4";
    if ((int64_t)p.N * p.H * p.W * p.C >= (1ll << 31)) return "more than 2^31 elements";
    if (p.x == p.y) return "y must not overlap x";
    const uintptr_t al = (uintptr_t)p.x | (uintptr_t)p.w | (uintptr_t)p.b | (uintptr_t)p.ta | (uintptr_t)p.ts | (uintptr_t)p.add |
                         (uintptr_t)p.ma | (uintptr_t)p.mu | (uintptr_t)p.y;
    if (al & 15) return "16-byte alignment needed";
    return nullptr;
}

inline const char* xcit_stem_refusal(const void* a, const void* b, int F, int H, int W, int C) {
    if (!a || !b) return "null argument";
    if (F <= 0 || H <= 0 || W <= 0 || C <= 0) return "frames, plane and channels must be positive";
    if ((int64_t)F * ((H + 1) / 2) * ((W + 1) / 2) * 9 * C >= (1ll << 31) || (int64_t)F * H * W * C >= (1ll << 31)) return "more than 2^31 elements";
    if (((uintptr_t)a | (uintptr_t)b) & 15) return "16-byte alignment needed";
    return nullptr;
}
