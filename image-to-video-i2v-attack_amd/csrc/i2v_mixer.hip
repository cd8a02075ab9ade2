// Token mixing of an MLP-Mixer / ResMLP block for gfx950 -- timm's `mlp_tokens` (Linear, GELU, Linear down the token axis) and
// ResMLP's `linear_tokens` -- on the (frame, token, channel) layout the transformer stack keeps its streams in, forward and input
// gradient, ONE launch per block and pass (I2VMixTokParams, i2v_params.h).
//
// One workgroup (4 waves) owns one frame and a tile of CT = 32 or 64 channels.  It stages the frame's (S, CT) slice of the input in
// LDS, computes the (Sh, CT) hidden tile into LDS with the bias and GELU applied in place, and multiplies that by the second weight
// matrix straight into the output: the hidden activation never reaches memory, and nothing is transposed -- the tiles lie as
// (token, channel), which is the B operand of W . tile as it stands.  The backward pass recomputes the pre-activation the same way,
// replaces the input tile by the output's gradient, and runs the two transposed products through the same tiles.
//
//   * products: v_mfma_f32_32x32x2_f32, D (32 rows of W x 32 channels) += A (32 x 2 of W) . B (2 x 32 of the tile).  A wave owns whole
//     32-row blocks of the product (blocks wave, wave + 4, ...) over all CT channels and walks the WHOLE contracted index itself: K is
//     never split, so an element is one fma chain in increasing k (the MFMA adds its two k in order).  Rows, channels and k beyond
//     the end are zero operands; a pair of k that lies wholly beyond K is not issued.
//   * the weights are shared by every workgroup (at most 512 x 196 floats) and come from global memory through L2: a lane reads sixteen
//     consecutive k of its row (four 16-byte loads where the row allows) per eight MFMA steps, one chunk ahead of its use.
//   * LDS: two tiles of (S, CT) and (Sh, CT) floats, rows of CT * 4 = 128 or 256 bytes, carved from one 16-byte-aligned dynamic
//     region at offsets that are multiples of 16.  Operand reads and the epilogue's writes are ds_read_b32 / ds_write_b32 with the 32
//     lanes of a half-wave on 32 consecutive floats of one row: conflict-free under the (address / 4) mod 32 rule, whose two half-waves
//     never conflict with each other; the staging writes are 16-byte writes of consecutive lanes to consecutive slots.
//   * output: the accumulator layout puts channel = lane mod 32, so a half-wave stores 128 contiguous bytes of one token row per
//     store (vector stores only, each element by the one lane that owns it; no atomics).
// Order of operations: I2VMixTokParams (i2v_params.h); i2v_mixer_host.h performs the same ones in the same order.  The result depends
// on neither the frame count nor the channel tile.
#include "i2v_be.h"
#include "i2v_gelu.h"

long long g_stat_mixtok = 0;

namespace {

struct MixGeom {
    int f, c0, l31, lk, wave;
};

constexpr int KCH = 16;      // k per chunk of weight loads: one chunk (4 x 16 bytes per lane) is in flight while the one before feeds 8 MFMA steps

// KCH consecutive k of row `wr` from k0: zero beyond K or when the row does not exist
__device__ __forceinline__ void mix_loadw(const float* __restrict__ wr, int k0, int K, bool rowok, bool vec, float (&w)[KCH]) {
    if (rowok && vec && k0 + KCH <= K) {
#pragma unroll
        for (int j = 0; j < KCH; j += 4) {
            const float4 a = *reinterpret_cast<const float4*>(wr + k0 + j);
            w[j] = a.x; w[j + 1] = a.y; w[j + 2] = a.z; w[j + 3] = a.w;
        }
    } else {
#pragma unroll
        for (int j = 0; j < KCH; ++j) w[j] = (rowok && k0 + j < K) ? wr[k0 + j] : 0.f;
    }
}

// D (M, CT) = W (M, K; K contiguous) . V (K, CT; in LDS, rows of CT floats); epi(m0, acc) receives each 32-row block:
// acc[nb][r] is row m0 + (r & 3) + 8 (r >> 2) + 4 lk, channel nb * 32 + l31
template <int NB, class Epi>
__device__ __forceinline__ void mix_product(const float* __restrict__ W, int M, int K, bool wvec, const float* V, const MixGeom& g, Epi epi) {
    constexpr int CT = 32 * NB;
    for (int m0 = g.wave * 32; m0 < M; m0 += 128) {
        const int m = m0 + g.l31;
        const bool rowok = m < M;
        const float* wr = W + (int64_t)(rowok ? m : 0) * K;
        f32x16 acc[NB];
#pragma unroll
        for (int nb = 0; nb < NB; ++nb)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[nb][r] = 0.f;
        float wn[KCH];
        mix_loadw(wr, 0, K, rowok, wvec, wn);
        for (int k0 = 0; k0 < K; k0 += KCH) {
            float w[KCH];
#pragma unroll
            for (int j = 0; j < KCH; ++j) w[j] = wn[j];
            if (k0 + KCH < K) mix_loadw(wr, k0 + KCH, K, rowok, wvec, wn);
#pragma unroll
            for (int s = 0; s < KCH / 2; ++s) {
                const int kb = k0 + 2 * s;
                if (kb < K) {                                   // (uniform over the workgroup)
                    const int k = kb + g.lk;
                    const bool kok = k < K;
                    const float a = g.lk ? w[2 * s + 1] : w[2 * s];        // zero beyond K already
                    const float* vr = V + (kok ? k : kb) * CT + g.l31;
#pragma unroll
                    for (int nb = 0; nb < NB; ++nb) {
                        float b = vr[nb * 32];
                        if (!kok) b = 0.f;
                        acc[nb] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc[nb], 0, 0, 0);
                    }
                }
            }
        }
        epi(m0, acc);
    }
}

// the frame's (S, CT) slice of `src` into the LDS tile X, columns beyond C zeroed: mode 0 as it is, 1 fma(scale, v, shift), 2 scale * v
template <int NB>
__device__ __forceinline__ void mix_stage(const float* __restrict__ src, bool vec, const float* __restrict__ scale,
                                          const float* __restrict__ shift, int mode, float* X, int S, int C, const MixGeom& g) {
    constexpr int CT = 32 * NB, Q = CT / 4;
    const float* base = src + (int64_t)g.f * S * C;
    for (int i = threadIdx.x; i < S * Q; i += 256) {
        const int s = i / Q, q = i - s * Q, cg = g.c0 + 4 * q;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (cg < C) {                                           // (C % 4 == 0: the quad is whole)
            const float* a = base + (int64_t)s * C + cg;
            if (vec) v = *reinterpret_cast<const float4*>(a);
            else v = make_float4(a[0], a[1], a[2], a[3]);
            if (mode == 1) {
                v.x = __builtin_fmaf(scale[cg], v.x, shift[cg]); v.y = __builtin_fmaf(scale[cg + 1], v.y, shift[cg + 1]);
                v.z = __builtin_fmaf(scale[cg + 2], v.z, shift[cg + 2]); v.w = __builtin_fmaf(scale[cg + 3], v.w, shift[cg + 3]);
            } else if (mode == 2) {
                v.x = __fmul_rn(scale[cg], v.x); v.y = __fmul_rn(scale[cg + 1], v.y);
                v.z = __fmul_rn(scale[cg + 2], v.z); v.w = __fmul_rn(scale[cg + 3], v.w);
            }
        }
        *reinterpret_cast<float4*>(X + s * CT + 4 * q) = v;
    }
}

template <int NB>
__global__ void __launch_bounds__(256) mixer_tokens_kernel(const I2VMixTokParams p, const int zvec, const int rvec, const int wavec,
                                                           const int wbvec, const int wcvec) {
    extern __shared__ __attribute__((aligned(16))) float mix_lds[];
    constexpr int CT = 32 * NB;
    const int S = p.S, Sh = p.Sh, C = p.C;
    float* X = mix_lds;                       // (S, CT)
    float* H = mix_lds + S * CT;              // (Sh, CT); S * CT * 4 is a multiple of 128
    MixGeom g;
    g.f = blockIdx.y; g.c0 = blockIdx.x * CT; g.l31 = threadIdx.x & 31; g.lk = (threadIdx.x >> 5) & 1; g.wave = threadIdx.x >> 6;
    const int64_t fo = (int64_t)g.f * S * C;

    // the last product's epilogue: rows are tokens, a half-wave stores 32 consecutive channels of one row
    auto store = [&](const float* bias, int m0, const f32x16 (&acc)[NB]) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int m = m0 + (r & 3) + 8 * (r >> 2) + 4 * g.lk;
            if (m >= S) continue;
            const float bv = bias ? bias[m] : 0.f;
#pragma unroll
            for (int nb = 0; nb < NB; ++nb) {
                const int cg = g.c0 + nb * 32 + g.l31;
                if (cg >= C) continue;
                const int64_t o = fo + (int64_t)m * C + cg;
                float v = acc[nb][r];
                if (!p.bwd) {
                    v = __fadd_rn(v, bv);
                    if (p.out_scale) v = __fmul_rn(p.out_scale[cg], v);
                    v = __fadd_rn(p.r[o], v);
                } else {
                    if (p.in_scale) v = __fmul_rn(p.in_scale[cg], v);
                    if (p.add0) v = __fadd_rn(p.add0[o], v);
                    if (p.add1) v = __fadd_rn(v, p.add1[o]);
                }
                p.out[o] = v;
            }
        }
    };

    if (!(p.bwd && Sh == 0)) mix_stage<NB>(p.z, zvec, p.in_scale, p.in_shift, p.in_scale ? 1 : 0, X, S, C, g);
    else mix_stage<NB>(p.r, rvec, p.out_scale, nullptr, p.out_scale ? 2 : 0, X, S, C, g);
    __syncthreads();
    if (Sh == 0) {
        if (!p.bwd) mix_product<NB>(p.wa, S, S, wavec, X, g, [&](int m0, const f32x16 (&acc)[NB]) { store(p.ba, m0, acc); });
        else mix_product<NB>(p.wb, S, S, wbvec, X, g, [&](int m0, const f32x16 (&acc)[NB]) { store(nullptr, m0, acc); });
        return;
    }
    // hidden tile: pre = wa . t + ba[row]; forward: GELU in place
    mix_product<NB>(p.wa, Sh, S, wavec, X, g, [&](int m0, const f32x16 (&acc)[NB]) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int m = m0 + (r & 3) + 8 * (r >> 2) + 4 * g.lk;
            if (m >= Sh) continue;
            const float bv = p.ba[m];
#pragma unroll
            for (int nb = 0; nb < NB; ++nb) {
                const float pre = __fadd_rn(acc[nb][r], bv);
                H[m * CT + nb * 32 + g.l31] = p.bwd ? pre : gelu_f(pre);
            }
        }
    });
    __syncthreads();
    if (!p.bwd) {
        mix_product<NB>(p.wb, S, Sh, wbvec, H, g, [&](int m0, const f32x16 (&acc)[NB]) { store(p.bb, m0, acc); });
        return;
    }
    // backward: the input tile becomes out_scale * g; dH = W2^T . g times gelu'(pre) in place; dz = W1^T . dH
    mix_stage<NB>(p.r, rvec, p.out_scale, nullptr, p.out_scale ? 2 : 0, X, S, C, g);
    __syncthreads();
    mix_product<NB>(p.wb, Sh, S, wbvec, X, g, [&](int m0, const f32x16 (&acc)[NB]) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int m = m0 + (r & 3) + 8 * (r >> 2) + 4 * g.lk;
            if (m >= Sh) continue;
#pragma unroll
            for (int nb = 0; nb < NB; ++nb) {
                float* h = H + m * CT + nb * 32 + g.l31;
                *h = __fmul_rn(acc[nb][r], gelu_grad_f(*h));
            }
        }
    });
    __syncthreads();
    mix_product<NB>(p.wc, S, Sh, wcvec, H, g, [&](int m0, const f32x16 (&acc)[NB]) { store(nullptr, m0, acc); });
}

bool mix_al16(const void* q) { return ((uintptr_t)q & 15) == 0; }

}  // namespace

int k_mixer_tokens_plan(I2VMixTokParams* p) {
    if (!p->out || !p->r || p->F < 0 || p->S < 1 || p->Sh < 0 || p->C < 4 || p->C % 4 != 0) return 1;
    if ((p->in_scale == nullptr) != (p->in_shift == nullptr)) return 1;
    if (p->Sh > 0 ? (!p->z || !p->wa || !p->ba || !p->wb || (p->bwd ? !p->wc : !p->bb)) : (p->bwd ? !p->wb : (!p->z || !p->wa || !p->ba))) return 1;
    const int want = p->ct;
    if (want != 0 && want != 32 && want != 64) return 1;
    const int ct = want ? want : 32;      // (measured: 32 is the faster tile on every served shape forward)
    if ((int64_t)(p->S + p->Sh) * ct * 4 > I2V_MIXTOK_LDS_MAX) return 1;
    p->ct = ct;
    p->lds_bytes = (p->S + p->Sh) * ct * 4;
    return 0;
}

int k_mixer_tokens(const I2VMixTokParams& p, i2v_stream_t st) {
    hipStream_t s = (hipStream_t)st;
    I2VMixTokParams q = p;
    if ((p.ct != 32 && p.ct != 64) || k_mixer_tokens_plan(&q) != 0 || q.ct != p.ct || q.lds_bytes != p.lds_bytes)
        return hip_fail(hipErrorInvalidValue, "k_mixer_tokens: launch not planned (k_mixer_tokens_plan)");
    if (p.F == 0) return 0;
    if ((int64_t)p.F * p.S * p.C >= (1ll << 31)) return hip_fail(hipErrorInvalidValue, "k_mixer_tokens: more than 2^31 elements");
    const dim3 grid((unsigned)((p.C + p.ct - 1) / p.ct), (unsigned)p.F);
    if (grid.y > 65535u) return hip_fail(hipErrorInvalidValue, "k_mixer_tokens: more than 65535 frames");
    // 16-byte accesses where the arrays allow them: activations by their base (C % 4 == 0), weight rows by their length too
    const int zvec = p.z ? mix_al16(p.z) : 0, rvec = mix_al16(p.r);
    const int Ka = p.S, Kb = p.bwd ? p.S : p.Sh, Kc = p.Sh;
    const int wavec = p.wa && mix_al16(p.wa) && Ka % 4 == 0, wbvec = p.wb && mix_al16(p.wb) && Kb % 4 == 0 && Kb > 0,
              wcvec = p.wc && mix_al16(p.wc) && Kc % 4 == 0 && Kc > 0;
    const int nb = p.ct / 32 - 1;
    if (p.lds_bytes > 64 * 1024) {      // past the default dynamic LDS limit: raised per launch (a host-side setting of the current device)
        const hipError_t e = nb ? hipFuncSetAttribute((const void*)mixer_tokens_kernel<2>, hipFuncAttributeMaxDynamicSharedMemorySize, I2V_MIXTOK_LDS_MAX)
                                : hipFuncSetAttribute((const void*)mixer_tokens_kernel<1>, hipFuncAttributeMaxDynamicSharedMemorySize, I2V_MIXTOK_LDS_MAX);
        if (e != hipSuccess) return hip_fail(e, "k_mixer_tokens: hipFuncSetAttribute(MaxDynamicSharedMemorySize)");
    }
    __atomic_fetch_add(&g_stat_mixtok, 1, __ATOMIC_RELAXED);
    if (nb) hipLaunchKernelGGL((mixer_tokens_kernel<2>), grid, dim3(256), (size_t)p.lds_bytes, s, p, zvec, rvec, wavec, wbvec, wcvec);
    else hipLaunchKernelGGL((mixer_tokens_kernel<1>), grid, dim3(256), (size_t)p.lds_bytes, s, p, zvec, rvec, wavec, wbvec, wcvec);
    LAUNCH_CHECK("mixer_tokens_kernel");
    return 0;
}
