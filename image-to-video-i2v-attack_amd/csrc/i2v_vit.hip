// Kernels of the ViT surrogate (include/i2v_vit.h).  Activations are TOKEN-MAJOR: a frame is a (tokens, C) row-major
// matrix, so every linear layer is one GEMM over frames * tokens rows and a head's q / k / v are 64-column slices of the qkv rows.
//
//   vit_gemm_kernel     C[b](m, n) = alpha * sum_k A[b](m, k) B[b](k, n)  (+ bias[n]) (+ R[b](m, n)), fp32 MFMA (v_mfma_f32_32x32x2_f32,
//                       exact f32 products and sums); batch b = outer * nb_in + inner with one stride per level, so the (frame, head)
//                       matrices of attention are one launch.  Epilogues: plain, GELU (C = pre-activation, C2 = gelu(C)), GELU
//                       backward (C = acc * gelu'(H)).
//   vit_layernorm_*     LayerNorm over the last axis (biased variance), forward saving (mean, rstd), backward to the input plus addends.
//   vit_softmax_*       row softmax over the keys in place (rows padded to a multiple of 4 floats), and its backward times a scale.
//   vit_patchify / vit_assemble     token assembly (patch x patch patches -> rows, prefix tokens + pos_embed) and its backward.
#include <algorithm>

#include "i2v_be.h"
#include "i2v_gelu.h"          // gelu_f, gelu_grad_f (shared with i2v_mixer.hip)
#include "i2v_vit_kernels.h"

namespace {

constexpr int TM = 128, TN = 128, KC = 16;
constexpr int ST = 132;        // LDS row stride of an operand transposed on the way in (K contiguous in memory): conflict-free writes
constexpr int SD = 160;        // ... of an operand stored as it is (M / N contiguous): the two 32-lane halves of an MFMA read 32 banks apart

__device__ __forceinline__ float4 ld4(const float* p, int lim, bool vec) {
    if (lim >= 4 && vec) return *reinterpret_cast<const float4*>(p);
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (lim > 0) v.x = p[0];
    if (lim > 1) v.y = p[1];
    if (lim > 2) v.z = p[2];
    if (lim > 3) v.w = p[3];
    return v;
}

// AK: A is K-contiguous (a_sk == 1), else M-contiguous (a_sm == 1).  BK: B is K-contiguous (b_sk == 1), else N-contiguous (b_sn == 1).
template <bool AK, bool BK>
__global__ void __launch_bounds__(256) vit_gemm_kernel(const VitGemm p) {
    __shared__ __attribute__((aligned(16))) float Ls[2][KC][AK ? ST : SD], Rs[2][KC][BK ? ST : SD];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, wm = wave >> 1, wn = wave & 1, l31 = lane & 31, lk = lane >> 5;
    const int tiles_n = (p.N + TN - 1) / TN;
    const int m0 = (blockIdx.x / tiles_n) * TM, n0 = (blockIdx.x % tiles_n) * TN;
    const int bo = blockIdx.y / p.nb_in, bi = blockIdx.y - bo * p.nb_in;
    const float* A = p.A + bo * p.a_bo + bi * p.a_bi;
    const float* B = p.B + bo * p.b_bo + bi * p.b_bi;
    // thread's share of a chunk, pieces h = 0, 1.  K-contiguous operand: row (m or n) t / 4 + 64 h, four k from (t % 4) * 4;
    // M/N-contiguous: k = t / 32 + 8 h, four rows from (t % 32) * 4
    const int r4 = t >> 2, k4 = (t & 3) * 4, kr = t >> 5, c4 = (t & 31) * 4;
    float4 ra[2], rb[2];
    auto fetch = [&](const int k0) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            if constexpr (AK) {
                const int m = m0 + r4 + 64 * h, k = k0 + k4;
                ra[h] = (m < p.M && k < p.K) ? ld4(A + m * p.a_sm + k, p.K - k, p.a_vec) : make_float4(0.f, 0.f, 0.f, 0.f);
            } else {
                const int m = m0 + c4, k = k0 + kr + 8 * h;
                ra[h] = (m < p.M && k < p.K) ? ld4(A + k * p.a_sk + m, p.M - m, p.a_vec) : make_float4(0.f, 0.f, 0.f, 0.f);
            }
            if constexpr (BK) {
                const int n = n0 + r4 + 64 * h, k = k0 + k4;
                rb[h] = (n < p.N && k < p.K) ? ld4(B + n * p.b_sn + k, p.K - k, p.b_vec) : make_float4(0.f, 0.f, 0.f, 0.f);
            } else {
                const int n = n0 + c4, k = k0 + kr + 8 * h;
                rb[h] = (n < p.N && k < p.K) ? ld4(B + k * p.b_sk + n, p.N - n, p.b_vec) : make_float4(0.f, 0.f, 0.f, 0.f);
            }
        }
    };
    auto stash = [&](const int buf) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            if constexpr (AK) {
                const int m = r4 + 64 * h;
                Ls[buf][k4][m] = ra[h].x; Ls[buf][k4 + 1][m] = ra[h].y; Ls[buf][k4 + 2][m] = ra[h].z; Ls[buf][k4 + 3][m] = ra[h].w;
            } else {
                *reinterpret_cast<float4*>(&Ls[buf][kr + 8 * h][c4]) = ra[h];
            }
            if constexpr (BK) {
                const int n = r4 + 64 * h;
                Rs[buf][k4][n] = rb[h].x; Rs[buf][k4 + 1][n] = rb[h].y; Rs[buf][k4 + 2][n] = rb[h].z; Rs[buf][k4 + 3][n] = rb[h].w;
            } else {
                *reinterpret_cast<float4*>(&Rs[buf][kr + 8 * h][c4]) = rb[h];
            }
        }
    };
    // the TRANSPOSED product D^T = B^T A^T per 32x32 fragment: lane -> m (column of D^T), register r -> n = (r&3) + 8(r>>2) + 4 lk, so
    // each lane owns four consecutive n per register quad and the epilogue reads and writes float4
    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
    const int nchunks = (p.K + KC - 1) / KC;
    fetch(0); stash(0);
    __syncthreads();
    for (int c = 0; c < nchunks; ++c) {
        const int buf = c & 1;
        if (c + 1 < nchunks) fetch((c + 1) * KC);
#pragma unroll
        for (int s = 0; s < KC / 2; ++s) {
            const int k = 2 * s + lk;
            const float a0 = Ls[buf][k][wm * 64 + l31], a1 = Ls[buf][k][wm * 64 + 32 + l31];
            const float b0 = Rs[buf][k][wn * 64 + l31], b1 = Rs[buf][k][wn * 64 + 32 + l31];
            acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(b0, a0, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(b1, a0, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(b0, a1, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(b1, a1, acc[1][1], 0, 0, 0);
        }
        if (c + 1 < nchunks) stash(buf ^ 1);
        __syncthreads();
    }
    const int64_t cb = bo * p.c_bo + bi * p.c_bi;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int m = m0 + wm * 64 + i * 32 + l31;
        if (m >= p.M) continue;
        const int64_t row = cb + (int64_t)m * p.c_sm;
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int n = n0 + wn * 64 + j * 32 + 8 * q + 4 * lk;
                if (n >= p.N) continue;
                const int lim = p.N - n;
                float v[4] = {acc[i][j][4 * q], acc[i][j][4 * q + 1], acc[i][j][4 * q + 2], acc[i][j][4 * q + 3]};
                if (p.alpha != 1.f)
                    for (int e = 0; e < 4; ++e) v[e] = __fmul_rn(p.alpha, v[e]);
                if (p.bias) {
                    const float4 bb = ld4(p.bias + n, lim, p.bias_vec);
                    v[0] = __fadd_rn(v[0], bb.x); v[1] = __fadd_rn(v[1], bb.y); v[2] = __fadd_rn(v[2], bb.z); v[3] = __fadd_rn(v[3], bb.w);
                }
                if (p.R) {
                    const float4 rr = ld4(p.R + row + n, lim, p.c_vec);
                    v[0] = __fadd_rn(rr.x, v[0]); v[1] = __fadd_rn(rr.y, v[1]); v[2] = __fadd_rn(rr.z, v[2]); v[3] = __fadd_rn(rr.w, v[3]);
                }
                if (p.mode == VIT_EPI_GELU_BWD) {
                    const float4 hh = ld4(p.H + row + n, lim, p.c_vec);
                    v[0] = __fmul_rn(v[0], gelu_grad_f(hh.x)); v[1] = __fmul_rn(v[1], gelu_grad_f(hh.y));
                    v[2] = __fmul_rn(v[2], gelu_grad_f(hh.z)); v[3] = __fmul_rn(v[3], gelu_grad_f(hh.w));
                }
                float* o = p.C + row + n;
                if (lim >= 4 && p.c_vec) *reinterpret_cast<float4*>(o) = make_float4(v[0], v[1], v[2], v[3]);
                else for (int e = 0; e < lim && e < 4; ++e) o[e] = v[e];
                if (p.mode == VIT_EPI_GELU) {
                    float* o2 = p.C2 + row + n;
                    const float g[4] = {gelu_f(v[0]), gelu_f(v[1]), gelu_f(v[2]), gelu_f(v[3])};
                    if (lim >= 4 && p.c_vec) *reinterpret_cast<float4*>(o2) = make_float4(g[0], g[1], g[2], g[3]);
                    else for (int e = 0; e < lim && e < 4; ++e) o2[e] = g[e];
                }
            }
    }
}

__device__ __forceinline__ float wsum(float v) {
    for (int o = 32; o > 0; o >>= 1) v = __fadd_rn(v, __shfl_xor(v, o));
    return v;
}
__device__ __forceinline__ float wmax(float v) {
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    return v;
}

// one wave per row; lanes walk the row in float4 steps (C % 4 == 0 and aligned rows) or element by element
__global__ void __launch_bounds__(256) vit_layernorm_kernel(const float* __restrict__ x, int64_t rows, int C, const float* __restrict__ gamma,
                                                            const float* __restrict__ beta, float eps, float* __restrict__ out,
                                                            float* __restrict__ mean, float* __restrict__ rstd, int vec) {
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= rows) return;
    const float* xr = x + r * C;
    float* orow = out + r * C;
    float s = 0.f;
    if (vec) for (int c = 4 * lane; c < C; c += 256) { const float4 v = *reinterpret_cast<const float4*>(xr + c); s = __fadd_rn(s, __fadd_rn(__fadd_rn(v.x, v.y), __fadd_rn(v.z, v.w))); }
    else for (int c = lane; c < C; c += 64) s = __fadd_rn(s, xr[c]);
    const float mu = __fdiv_rn(wsum(s), (float)C);
    float q = 0.f;
    if (vec) for (int c = 4 * lane; c < C; c += 256) {
        const float4 v = *reinterpret_cast<const float4*>(xr + c);
        const float a = __fsub_rn(v.x, mu), b = __fsub_rn(v.y, mu), cc = __fsub_rn(v.z, mu), d = __fsub_rn(v.w, mu);
        q = __fadd_rn(q, __fadd_rn(__fadd_rn(__fmul_rn(a, a), __fmul_rn(b, b)), __fadd_rn(__fmul_rn(cc, cc), __fmul_rn(d, d))));
    }
    else for (int c = lane; c < C; c += 64) { const float a = __fsub_rn(xr[c], mu); q = __fadd_rn(q, __fmul_rn(a, a)); }
    const float rs = 1.f / sqrtf(__fadd_rn(__fdiv_rn(wsum(q), (float)C), eps));
    if (lane == 0) { mean[r] = mu; rstd[r] = rs; }
    if (vec) for (int c = 4 * lane; c < C; c += 256) {
        const float4 v = *reinterpret_cast<const float4*>(xr + c), g = *reinterpret_cast<const float4*>(gamma + c),
                     b = *reinterpret_cast<const float4*>(beta + c);
        float4 o;
        o.x = __fadd_rn(__fmul_rn(__fmul_rn(__fsub_rn(v.x, mu), rs), g.x), b.x);
        o.y = __fadd_rn(__fmul_rn(__fmul_rn(__fsub_rn(v.y, mu), rs), g.y), b.y);
        o.z = __fadd_rn(__fmul_rn(__fmul_rn(__fsub_rn(v.z, mu), rs), g.z), b.z);
        o.w = __fadd_rn(__fmul_rn(__fmul_rn(__fsub_rn(v.w, mu), rs), g.w), b.w);
        *reinterpret_cast<float4*>(orow + c) = o;
    }
    else for (int c = lane; c < C; c += 64) orow[c] = __fadd_rn(__fmul_rn(__fmul_rn(__fsub_rn(xr[c], mu), rs), gamma[c]), beta[c]);
}

// dx = add0 + add1 + rstd (dyg - mean(dyg) - xhat mean(dyg xhat)), dyg = dy * gamma, xhat = (x - mean) rstd.  dx may alias add0 / add1
// (each element is read and written by the same lane).
__global__ void __launch_bounds__(256) vit_layernorm_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ x, const float* __restrict__ mean,
                                                                const float* __restrict__ rstd, const float* __restrict__ gamma, int64_t rows, int C,
                                                                const float* add0, const float* add1, float* dx, int vec) {
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= rows) return;
    const float mu = mean[r], rs = rstd[r];
    const float *dyr = dy + r * C, *xr = x + r * C;
    float s1 = 0.f, s2 = 0.f;
    auto acc1 = [&](float d, float g, float xv) {
        const float dg = __fmul_rn(d, g), xh = __fmul_rn(__fsub_rn(xv, mu), rs);
        s1 = __fadd_rn(s1, dg); s2 = __fadd_rn(s2, __fmul_rn(dg, xh));
    };
    if (vec) for (int c = 4 * lane; c < C; c += 256) {
        const float4 d = *reinterpret_cast<const float4*>(dyr + c), g = *reinterpret_cast<const float4*>(gamma + c),
                     xv = *reinterpret_cast<const float4*>(xr + c);
        acc1(d.x, g.x, xv.x); acc1(d.y, g.y, xv.y); acc1(d.z, g.z, xv.z); acc1(d.w, g.w, xv.w);
    }
    else for (int c = lane; c < C; c += 64) acc1(dyr[c], gamma[c], xr[c]);
    const float m1 = __fdiv_rn(wsum(s1), (float)C), m2 = __fdiv_rn(wsum(s2), (float)C);
    auto one = [&](float d, float g, float xv) {
        const float dg = __fmul_rn(d, g), xh = __fmul_rn(__fsub_rn(xv, mu), rs);
        return __fmul_rn(rs, __fsub_rn(__fsub_rn(dg, m1), __fmul_rn(xh, m2)));
    };
    float* dxr = dx + r * C;
    const float* a0 = add0 ? add0 + r * C : nullptr;
    const float* a1 = add1 ? add1 + r * C : nullptr;
    if (vec) for (int c = 4 * lane; c < C; c += 256) {
        const float4 d = *reinterpret_cast<const float4*>(dyr + c), g = *reinterpret_cast<const float4*>(gamma + c),
                     xv = *reinterpret_cast<const float4*>(xr + c);
        float4 o = make_float4(one(d.x, g.x, xv.x), one(d.y, g.y, xv.y), one(d.z, g.z, xv.z), one(d.w, g.w, xv.w));
        if (a0) { const float4 u = *reinterpret_cast<const float4*>(a0 + c); o.x = __fadd_rn(u.x, o.x); o.y = __fadd_rn(u.y, o.y); o.z = __fadd_rn(u.z, o.z); o.w = __fadd_rn(u.w, o.w); }
        if (a1) { const float4 u = *reinterpret_cast<const float4*>(a1 + c); o.x = __fadd_rn(o.x, u.x); o.y = __fadd_rn(o.y, u.y); o.z = __fadd_rn(o.z, u.z); o.w = __fadd_rn(o.w, u.w); }
        *reinterpret_cast<float4*>(dxr + c) = o;
    }
    else for (int c = lane; c < C; c += 64) {
        float o = one(dyr[c], gamma[c], xr[c]);
        if (a0) o = __fadd_rn(a0[c], o);
        if (a1) o = __fadd_rn(o, a1[c]);
        dxr[c] = o;
    }
}

// one wave per row of N keys at row stride ld (ld % 4 == 0: float4 over the row, the tail element by element)
__global__ void __launch_bounds__(256) vit_softmax_kernel(float* __restrict__ X, int64_t rows, int N, int ld) {
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= rows) return;
    float* x = X + r * ld;
    const int N4 = N & ~3;
    float m = -INFINITY;
    for (int c = 4 * lane; c < N4; c += 256) { const float4 v = *reinterpret_cast<const float4*>(x + c); m = fmaxf(m, fmaxf(fmaxf(v.x, v.y), fmaxf(v.z, v.w))); }
    for (int c = N4 + lane; c < N; c += 64) m = fmaxf(m, x[c]);
    m = wmax(m);
    float s = 0.f;
    for (int c = 4 * lane; c < N4; c += 256) {
        float4 v = *reinterpret_cast<const float4*>(x + c);
        v.x = expf(__fsub_rn(v.x, m)); v.y = expf(__fsub_rn(v.y, m)); v.z = expf(__fsub_rn(v.z, m)); v.w = expf(__fsub_rn(v.w, m));
        s = __fadd_rn(s, __fadd_rn(__fadd_rn(v.x, v.y), __fadd_rn(v.z, v.w)));
        *reinterpret_cast<float4*>(x + c) = v;
    }
    for (int c = N4 + lane; c < N; c += 64) { const float e = expf(__fsub_rn(x[c], m)); x[c] = e; s = __fadd_rn(s, e); }
    const float inv = __fdiv_rn(1.f, wsum(s));
    for (int c = 4 * lane; c < N4; c += 256) {
        float4 v = *reinterpret_cast<const float4*>(x + c);
        v.x = __fmul_rn(v.x, inv); v.y = __fmul_rn(v.y, inv); v.z = __fmul_rn(v.z, inv); v.w = __fmul_rn(v.w, inv);
        *reinterpret_cast<float4*>(x + c) = v;
    }
    for (int c = N4 + lane; c < N; c += 64) x[c] = __fmul_rn(x[c], inv);
}

// dX = scale * P * (dX - sum_j dX P), in place on dX
__global__ void __launch_bounds__(256) vit_softmax_bwd_kernel(float* __restrict__ dX, const float* __restrict__ P, int64_t rows, int N, int ld,
                                                              float scale) {
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= rows) return;
    float* d = dX + r * ld;
    const float* pr = P + r * ld;
    const int N4 = N & ~3;
    float s = 0.f;
    for (int c = 4 * lane; c < N4; c += 256) {
        const float4 a = *reinterpret_cast<const float4*>(d + c), b = *reinterpret_cast<const float4*>(pr + c);
        s = __fadd_rn(s, __fadd_rn(__fadd_rn(__fmul_rn(a.x, b.x), __fmul_rn(a.y, b.y)), __fadd_rn(__fmul_rn(a.z, b.z), __fmul_rn(a.w, b.w))));
    }
    for (int c = N4 + lane; c < N; c += 64) s = __fadd_rn(s, __fmul_rn(d[c], pr[c]));
    s = wsum(s);
    for (int c = 4 * lane; c < N4; c += 256) {
        float4 a = *reinterpret_cast<const float4*>(d + c);
        const float4 b = *reinterpret_cast<const float4*>(pr + c);
        a.x = __fmul_rn(scale, __fmul_rn(b.x, __fsub_rn(a.x, s))); a.y = __fmul_rn(scale, __fmul_rn(b.y, __fsub_rn(a.y, s)));
        a.z = __fmul_rn(scale, __fmul_rn(b.z, __fsub_rn(a.z, s))); a.w = __fmul_rn(scale, __fmul_rn(b.w, __fsub_rn(a.w, s)));
        *reinterpret_cast<float4*>(d + c) = a;
    }
    for (int c = N4 + lane; c < N; c += 64) d[c] = __fmul_rn(scale, __fmul_rn(pr[c], __fsub_rn(d[c], s)));
}

// image (F, Cin, gh*P, gw*P) <-> patch rows (F*gh*gw, Cin*P*P), row = (f, py, px), column = (c, ky, kx) as the conv weight flattens.
// One thread per four consecutive kx (P % 4 == 0).
__global__ void __launch_bounds__(256) vit_patchify_kernel(const float* __restrict__ img, float* __restrict__ out, int F, int Cin, int gh, int gw,
                                                           int P, float* __restrict__ gimg, int accumulate) {
    const int q = P / 4;
    const int64_t total = (int64_t)F * gh * gw * Cin * P * q;
    const int W = gw * P, H = gh * P;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
        int64_t rest = e;
        const int kx4 = (int)(rest % q); rest /= q;
        const int ky = (int)(rest % P); rest /= P;
        const int c = (int)(rest % Cin); rest /= Cin;
        const int px = (int)(rest % gw); rest /= gw;
        const int py = (int)(rest % gh); rest /= gh;
        const int f = (int)rest;
        const int64_t pix = (((int64_t)f * Cin + c) * H + py * P + ky) * W + px * P + kx4 * 4;
        const int64_t col = (((int64_t)f * gh + py) * gw + px) * (Cin * P * P) + (c * P + ky) * P + kx4 * 4;
        if (gimg) {                 // backward: the patch rows' gradient back into the image (every pixel in exactly one patch)
            float4 v = *reinterpret_cast<const float4*>(out + col);
            if (accumulate) {
                const float4 o = *reinterpret_cast<const float4*>(gimg + pix);
                v.x = __fadd_rn(o.x, v.x); v.y = __fadd_rn(o.y, v.y); v.z = __fadd_rn(o.z, v.z); v.w = __fadd_rn(o.w, v.w);
            }
            *reinterpret_cast<float4*>(gimg + pix) = v;
        } else {
            *reinterpret_cast<float4*>(out + col) = *reinterpret_cast<const float4*>(img + pix);
        }
    }
}

// x[f][t][c] = (t < NP ? prefix[t][c] : E[f*(T-NP) + t-NP][c]) + pos[t][c]: NP prefix rows (cls, then a distilled model's dist token)
// ahead of the patch rows
__global__ void __launch_bounds__(256) vit_assemble_kernel(const float* __restrict__ E, const float* __restrict__ prefix, int NP,
                                                           const float* __restrict__ pos, float* __restrict__ x, int F, int T, int C) {
    const int c4n = C / 4;
    const int64_t total = (int64_t)F * T * c4n;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
        const int c = (int)(e % c4n) * 4;
        const int64_t ft = e / c4n;
        const int tt = (int)(ft % T), f = (int)(ft / T);
        const float4 a = tt < NP ? *reinterpret_cast<const float4*>(prefix + (int64_t)tt * C + c)
                                 : *reinterpret_cast<const float4*>(E + ((int64_t)f * (T - NP) + tt - NP) * C + c);
        const float4 p = *reinterpret_cast<const float4*>(pos + (int64_t)tt * C + c);
        *reinterpret_cast<float4*>(x + ft * C + c) = make_float4(__fadd_rn(a.x, p.x), __fadd_rn(a.y, p.y), __fadd_rn(a.z, p.z), __fadd_rn(a.w, p.w));
    }
}

inline bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }
inline unsigned grid_for(int64_t n) { return (unsigned)std::min<int64_t>((n + 255) / 256, 65536); }

}  // namespace

int vit_gemm(VitGemm p, hipStream_t s) {
    if (p.M <= 0 || p.N <= 0 || p.batch <= 0) return 0;
    if (p.nb_in <= 0) p.nb_in = 1;
    const bool ak = p.a_sk == 1, bk = p.b_sk == 1;
    if (!ak && p.a_sm != 1) return i2v_api_fail("vit_gemm: A must be contiguous along M or K");
    if (!bk && p.b_sn != 1) return i2v_api_fail("vit_gemm: B must be contiguous along K or N");
    if (p.mode == VIT_EPI_GELU && !p.C2) return i2v_api_fail("vit_gemm: the GELU epilogue needs its second output");
    if (p.mode == VIT_EPI_GELU_BWD && !p.H) return i2v_api_fail("vit_gemm: the GELU backward epilogue needs the pre-activation");
    const int64_t a_ld = ak ? p.a_sm : p.a_sk, b_ld = bk ? p.b_sn : p.b_sk;
    p.a_vec = al16(p.A) && a_ld % 4 == 0 && p.a_bo % 4 == 0 && p.a_bi % 4 == 0;
    p.b_vec = al16(p.B) && b_ld % 4 == 0 && p.b_bo % 4 == 0 && p.b_bi % 4 == 0;
    p.c_vec = al16(p.C) && p.c_sm % 4 == 0 && p.c_bo % 4 == 0 && p.c_bi % 4 == 0 && (!p.R || al16(p.R)) && (!p.C2 || al16(p.C2)) &&
              (!p.H || al16(p.H));
    p.bias_vec = !p.bias || al16(p.bias);
    if (p.K <= 0) return i2v_api_fail("vit_gemm: K must be positive");
    const int64_t tiles = (int64_t)((p.M + TM - 1) / TM) * ((p.N + TN - 1) / TN);
    if (tiles > 0x7fffffff || p.batch > 65535) return i2v_api_fail("vit_gemm: grid too large");
    const dim3 grid((unsigned)tiles, (unsigned)p.batch);
    if (ak && bk) hipLaunchKernelGGL((vit_gemm_kernel<true, true>), grid, dim3(256), 0, s, p);
    else if (ak) hipLaunchKernelGGL((vit_gemm_kernel<true, false>), grid, dim3(256), 0, s, p);
    else if (bk) hipLaunchKernelGGL((vit_gemm_kernel<false, true>), grid, dim3(256), 0, s, p);
    else hipLaunchKernelGGL((vit_gemm_kernel<false, false>), grid, dim3(256), 0, s, p);
    return vit_launch_check("vit_gemm");
}

int vit_layernorm(const float* x, int64_t rows, int C, const float* gamma, const float* beta, float eps, float* out, float* mean, float* rstd,
                  hipStream_t s) {
    if (rows <= 0) return 0;
    const int vec = C % 4 == 0 && al16(x) && al16(out) && al16(gamma) && al16(beta);
    hipLaunchKernelGGL(vit_layernorm_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, s, x, rows, C, gamma, beta, eps, out, mean, rstd, vec);
    return vit_launch_check("vit_layernorm");
}

int vit_layernorm_bwd(const float* dy, const float* x, const float* mean, const float* rstd, const float* gamma, int64_t rows, int C,
                      const float* add0, const float* add1, float* dx, hipStream_t s) {
    if (rows <= 0) return 0;
    const int vec = C % 4 == 0 && al16(dy) && al16(x) && al16(gamma) && al16(dx) && (!add0 || al16(add0)) && (!add1 || al16(add1));
    hipLaunchKernelGGL(vit_layernorm_bwd_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, s, dy, x, mean, rstd, gamma, rows, C, add0, add1,
                       dx, vec);
    return vit_launch_check("vit_layernorm_bwd");
}

int vit_softmax(float* X, int64_t rows, int N, int ld, hipStream_t s) {
    if (rows <= 0) return 0;
    if (ld % 4 != 0 || ld < N || !al16(X)) return i2v_api_fail("vit_softmax: rows must be 16-byte aligned (ld % 4 == 0, ld >= N)");
    hipLaunchKernelGGL(vit_softmax_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, s, X, rows, N, ld);
    return vit_launch_check("vit_softmax");
}

int vit_softmax_bwd(float* dX, const float* P, int64_t rows, int N, int ld, float scale, hipStream_t s) {
    if (rows <= 0) return 0;
    if (ld % 4 != 0 || ld < N || !al16(dX) || !al16(P)) return i2v_api_fail("vit_softmax_bwd: rows must be 16-byte aligned (ld % 4 == 0, ld >= N)");
    hipLaunchKernelGGL(vit_softmax_bwd_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, s, dX, P, rows, N, ld, scale);
    return vit_launch_check("vit_softmax_bwd");
}

int vit_patchify(const float* img, float* patches, int F, int Cin, int gh, int gw, int P, float* gimg, int accumulate, hipStream_t s) {
    if (P % 4 != 0 || !al16(patches) || !al16(gimg ? gimg : img)) return i2v_api_fail("vit_patchify: patch size % 4 and 16-byte alignment needed");
    const int64_t n = (int64_t)F * gh * gw * Cin * P * (P / 4);
    if (n <= 0) return 0;
    hipLaunchKernelGGL(vit_patchify_kernel, dim3(grid_for(n)), dim3(256), 0, s, img, patches, F, Cin, gh, gw, P, gimg, accumulate);
    return vit_launch_check("vit_patchify");
}

int vit_assemble(const float* E, const float* prefix, int n_prefix, const float* pos, float* x, int F, int T, int C, hipStream_t s) {
    if (n_prefix < 1 || n_prefix >= T) return i2v_api_fail("vit_assemble: the prefix tokens must leave at least one patch row");
    if (C % 4 != 0 || !al16(E) || !al16(prefix) || !al16(pos) || !al16(x)) return i2v_api_fail("vit_assemble: C % 4 and 16-byte alignment needed");
    const int64_t n = (int64_t)F * T * (C / 4);
    if (n <= 0) return 0;
    hipLaunchKernelGGL(vit_assemble_kernel, dim3(grid_for(n)), dim3(256), 0, s, E, prefix, n_prefix, pos, x, F, T, C);
    return vit_launch_check("vit_assemble");
}

int vit_launch_check(const char* what) {
    const hipError_t e = hipGetLastError();
    if (e == hipSuccess) return 0;
    char buf[256];
    snprintf(buf, sizeof buf, "%s: %s", what, hipGetErrorString(e));
    return i2v_api_fail(buf);
}
