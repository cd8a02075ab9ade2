// The XCiT launches for gfx950 (i2v_xcit_kernels.h): cross-covariance attention (timm's `XCA`), forward and input gradient; the token-major
// depthwise 3 x 3 of the local patch interaction; and the gather / scatter pair of the stride-2 stem convolutions.
//
// CROSS-COVARIANCE ATTENTION.  One workgroup (4 waves) owns one (frame, head); the dh x dh problem never leaves it.  DP = dh rounded up to
// 16 is the width the MFMA tiles see, columns dh .. DP and tokens past T are zero operands in LDS, never in memory.  LDS holds token tiles
// of TT rows by DP + 4 floats and the DP x (DP + 4) matrices; T is bounded by nothing.
//   FORWARD, two sweeps over the tokens (TT = 64):
//     1. q and k tiles -> LDS; G = q^T k by v_mfma_f32_16x16x4_f32 in accumulators that live across the whole sweep (wave w owns the 16 x 16
//        tiles w, w + 4, ... of G, at most 4); thread c adds the squares of column c of the tile, q for c < DP and k for DP <= c < 2 DP
//     2. in LDS: nq = max(sqrt(ssq), 1e-12); Gh = G / nq[i] / nk[j] (normalised AFTER the product) -> gram; A = softmax_j(temperature Gh),
//        one wave per row -> probs and LDS
//     3. v tiles -> LDS; out = v A^T by the same MFMA, both operands float4 from LDS
//   BACKWARD, one launch, two sweeps (TT = 32):
//     1. (dout, v) tiles -> dA = dout^T v as step 1 above
//     2. in LDS, one wave per row i: dS = A (dA - sum_j dA A), dG = temperature dS, r[i] = sum_j dG Gh; then c[j] = sum_i dG Gh by thread j;
//        the matrices the second sweep multiplies by: A^T, M1[i][j] = dG[i][j] / nk[j], M2[j][i] = dG[i][j] / nq[i]
//     3. (dout, q, k) tiles -> dv = dout A, dq = (k M1^T - q r / nq) / nq, dk = (q M2^T - k c / nk) / nk
// ORDER OF EVERY SUM (include/i2v_xcit.h states it; -ffp-contract=off, every fma written out):
//   * an element of G or dA is ONE fp32 fma chain from 0 over the tokens in increasing order (the fp32 MFMA is bitwise an fmaf chain, four
//     tokens per instruction); a column's sum of squares likewise, one fmaf per token
//   * an element of out, dv, and the products inside dq and dk is one chain from 0 over the contracted head index in chunks of 16, inside a
//     chunk in the order 0 4 8 12 | 1 5 9 13 | 2 6 10 14 | 3 7 11 15
//   * a row sum (softmax denominator, sum_j dA A, r): lane j holds element j, then a butterfly over lane distances 32 .. 1; c[j] adds rows
//     in increasing order from 0;  A = exp(S - max) / sum
// A workgroup reads and writes its own frame and head only and nothing depends on the grid: reruns repeat the bits, and frame 0 of an
// n-frame call has the bits of a 1-frame call.  Every output element has one owner; no atomics; vector-unit stores only.
#include "i2v_be.h"
#include "i2v_gelu.h"
#include "i2v_vit_kernels.h"     // vit_launch_check
#include "i2v_xcit_kernels.h"

long long g_stat_xcit = 0;

namespace {

constexpr int TT_FWD = 64, TT_BWD = 32, XCIT_LDS_MAX = 160 * 1024;

__device__ __forceinline__ float xc_wsum(float v) {
    for (int o = 32; o > 0; o >>= 1) v = __fadd_rn(v, __shfl_xor(v, o));
    return v;
}
__device__ __forceinline__ float xc_wmax(float v) {
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    return v;
}

// LDS tile (TT rows, DP columns at row stride ldm) = rows t0 .. t0 + TT of X (row stride sx), columns 0 .. dh; zero past T and past dh
template <int TT>
__device__ __forceinline__ void load_tile(const float* __restrict__ X, int64_t sx, int t0, int T, int dh, int DP, int ldm, float* tile) {
    const int q4 = DP / 4;
    for (int e = threadIdx.x; e < TT * q4; e += 256) {
        const int row = e / q4, c = 4 * (e - row * q4);
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (t0 + row < T && c < dh) v = *reinterpret_cast<const float4*>(X + (int64_t)(t0 + row) * sx + c);      // (dh % 4 == 0: the quad is whole or absent)
        *reinterpret_cast<float4*>(tile + row * ldm + c) = v;
    }
}

// acc[n]: the 16 x 16 tile (wave + 4 n) of X^T Y (DP x DP, row-major over DP / 16 tiles a side), summed over all T tokens in increasing
// order.  With SSQ, thread c < DP returns the sum of squares of column c of X and thread DP <= c < 2 DP that of column c - DP of Y.
template <int TT, bool SSQ>
__device__ __forceinline__ float cov_sweep(const float* __restrict__ X, int64_t sx, const float* __restrict__ Y, int64_t sy, int T, int dh,
                                           int DP, int ldm, float* tx, float* ty, f32x4 (&acc)[4]) {
    const int wave = threadIdx.x >> 6, r = threadIdx.x & 15, g = (threadIdx.x >> 4) & 3, NT = DP / 16;
    float ssq = 0.f;
#pragma unroll
    for (int n = 0; n < 4; ++n) acc[n] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int t0 = 0; t0 < T; t0 += TT) {
        __syncthreads();                                                  // the previous tile is consumed
        load_tile<TT>(X, sx, t0, T, dh, DP, ldm, tx);
        load_tile<TT>(Y, sy, t0, T, dh, DP, ldm, ty);
        __syncthreads();
        if (SSQ && (int)threadIdx.x < 2 * DP) {
            const float* col = (int)threadIdx.x < DP ? tx + threadIdx.x : ty + (threadIdx.x - DP);
            for (int t = 0; t < TT; ++t) ssq = __builtin_fmaf(col[t * ldm], col[t * ldm], ssq);
        }
#pragma unroll
        for (int n = 0; n < 4; ++n) {
            const int tile = wave + 4 * n;
            if (tile >= NT * NT) continue;                                // (uniform over the wave)
            const float* ap = tx + g * ldm + 16 * (tile / NT) + r;        // A[m = column i of X][k = token]
            const float* bp = ty + g * ldm + 16 * (tile % NT) + r;        // B[k = token][n = column j of Y]
            for (int t = 0; t < TT; t += 4) acc[n] = __builtin_amdgcn_mfma_f32_16x16x4f32(ap[t * ldm], bp[t * ldm], acc[n], 0, 0, 0);
        }
    }
    return ssq;
}

// acc[n] -> M (DP x DP at row stride ldm): acc[n][i] is row 16 ti + 4 g + i, column 16 tj + r of tile (wave + 4 n)
__device__ __forceinline__ void cov_store(const f32x4 (&acc)[4], int DP, int ldm, float* M) {
    const int wave = threadIdx.x >> 6, r = threadIdx.x & 15, g = (threadIdx.x >> 4) & 3, NT = DP / 16;
#pragma unroll
    for (int n = 0; n < 4; ++n) {
        const int tile = wave + 4 * n;
        if (tile >= NT * NT) continue;
        float* o = M + (16 * (tile / NT) + 4 * g) * ldm + 16 * (tile % NT) + r;
#pragma unroll
        for (int i = 0; i < 4; ++i) o[i * ldm] = acc[n][i];
    }
}

// the 16 x 16 tile (sub, nt) of X M^T: X an LDS token tile, M an LDS matrix, both at row stride ldm; the contracted index runs over DP.
// acc[i]: token row 16 sub + 4 g + i, column 16 nt + r
__device__ __forceinline__ f32x4 tile_times_mt(const float* X, const float* M, int sub, int nt, int DP, int ldm) {
    const int r = threadIdx.x & 15, g = (threadIdx.x >> 4) & 3;
    const float* xp = X + (16 * sub + r) * ldm + 4 * g;
    const float* mp = M + (16 * nt + r) * ldm + 4 * g;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int k0 = 0; k0 < DP; k0 += 16) {
        const float4 a = *reinterpret_cast<const float4*>(xp + k0);
        const float4 b = *reinterpret_cast<const float4*>(mp + k0);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, b.x, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, b.y, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, b.z, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, b.w, acc, 0, 0, 0);
    }
    return acc;
}

constexpr int64_t xcit_fwd_lds(int dh) { return (int64_t)((2 * TT_FWD + xcit_dp(dh)) * (xcit_dp(dh) + 4) + 2 * xcit_dp(dh)) * 4; }
constexpr int64_t xcit_bwd_lds(int dh) { return (int64_t)((3 * TT_BWD + 4 * xcit_dp(dh)) * (xcit_dp(dh) + 4) + 4 * xcit_dp(dh)) * 4; }

__global__ void __launch_bounds__(256) xcit_attn_fwd_kernel(const XcitAttn p) {
    extern __shared__ __attribute__((aligned(16))) float xcit_lds[];
    const int h = blockIdx.x, f = blockIdx.y, T = p.T, dh = p.dh, C = p.H * dh, DP = xcit_dp(dh), ldm = DP + 4;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, r = threadIdx.x & 15, g = (threadIdx.x >> 4) & 3, NT = DP / 16;
    float* t0s = xcit_lds;                       // q, then v
    float* t1s = t0s + TT_FWD * ldm;             // k
    float* Am = t1s + TT_FWD * ldm;              // G, then A
    float* nq = Am + DP * ldm;
    float* nk = nq + DP;
    const float* qkv = p.qkv + (int64_t)f * T * 3 * C + h * dh;
    const int64_t fh = (int64_t)f * p.H + h;
    float* gram = p.gram + fh * (dh + 2) * dh;
    float* probs = p.probs + fh * dh * dh;

    f32x4 acc[4];
    const float ssq = cov_sweep<TT_FWD, true>(qkv, 3 * C, qkv + C, 3 * C, T, dh, DP, ldm, t0s, t1s, acc);
    cov_store(acc, DP, ldm, Am);
    if ((int)threadIdx.x < 2 * DP) nq[threadIdx.x] = fmaxf(sqrtf(ssq), XCIT_NORM_EPS);      // (nk follows nq)
    __syncthreads();
    if ((int)threadIdx.x < dh) {
        gram[dh * dh + threadIdx.x] = nq[threadIdx.x];
        gram[(dh + 1) * dh + threadIdx.x] = nk[threadIdx.x];
    }
    const float temp = p.temperature[h];
    for (int i = wave; i < dh; i += 4) {                                   // one wave per row of the dh x dh matrix
        const bool ok = lane < dh;
        const float gh = ok ? __fdiv_rn(__fdiv_rn(Am[i * ldm + lane], nq[i]), nk[lane]) : 0.f;
        const float s = __fmul_rn(temp, gh);
        const float m = xc_wmax(ok ? s : -INFINITY);
        const float e = ok ? expf(__fsub_rn(s, m)) : 0.f;
        const float a = __fdiv_rn(e, xc_wsum(e));
        if (ok) {
            gram[i * dh + lane] = gh;
            probs[i * dh + lane] = a;
        }
        if (lane < DP) Am[i * ldm + lane] = a;                             // (columns dh .. DP: zeros; rows dh .. DP hold the zeros of G)
    }
    float* out = p.out + (int64_t)f * T * C + h * dh;
    for (int t0 = 0; t0 < T; t0 += TT_FWD) {
        __syncthreads();                                                   // A is whole; the previous tile is consumed
        load_tile<TT_FWD>(qkv + 2 * C, 3 * C, t0, T, dh, DP, ldm, t0s);
        __syncthreads();
        for (int job = wave; job < (TT_FWD / 16) * NT; job += 4) {
            const int sub = job % (TT_FWD / 16), nt = job / (TT_FWD / 16);
            if (t0 + 16 * sub >= T) continue;                              // (uniform over the wave)
            const f32x4 o = tile_times_mt(t0s, Am, sub, nt, DP, ldm);
            const int col = 16 * nt + r;
            if (col >= dh) continue;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int t = t0 + 16 * sub + 4 * g + i;
                if (t < T) out[(int64_t)t * C + col] = o[i];
            }
        }
    }
}

__global__ void __launch_bounds__(256) xcit_attn_bwd_kernel(const XcitAttn p) {
    extern __shared__ __attribute__((aligned(16))) float xcit_lds[];
    const int h = blockIdx.x, f = blockIdx.y, T = p.T, dh = p.dh, C = p.H * dh, DP = xcit_dp(dh), ldm = DP + 4;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, r = threadIdx.x & 15, g = (threadIdx.x >> 4) & 3, NT = DP / 16;
    float* t0s = xcit_lds;                       // dout
    float* t1s = t0s + TT_BWD * ldm;             // v, then q
    float* t2s = t1s + TT_BWD * ldm;             // k
    float* M0 = t2s + TT_BWD * ldm;              // dA, then dG Gh
    float* At = M0 + DP * ldm;                   // A^T
    float* M1 = At + DP * ldm;                   // [i][j] dG[i][j] / nk[j]
    float* M2 = M1 + DP * ldm;                   // [j][i] dG[i][j] / nq[i]
    float* nq = M2 + DP * ldm;
    float* nk = nq + DP;
    float* rq = nk + DP;                         // r[i] / nq[i]
    float* ck = rq + DP;                         // c[j] / nk[j]
    const float* qkv = p.qkv + (int64_t)f * T * 3 * C + h * dh;
    const float* dout = p.dout + (int64_t)f * T * C + h * dh;
    float* dqkv = p.dqkv + (int64_t)f * T * 3 * C + h * dh;
    const int64_t fh = (int64_t)f * p.H + h;
    const float* gram = p.gram + fh * (dh + 2) * dh;
    const float* probs = p.probs + fh * dh * dh;

    for (int e = threadIdx.x; e < 3 * DP * ldm; e += 256) At[e] = 0.f;     // A^T, M1, M2: rows and columns dh .. DP stay zero
    if ((int)threadIdx.x < DP) {
        const bool ok = (int)threadIdx.x < dh;
        nq[threadIdx.x] = ok ? gram[dh * dh + threadIdx.x] : 1.f;
        nk[threadIdx.x] = ok ? gram[(dh + 1) * dh + threadIdx.x] : 1.f;
        rq[threadIdx.x] = 0.f;
        ck[threadIdx.x] = 0.f;
    }
    f32x4 acc[4];
    (void)cov_sweep<TT_BWD, false>(dout, C, qkv + 2 * C, 3 * C, T, dh, DP, ldm, t0s, t1s, acc);      // dA = dout^T v
    cov_store(acc, DP, ldm, M0);
    __syncthreads();
    const float temp = p.temperature[h];
    for (int i = wave; i < dh; i += 4) {
        const bool ok = lane < dh;
        const float a = ok ? probs[i * dh + lane] : 0.f;
        const float d = ok ? M0[i * ldm + lane] : 0.f;
        const float s = xc_wsum(__fmul_rn(d, a));
        const float dg = __fmul_rn(temp, __fmul_rn(a, __fsub_rn(d, s)));
        const float pg = ok ? __fmul_rn(dg, gram[i * dh + lane]) : 0.f;
        const float ri = xc_wsum(pg);
        if (ok) {
            M0[i * ldm + lane] = pg;
            At[lane * ldm + i] = a;
            M1[i * ldm + lane] = __fdiv_rn(dg, nk[lane]);
            M2[lane * ldm + i] = __fdiv_rn(dg, nq[i]);
        }
        if (lane == 0) rq[i] = __fdiv_rn(ri, nq[i]);
    }
    __syncthreads();
    if ((int)threadIdx.x < dh) {
        float c = 0.f;
        for (int i = 0; i < dh; ++i) c = __fadd_rn(c, M0[i * ldm + threadIdx.x]);
        ck[threadIdx.x] = __fdiv_rn(c, nk[threadIdx.x]);
    }
    for (int t0 = 0; t0 < T; t0 += TT_BWD) {
        __syncthreads();                                                   // the matrices are whole; the previous tiles are consumed
        load_tile<TT_BWD>(dout, C, t0, T, dh, DP, ldm, t0s);
        load_tile<TT_BWD>(qkv, 3 * C, t0, T, dh, DP, ldm, t1s);
        load_tile<TT_BWD>(qkv + C, 3 * C, t0, T, dh, DP, ldm, t2s);
        __syncthreads();
        constexpr int SUBS = TT_BWD / 16;
        for (int job = wave; job < 3 * SUBS * NT; job += 4) {
            const int which = job / (SUBS * NT), rem = job - which * SUBS * NT, sub = rem % SUBS, nt = rem / SUBS;
            if (t0 + 16 * sub >= T) continue;                              // (uniform over the wave)
            // which 0: dv = dout A | 1: dq from k M1^T | 2: dk from q M2^T
            const f32x4 o = tile_times_mt(which == 0 ? t0s : which == 1 ? t2s : t1s, which == 0 ? At : which == 1 ? M1 : M2, sub, nt, DP, ldm);
            const int col = 16 * nt + r;
            if (col >= dh) continue;
            const float* self = which == 1 ? t1s : t2s;                    // the tile of the operand being differentiated
            const float rc = which == 1 ? rq[col] : ck[col], nn = which == 1 ? nq[col] : nk[col];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int tl = 16 * sub + 4 * g + i, t = t0 + tl;
                if (t >= T) continue;
                float v = o[i];
                if (which) v = __fdiv_rn(__fsub_rn(v, __fmul_rn(self[tl * ldm + col], rc)), nn);
                dqkv[(int64_t)t * 3 * C + (which == 0 ? 2 * C : which == 1 ? 0 : C) + col] = v;
            }
        }
    }
}

__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }

// one thread per (frame, position, channel quad): bias, then the nine taps in increasing order, one fma each; then add; then the multiply
__global__ void __launch_bounds__(256) xcit_dw3_kernel(const XcitDw3 p) {
    const int c4n = p.C / 4;
    const int64_t total = (int64_t)p.N * p.H * p.W * c4n;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
        const int c = 4 * (int)(e % c4n);
        const int64_t pos = e / c4n;
        const int x = (int)(pos % p.W), y = (int)((pos / p.W) % p.H);
        const int64_t n = pos / ((int64_t)p.W * p.H);
        float4 acc = p.b ? ld4(p.b + c) : make_float4(0.f, 0.f, 0.f, 0.f);
        float4 ta = make_float4(0.f, 0.f, 0.f, 0.f), ts = ta;
        if (p.ta) { ta = ld4(p.ta + c); ts = ld4(p.ts + c); }
        for (int ky = 0; ky < 3; ++ky) {
            const int yy = y + ky - 1;
            if (yy < 0 || yy >= p.H) continue;
            for (int kx = 0; kx < 3; ++kx) {
                const int xx = x + kx - 1;
                if (xx < 0 || xx >= p.W) continue;
                float4 v = ld4(p.x + ((n * p.H + yy) * p.W + xx) * p.C + c);
                if (p.ta) {
                    v.x = __builtin_fmaf(ta.x, gelu_f(v.x), ts.x); v.y = __builtin_fmaf(ta.y, gelu_f(v.y), ts.y);
                    v.z = __builtin_fmaf(ta.z, gelu_f(v.z), ts.z); v.w = __builtin_fmaf(ta.w, gelu_f(v.w), ts.w);
                }
                const float4 w = ld4(p.w + (3 * ky + kx) * p.C + c);
                acc.x = __builtin_fmaf(w.x, v.x, acc.x); acc.y = __builtin_fmaf(w.y, v.y, acc.y);
                acc.z = __builtin_fmaf(w.z, v.z, acc.z); acc.w = __builtin_fmaf(w.w, v.w, acc.w);
            }
        }
        const int64_t o = pos * p.C + c;
        if (p.add) {
            const float4 a = ld4(p.add + o);
            acc.x = __fadd_rn(acc.x, a.x); acc.y = __fadd_rn(acc.y, a.y); acc.z = __fadd_rn(acc.z, a.z); acc.w = __fadd_rn(acc.w, a.w);
        }
        if (p.ma) {
            const float4 m = ld4(p.ma + c), u = ld4(p.mu + o);
            acc.x = __fmul_rn(acc.x, __fmul_rn(m.x, gelu_grad_f(u.x))); acc.y = __fmul_rn(acc.y, __fmul_rn(m.y, gelu_grad_f(u.y)));
            acc.z = __fmul_rn(acc.z, __fmul_rn(m.z, gelu_grad_f(u.z))); acc.w = __fmul_rn(acc.w, __fmul_rn(m.w, gelu_grad_f(u.w)));
        }
        *reinterpret_cast<float4*>(p.y + o) = acc;
    }
}

// one thread per element of rows (V = 1) or per channel quad of it (V = 4: token-major src with C % 4 == 0)
template <int V>
__global__ void __launch_bounds__(256) xcit_gather_kernel(const float* __restrict__ src, float* __restrict__ rows, int F, int H, int W, int C,
                                                          int nchw) {
    const int Ho = (H + 1) / 2, Wo = (W + 1) / 2, cn = C / V;
    const int64_t total = (int64_t)F * Ho * Wo * 9 * cn;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
        const int c = V * (int)(e % cn), tap = (int)((e / cn) % 9);
        const int64_t row = e / (9 * (int64_t)cn);
        const int ox = (int)(row % Wo), oy = (int)((row / Wo) % Ho);
        const int64_t f = row / ((int64_t)Wo * Ho);
        const int y = 2 * oy - 1 + tap / 3, x = 2 * ox - 1 + tap % 3;
        const bool in = y >= 0 && y < H && x >= 0 && x < W;
        float* o = rows + row * 9 * C + tap * C + c;
        if (V == 4) {
            *reinterpret_cast<float4*>(o) = in ? ld4(src + ((f * H + y) * W + x) * C + c) : make_float4(0.f, 0.f, 0.f, 0.f);
        } else {
            *o = !in ? 0.f : nchw ? src[((f * C + c) * H + y) * W + x] : src[((f * H + y) * W + x) * C + c];
        }
    }
}

// one thread per element of dst (V = 1; the image layout is walked with x fastest) or per channel quad of it (V = 4)
template <int V>
__global__ void __launch_bounds__(256) xcit_scatter_kernel(const float* __restrict__ drows, const float* __restrict__ pre, float* __restrict__ dst,
                                                           int F, int H, int W, int C, int nchw, int accumulate) {
    const int Ho = (H + 1) / 2, Wo = (W + 1) / 2, cn = C / V;
    const int64_t total = (int64_t)F * H * W * cn;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
        int c, x, y;
        int64_t f;
        if (nchw) {
            x = (int)(e % W); y = (int)((e / W) % H); c = (int)((e / ((int64_t)W * H)) % C); f = e / ((int64_t)W * H * C);
        } else {
            c = V * (int)(e % cn); x = (int)((e / cn) % W); y = (int)((e / ((int64_t)cn * W)) % H); f = e / ((int64_t)cn * W * H);
        }
        float acc[V];
#pragma unroll
        for (int i = 0; i < V; ++i) acc[i] = 0.f;
        for (int ky = 0; ky < 3; ++ky) {
            const int ty = y + 1 - ky;
            if (ty < 0 || (ty & 1) || ty / 2 >= Ho) continue;
            for (int kx = 0; kx < 3; ++kx) {
                const int tx = x + 1 - kx;
                if (tx < 0 || (tx & 1) || tx / 2 >= Wo) continue;
                const float* d = drows + ((f * Ho + ty / 2) * Wo + tx / 2) * 9 * C + (3 * ky + kx) * C + c;
                if (V == 4) {
                    const float4 v = ld4(d);
                    acc[0] = __fadd_rn(acc[0], v.x); acc[1 % V] = __fadd_rn(acc[1 % V], v.y);
                    acc[2 % V] = __fadd_rn(acc[2 % V], v.z); acc[3 % V] = __fadd_rn(acc[3 % V], v.w);
                } else {
                    acc[0] = __fadd_rn(acc[0], *d);
                }
            }
        }
        const int64_t tm = ((f * H + y) * W + x) * C + c;                  // token-major index
        if (pre) {
#pragma unroll
            for (int i = 0; i < V; ++i) acc[i] = __fmul_rn(acc[i], gelu_grad_f(pre[tm + i]));
        }
        if (V == 4) {
            *reinterpret_cast<float4*>(dst + tm) = make_float4(acc[0], acc[1 % V], acc[2 % V], acc[3 % V]);
        } else {
            float* o = dst + (nchw ? ((f * C + c) * H + y) * W + x : tm);
            *o = accumulate ? __fadd_rn(*o, acc[0]) : acc[0];
        }
    }
}

int refuse(const char* who, const char* why) {
    char buf[256];
    snprintf(buf, sizeof buf, "%s: %s: %s", who, hipGetErrorName(hipErrorInvalidValue), why);
    return i2v_api_fail(buf);
}

// the dynamic LDS limit of a kernel is raised past the default 64 KiB per launch (a host-side setting of the current device)
template <class K>
int raise_lds(K kernel, int64_t bytes, const char* who) {
    if (bytes <= 64 * 1024) return 0;
    const hipError_t e = hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, XCIT_LDS_MAX);
    if (e == hipSuccess) return 0;
    char buf[256];
    snprintf(buf, sizeof buf, "%s: hipFuncSetAttribute(MaxDynamicSharedMemorySize): %s", who, hipGetErrorString(e));
    return i2v_api_fail(buf);
}

unsigned blocks_for(int64_t n) { return (unsigned)std::min<int64_t>((n + 255) / 256, 65536); }

}  // namespace

static_assert(xcit_bwd_lds(XCIT_MAX_DH) <= XCIT_LDS_MAX && xcit_fwd_lds(XCIT_MAX_DH) <= XCIT_LDS_MAX, "the widest head must fit the LDS");

int xcit_attention(const XcitAttn& p, hipStream_t s) {
    const char* who = "xcit_attention";
    if (const char* why = xcit_attn_refusal(p, false)) return refuse(who, why);
    const int64_t lds = xcit_fwd_lds(p.dh);
    if (raise_lds(xcit_attn_fwd_kernel, lds, who)) return 1;
    __atomic_fetch_add(&g_stat_xcit, 1, __ATOMIC_RELAXED);
    hipLaunchKernelGGL(xcit_attn_fwd_kernel, dim3((unsigned)p.H, (unsigned)p.F), dim3(256), (size_t)lds, s, p);
    return vit_launch_check(who);
}

int xcit_attention_bwd(const XcitAttn& p, hipStream_t s) {
    const char* who = "xcit_attention_bwd";
    if (const char* why = xcit_attn_refusal(p, true)) return refuse(who, why);
    const int64_t lds = xcit_bwd_lds(p.dh);
    if (raise_lds(xcit_attn_bwd_kernel, lds, who)) return 1;
    __atomic_fetch_add(&g_stat_xcit, 1, __ATOMIC_RELAXED);
    hipLaunchKernelGGL(xcit_attn_bwd_kernel, dim3((unsigned)p.H, (unsigned)p.F), dim3(256), (size_t)lds, s, p);
    return vit_launch_check(who);
}

int xcit_dw3(const XcitDw3& p, hipStream_t s) {
    if (const char* why = xcit_dw3_refusal(p)) return refuse("xcit_dw3", why);
    hipLaunchKernelGGL(xcit_dw3_kernel, dim3(blocks_for((int64_t)p.N * p.H * p.W * (p.C / 4))), dim3(256), 0, s, p);
    return vit_launch_check("xcit_dw3");
}

int xcit_stem_gather(const float* src, float* rows, int F, int H, int W, int C, int nchw, hipStream_t s) {
    if (const char* why = xcit_stem_refusal(src, rows, F, H, W, C)) return refuse("xcit_stem_gather", why);
    const int64_t n = (int64_t)F * ((H + 1) / 2) * ((W + 1) / 2) * 9 * C;
    if (!nchw && C % 4 == 0)
        hipLaunchKernelGGL(xcit_gather_kernel<4>, dim3(blocks_for(n / 4)), dim3(256), 0, s, src, rows, F, H, W, C, 0);
    else
        hipLaunchKernelGGL(xcit_gather_kernel<1>, dim3(blocks_for(n)), dim3(256), 0, s, src, rows, F, H, W, C, nchw);
    return vit_launch_check("xcit_stem_gather");
}

int xcit_stem_scatter(const float* drows, const float* pre, float* dst, int F, int H, int W, int C, int nchw, int accumulate, hipStream_t s) {
    const char* why = xcit_stem_refusal(drows, dst, F, H, W, C);
    if (!why && ((uintptr_t)pre & 15)) why = "16-byte alignment needed";
    if (!why && nchw && pre) why = "the image layout takes no pre-activation";
    if (!why && !nchw && accumulate) why = "only the image layout accumulates";
    if (why) return refuse("xcit_stem_scatter", why);
    const int64_t n = (int64_t)F * H * W * C;
    if (!nchw && C % 4 == 0)
        hipLaunchKernelGGL(xcit_scatter_kernel<4>, dim3(blocks_for(n / 4)), dim3(256), 0, s, drows, pre, dst, F, H, W, C, 0, 0);
    else
        hipLaunchKernelGGL(xcit_scatter_kernel<1>, dim3(blocks_for(n)), dim3(256), 0, s, drows, pre, dst, F, H, W, C, nchw, accumulate);
    return vit_launch_check("xcit_stem_scatter");
}
