// The BEiT launches for gfx950 (i2v_beit_kernels.h): biased global attention -- timm's `beit.Attention` between its Linears,
// softmax(scale q k^T + B_h) v with a dense per-head (T, T) bias, or plain attention with a null one -- forward and input gradient, and the
// small bias-add launch of the shared-launch route.
//
// BIASED GLOBAL ATTENTION.  Up to 208 tokens, heads up to 64 wide: one head's whole K and V are staged in LDS once per workgroup, as
// 16 NT rows (NT = the number of 16-key tiles, rounded up to one of 1, 2, 4, 8, 13: the kernels are compiled per NT) of 64 columns at row
// stride 68; rows past T and columns past dh are zero operands in LDS, never in memory (a head narrower than 64 is computed at width
// 64: zero products leave a chain's bits alone).  A workgroup is 4 waves and owns one (frame, head); the fp32 MFMA
// (v_mfma_f32_16x16x4_f32) forms every product.  At T = 197 K and V take 113 152 B of the CU's 160 KB, which leaves no room for four
// waves' probability tiles -- so the probabilities NEVER TOUCH LDS: a wave forms the TRANSPOSED score tile S^T = K q^T of its 16 queries
// (A from the LDS K rows, B from the wave's q rows, read from memory straight into registers, each element once).  Lane (r, g) then
// holds S^T[key 16 nt + 4 g + i][query r] in register i of accumulator tile nt, which is already the A operand of out = P v when the four
// k-slots of MFMA i take the keys {16 nt + 4 g' + i : g' = 0..3} and B reads the matching V rows.  A softmax row is spread over a lane's
// registers and the four lanes r, r + 16, r + 32, r + 48.
//   FORWARD, grid (heads, frames): wave w takes the query tiles w, w + 4, ...: S^T in NT accumulator tiles, scale, bias, softmax in
//     registers, out = P v; nothing but out is written.  The waves do not synchronise after the staging.
//   BACKWARD, two launches, P recomputed (nothing is saved):
//     1. dq, same ownership: dP^T = V dout^T as S^T, dS = scale P (dP - rowsum(dP P)) in registers, dq = dS k (B from the K rows).
//     2. dk / dv, grid (heads, frames): the workgroup owns ALL of its (frame, head)'s key rows.  First the waves compute every query
//        row's maximum, denominator and rowsum(dP P) as launch 1 does and leave them in LDS (3 floats per query).  Then wave w owns the
//        key tiles w, w + 4, ... and walks ALL query tiles in increasing order: the 16 x 16 tile S = q k^T (A from q in memory, B from the
//        K rows) and dP likewise put lane (r, g)'s register i at [query 4 g + i][key r], the A operand of dv += P^T dout and
//        dk += dS^T q with B = the dout / q rows from memory; the accumulators (4 key tiles x 4 column tiles each) live across the
//        whole walk.  (A wave whose fourth key tile does not exist computes the last tile once more and does not store it.)
// FENCES: the products over the key tiles are straight-line code, and left alone the scheduler reads the LDS rows of all 13 tiles ahead
// of the first MFMA (past 512 registers: 113 to 139 spilled to scratch per query tile).  A scheduling fence behind every second key tile
// keeps two tiles' reads in flight over two tiles' MFMAs.
// NO REGISTER ARRAY IS UPDATED UNDER A RUN-TIME CONDITION, and every load is unconditional (a row past T or a column past dh is read at
// a clamped, valid address and then replaced by zero).  A workgroup at T = 197 is alone on its CU, one wave per SIMD, so nothing hides a
// load's latency but the wave's own other loads; and a guard such as `if (nt < NT)` around an update of 13 accumulator tiles made the
// compiler copy the tiles at every join (6 000 moves for 416 MFMAs: that build ran at a tenth of the arithmetic floor).
// ORDER OF EVERY SUM (include/i2v_beit.h states it; -ffp-contract=off):
//   * an element of q k^T or dout v^T is one fp32 fma chain from 0 over the head index in chunks of 16, inside a chunk in the order
//     0 4 8 12 | 1 5 9 13 | 2 6 10 14 | 3 7 11 15 (the fp32 MFMA is bitwise an fmaf chain) -- the same chain in both layouts; then
//     S = that * scale, then + bias
//   * a row maximum, softmax denominator or rowsum(dP P): lane group g takes its keys 16 nt + 4 g + i in increasing order (nt, then i),
//     then a butterfly over lane distances 16 and 32;  P = exp(S - max) / sum;  dS = scale (P (dP - rowsum))
//   * an element of out or dq is one chain from 0 over the key tiles in increasing order, inside a tile in the order
//     0 4 8 12 | 1 5 9 13 | 2 6 10 14 | 3 7 11 15; an element of dk or dv is one chain from 0 over ALL the query tiles in increasing
//     order, inside a tile in that same order
// Nothing depends on the grid and a workgroup reads and writes its own frame and head only: reruns repeat the bits, and frame 0 of an
// n-frame call has the bits of a 1-frame call.  Every output element has one owner; no atomics; vector-unit stores only.
#include <algorithm>

#include "i2v_be.h"
#include "i2v_beit_kernels.h"
#include "i2v_vit_kernels.h"     // vit_launch_check

long long g_stat_beit = 0;

namespace {

constexpr int LDM = BEIT_MAX_DH + 4, BT_LDS_MAX = 160 * 1024;

__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ float4 keep4(float4 v, bool ok) { return ok ? v : make_float4(0.f, 0.f, 0.f, 0.f); }
__device__ __forceinline__ float quad_sum(float v) {      // over the lanes r, r + 16, r + 32, r + 48; the same bits in all four
    v = v + __shfl_xor(v, 16);
    return v + __shfl_xor(v, 32);
}
__device__ __forceinline__ float quad_max(float v) {
    v = fmaxf(v, __shfl_xor(v, 16));
    return fmaxf(v, __shfl_xor(v, 32));
}
__device__ __forceinline__ f32x4 mfma4(float4 a, float4 b, f32x4 c) {      // four k-steps: the operands' x, y, z, w in turn
    c = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, b.x, c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, b.y, c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, b.z, c, 0, 0, 0);
    return __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, b.w, c, 0, 0, 0);
}

// LDS tile (TP rows of 64 columns at row stride LDM) = the T rows of X (row stride sx), columns 0 .. dh; zero past T and dh
__device__ __forceinline__ void stage_rows(const float* __restrict__ X, int64_t sx, int T, int TP, int dh, float* tile) {
    const int n = TP * 16;
#pragma unroll 4
    for (int e0 = 0; e0 < n; e0 += 256) {
        const int e = min(e0 + (int)threadIdx.x, n - 1);                   // (a thread past the end repeats the last quad: the same value)
        const int row = e >> 4, c = 4 * (e & 15);
        const float4 v = ld4(X + (int64_t)min(row, T - 1) * sx + min(c, dh - 4));      // (dh % 4 == 0: the quad is whole or absent)
        *reinterpret_cast<float4*>(tile + row * LDM + c) = keep4(v, row < T && c < dh);
    }
}

// this lane's operand quads of row `row` of X (row stride sx; a row past T: zeros): x[kc] = columns 16 kc + 4 g .. + 3
__device__ __forceinline__ void row_frag(const float* X, int64_t sx, int row, int T, int dh, float4 (&x)[4]) {
    const int g = (threadIdx.x >> 4) & 3;
    const float* p = X + (int64_t)min(row, T - 1) * sx;
#pragma unroll
    for (int kc = 0; kc < 4; ++kc) {
        const int c = 16 * kc + 4 * g;
        x[kc] = keep4(ld4(p + min(c, dh - 4)), row < T && c < dh);
    }
}

// this lane's bias elements, laid out as the transposed score tile: b[nt][i] = brow[16 nt + 4 g + i], brow a row of T valid floats
template <int NT>
__device__ __forceinline__ void bias_frag(const float* brow, int T, f32x4 (&b)[NT]) {
    const int g = (threadIdx.x >> 4) & 3;
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
        for (int i = 0; i < 4; ++i) b[nt][i] = brow[min(16 * nt + 4 * g + i, T - 1)];
}

// acc[nt][i] = (M X^T)[row 16 nt + 4 g + i of M][row r of X]: M an LDS tile of 16 NT rows, X the wave's 16 rows as row_frag leaves them
template <int NT>
__device__ __forceinline__ void m_times_rows_t(const float4 (&x)[4], const float* M, f32x4 (&acc)[NT]) {
    const int r = threadIdx.x & 15, g = (threadIdx.x >> 4) & 3;
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
        acc[nt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int kc = 0; kc < 4; ++kc) acc[nt] = mfma4(ld4(M + (16 * nt + r) * LDM + 16 * kc + 4 * g), x[kc], acc[nt]);
        if (nt % 2 == 1) __builtin_amdgcn_sched_barrier(0);               // (keeps the scheduler from reading every tile's rows ahead: FENCES)
    }
    __builtin_amdgcn_sched_barrier(0);
}

// the 16 x 16 tile (X M^T): [i] = [row 4 g + i of X][row r of the 16 rows of M at `mrow` = M + (16 kt + r) LDM + 4 g]: the same chain
__device__ __forceinline__ f32x4 rows_times_m_t(const float4 (&x)[4], const float* mrow) {
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int kc = 0; kc < 4; ++kc) acc = mfma4(x[kc], ld4(mrow + 16 * kc), acc);
    return acc;
}

// q k^T (as m_times_rows_t leaves it) -> P^T = softmax over the T keys of (scale S + bias), in place; keys past T get 0.
// `b`: this lane's query's bias elements (bias_frag), added where `biased`.  Leaves the row's maximum and denominator in m and l.
template <int NT>
__device__ __forceinline__ void softmax_t(f32x4 (&acc)[NT], int T, float scale, const f32x4 (&b)[NT], bool biased, float& m, float& l) {
    const int g = (threadIdx.x >> 4) & 3;
    m = -INFINITY;
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float s = acc[nt][i] * scale;
            acc[nt][i] = biased ? s + b[nt][i] : s;
            m = 16 * nt + 4 * g + i < T ? fmaxf(m, acc[nt][i]) : m;
        }
    m = quad_max(m);                                                       // (T >= 1: key 0 is real, the maximum is finite)
    l = 0.f;
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            acc[nt][i] = 16 * nt + 4 * g + i < T ? expf(acc[nt][i] - m) : 0.f;
            l = l + acc[nt][i];
        }
    l = quad_sum(l);
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) acc[nt] = f32x4{acc[nt][0] / l, acc[nt][1] / l, acc[nt][2] / l, acc[nt][3] / l};
}

// P^T, dP^T -> dS^T = scale P (dP - rowsum(dP P)) into dp; returns the rowsum
template <int NT>
__device__ __forceinline__ float softmax_bwd_t(const f32x4 (&p)[NT], f32x4 (&dp)[NT], float scale) {
    float d = 0.f;
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
        for (int i = 0; i < 4; ++i) d = d + dp[nt][i] * p[nt][i];
    d = quad_sum(d);
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
        for (int i = 0; i < 4; ++i) dp[nt][i] = scale * (p[nt][i] * (dp[nt][i] - d));
    return d;
}

// o[dt][i] = (P M)[query 4 g + i][column 16 dt + r]: P^T in registers as softmax_t leaves it, M an LDS tile of 16 NT rows.  MFMA i of key
// tile nt takes the keys 16 nt + 4 g' + i in its four k-slots g'; the four column tiles are four independent chains
template <int NT>
__device__ __forceinline__ void p_times_m(const f32x4 (&p)[NT], const float* M, f32x4 (&o)[4]) {
    const int r = threadIdx.x & 15, g = (threadIdx.x >> 4) & 3;
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) o[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float* b = M + (16 * nt + 4 * g + i) * LDM + r;
#pragma unroll
            for (int dt = 0; dt < 4; ++dt) o[dt] = __builtin_amdgcn_mfma_f32_16x16x4f32(p[nt][i], b[16 * dt], o[dt], 0, 0, 0);
            if (i == 3 && nt % 2 == 1) __builtin_amdgcn_sched_barrier(0);  // (FENCES)
        }
    __builtin_amdgcn_sched_barrier(0);
}

// rows q0 .. q0 + 16 of dst (row stride ld), columns 0 .. dh
__device__ __forceinline__ void store_rows(const f32x4 (&o)[4], float* dst, int64_t ld, int q0, int T, int dh) {
    const int r = threadIdx.x & 15, g = (threadIdx.x >> 4) & 3;
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) {
        const int col = 16 * dt + r;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int t = q0 + 4 * g + i;
            if (t < T && col < dh) dst[(int64_t)t * ld + col] = o[dt][i];
        }
    }
}

constexpr int nt_bucket(int T) { return T <= 16 ? 1 : T <= 32 ? 2 : T <= 64 ? 4 : T <= 128 ? 8 : BEIT_MAX_T / 16; }
constexpr int64_t kv_lds(int NT) { return (int64_t)2 * 16 * NT * LDM * 4; }                 // K and V
constexpr int64_t walk_lds(int NT) { return kv_lds(NT) + (int64_t)3 * 16 * NT * 4; }        // ... and three floats per query

struct Geo {
    int T, dh, C, wave, r, g;
    const float* qkv;      // q of this (frame, head); k at + C, v at + 2 C; row stride 3 C
    const float* bias;     // this head's (T, T); without a bias T valid floats that are read and not used
    bool biased;
    float *Ks, *Vs;
};

template <int NT>
__device__ __forceinline__ Geo stage(const BeitAttn& p, float* lds) {
    Geo G;
    const int h = blockIdx.x, f = blockIdx.y;
    G.T = p.T; G.dh = p.dh; G.C = p.H * p.dh;
    G.wave = threadIdx.x >> 6; G.r = threadIdx.x & 15; G.g = (threadIdx.x >> 4) & 3;
    G.qkv = p.qkv + (int64_t)f * G.T * 3 * G.C + h * G.dh;
    G.biased = p.bias != nullptr;
    G.bias = G.biased ? p.bias + (int64_t)h * G.T * G.T : nullptr;
    G.Ks = lds;
    G.Vs = lds + 16 * NT * LDM;
    stage_rows(G.qkv + G.C, 3 * G.C, G.T, 16 * NT, G.dh, G.Ks);
    stage_rows(G.qkv + 2 * G.C, 3 * G.C, G.T, 16 * NT, G.dh, G.Vs);
    __syncthreads();
    return G;
}

// P^T of query tile qt in acc, its row statistics in m and l.  A query past T is a row of zeros under the last row's bias: finite,
// never stored
template <int NT>
__device__ __forceinline__ void probs_t(const Geo& G, int qt, float scale, f32x4 (&acc)[NT], float& m, float& l) {
    const int row = 16 * qt + G.r;
    float4 x[4];
    f32x4 b[NT];
    row_frag(G.qkv, 3 * G.C, row, G.T, G.dh, x);
    // (issued ahead of the products, consumed behind them; without a bias element 0 of the frame's qkv is read T times and not used)
    bias_frag<NT>(G.biased ? G.bias + (int64_t)min(row, G.T - 1) * G.T : G.qkv, G.biased ? G.T : 1, b);
    m_times_rows_t<NT>(x, G.Ks, acc);
    softmax_t<NT>(acc, G.T, scale, b, G.biased, m, l);
}

// ... and dS^T of that tile in dp from this (frame, head)'s dout (row stride C); returns rowsum(dP P)
template <int NT>
__device__ __forceinline__ float dscores_t(const Geo& G, int qt, float scale, const float* dout, const f32x4 (&acc)[NT], f32x4 (&dp)[NT]) {
    float4 x[4];
    row_frag(dout, G.C, 16 * qt + G.r, G.T, G.dh, x);
    m_times_rows_t<NT>(x, G.Vs, dp);
    return softmax_bwd_t<NT>(acc, dp, scale);
}

// BWD = false: out = softmax(scale q k^T + bias) v.  BWD = true: dq = dS k
template <int NT, bool BWD>
__global__ void __launch_bounds__(256) beit_attn_rows_kernel(const BeitAttn p) {
    extern __shared__ __attribute__((aligned(16))) float bt_lds[];
    const Geo G = stage<NT>(p, bt_lds);
    const int f = blockIdx.y, h = blockIdx.x, NQ = (G.T + 15) / 16;
    const float* dout = BWD ? p.dout + (int64_t)f * G.T * G.C + h * G.dh : nullptr;
    float* dst = BWD ? p.dqkv + (int64_t)f * G.T * 3 * G.C + h * G.dh : p.out + (int64_t)f * G.T * G.C + h * G.dh;
    for (int qt = G.wave; qt < NQ; qt += 4) {                              // (no barrier below: K and V are only read)
        f32x4 acc[NT], o[4];
        float m, l;
        probs_t<NT>(G, qt, p.scale, acc, m, l);
        if (BWD) {
            f32x4 dp[NT];
            dscores_t<NT>(G, qt, p.scale, dout, acc, dp);
            p_times_m<NT>(dp, G.Ks, o);
        } else {
            p_times_m<NT>(acc, G.Vs, o);
        }
        store_rows(o, dst, BWD ? 3 * G.C : G.C, 16 * qt, G.T, G.dh);
    }
}

template <int NT>
__global__ void __launch_bounds__(256) beit_attn_dkv_kernel(const BeitAttn p) {
    extern __shared__ __attribute__((aligned(16))) float bt_lds[];
    const Geo G = stage<NT>(p, bt_lds);
    const int f = blockIdx.y, h = blockIdx.x, T = G.T, C = G.C, dh = G.dh, r = G.r, g = G.g, NQ = (T + 15) / 16;
    constexpr int TP = 16 * NT;
    const float* dout = p.dout + (int64_t)f * T * C + h * dh;
    float* St = G.Vs + TP * LDM;                                           // [max | denominator | rowsum(dP P)], TP each
    for (int qt = G.wave; qt < NQ; qt += 4) {
        f32x4 acc[NT], dp[NT];
        float m, l;
        probs_t<NT>(G, qt, p.scale, acc, m, l);
        const float d = dscores_t<NT>(G, qt, p.scale, dout, acc, dp);
        if (g == 0) {
            St[16 * qt + r] = m;
            St[TP + 16 * qt + r] = l;
            St[2 * TP + 16 * qt + r] = d;
        }
    }
    __syncthreads();
    f32x4 aK[4][4], aV[4][4];
#pragma unroll
    for (int n = 0; n < 4; ++n)
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) aK[n][dt] = aV[n][dt] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int NK = (T + 15) / 16;                                          // key tiles with a real key
    for (int qt = 0; qt < NQ; ++qt) {                                      // ALL the queries, in increasing order
        const int q0 = 16 * qt;
        float4 xq[4], xg[4];
        row_frag(G.qkv, 3 * C, q0 + r, T, dh, xq);
        row_frag(dout, C, q0 + r, T, dh, xg);
        float qb[4][4], gb[4][4], sm[4], sl[4], sd[4], bb[4][4];           // B operands: [i][dt] = [query q0 + 4 g + i][column 16 dt + r]
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int t = q0 + 4 * g + i, tc = min(t, T - 1);
            sm[i] = St[t]; sl[i] = St[TP + t]; sd[i] = St[2 * TP + t];
            const float* brow = G.biased ? G.bias + (int64_t)tc * T : G.qkv;
#pragma unroll
            for (int dt = 0; dt < 4; ++dt) {
                const int col = 16 * dt + r, cc = min(col, dh - 1);
                const bool ok = t < T && col < dh;
                const float qv = G.qkv[(int64_t)tc * 3 * C + cc], gv = dout[(int64_t)tc * C + cc];
                qb[i][dt] = ok ? qv : 0.f;
                gb[i][dt] = ok ? gv : 0.f;
            }
#pragma unroll
            for (int n = 0; n < 4; ++n) bb[i][n] = brow[G.biased ? min(16 * (G.wave + 4 * n) + r, T - 1) : 0];      // [i][n]: this wave's key tiles
        }
#pragma unroll
        for (int n = 0; n < 4; ++n) {
            const int kt = G.wave + 4 * n, key = 16 * kt + r;
            const int lrow = 16 * min(kt, NK - 1) + r;                     // (a key tile that does not exist: the last one again, not stored)
            const f32x4 S = rows_times_m_t(xq, G.Ks + lrow * LDM + 4 * g);
            const f32x4 dP = rows_times_m_t(xg, G.Vs + lrow * LDM + 4 * g);
            float P[4], dS[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const bool ok = q0 + 4 * g + i < T && key < T;             // a query or a key past T takes no part
                const float s0 = S[i] * p.scale, s = G.biased ? s0 + bb[i][n] : s0;
                P[i] = ok ? expf(s - sm[i]) / sl[i] : 0.f;
                dS[i] = ok ? p.scale * (P[i] * (dP[i] - sd[i])) : 0.f;
            }
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int dt = 0; dt < 4; ++dt) {
                    aV[n][dt] = __builtin_amdgcn_mfma_f32_16x16x4f32(P[i], gb[i][dt], aV[n][dt], 0, 0, 0);
                    aK[n][dt] = __builtin_amdgcn_mfma_f32_16x16x4f32(dS[i], qb[i][dt], aK[n][dt], 0, 0, 0);
                }
        }
    }
    float* dk = p.dqkv + (int64_t)f * T * 3 * C + C + h * dh;
#pragma unroll
    for (int n = 0; n < 4; ++n) {                                          // (rows at or past T are not stored: store_rows)
        store_rows(aK[n], dk, 3 * C, 16 * (G.wave + 4 * n), T, dh);
        store_rows(aV[n], dk + C, 3 * C, 16 * (G.wave + 4 * n), T, dh);
    }
}

// one thread per quad of S
__global__ void __launch_bounds__(256) beit_bias_add_kernel(float* __restrict__ S, const float* __restrict__ bias, int64_t total4, int64_t per4) {
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total4; e += (int64_t)gridDim.x * 256) {
        float4 v = ld4(S + 4 * e);
        const float4 b = ld4(bias + 4 * (e % per4));
        v.x = v.x + b.x; v.y = v.y + b.y; v.z = v.z + b.z; v.w = v.w + b.w;
        *reinterpret_cast<float4*>(S + 4 * e) = v;
    }
}

int refuse(const char* who, const char* why) {
    char buf[256];
    snprintf(buf, sizeof buf, "%s: %s: %s", who, hipGetErrorName(hipErrorInvalidValue), why);
    return i2v_api_fail(buf);
}

// the dynamic LDS limit of a kernel is raised past the default 64 KiB once per device (a host-side setting of that device), not per
// launch: the launch itself then makes no runtime call but the launch.  The NT = 8 and NT = 13 kernels need it
int raise_lds(const char* who, int which, const void* kernel) {
    static bool done[6][64] = {};      // by kernel and device ordinal; a racing second call sets the same attribute again, which is harmless
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) dev = -1;
    if (dev >= 0 && __atomic_load_n(&done[which][dev], __ATOMIC_ACQUIRE)) return 0;
    const hipError_t e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, BT_LDS_MAX);
    if (e != hipSuccess) {
        char buf[256];
        snprintf(buf, sizeof buf, "%s: hipFuncSetAttribute(MaxDynamicSharedMemorySize): %s", who, hipGetErrorString(e));
        return i2v_api_fail(buf);
    }
    if (dev >= 0) __atomic_store_n(&done[which][dev], true, __ATOMIC_RELEASE);
    return 0;
}

// which: 0 forward, 1 dq, 2 dk / dv
template <int NT>
int launch(const char* who, int which, const BeitAttn& p, hipStream_t s) {
    const dim3 grid((unsigned)p.H, (unsigned)p.F);
    const void* k = which == 0 ? (const void*)beit_attn_rows_kernel<NT, false>
                  : which == 1 ? (const void*)beit_attn_rows_kernel<NT, true> : (const void*)beit_attn_dkv_kernel<NT>;
    const int64_t lds = which == 2 ? walk_lds(NT) : kv_lds(NT);
    if (lds > 64 * 1024 && raise_lds(who, which + (NT > 8 ? 3 : 0), k)) return 1;      // (slots 0 .. 2: NT = 8; 3 .. 5: NT = 13)
    if (which == 0) hipLaunchKernelGGL((beit_attn_rows_kernel<NT, false>), grid, dim3(256), (size_t)lds, s, p);
    else if (which == 1) hipLaunchKernelGGL((beit_attn_rows_kernel<NT, true>), grid, dim3(256), (size_t)lds, s, p);
    else hipLaunchKernelGGL((beit_attn_dkv_kernel<NT>), grid, dim3(256), (size_t)lds, s, p);
    return 0;
}

int launch_for(const char* who, int which, const BeitAttn& p, hipStream_t s) {
    switch (nt_bucket(p.T)) {
        case 1: return launch<1>(who, which, p, s);
        case 2: return launch<2>(who, which, p, s);
        case 4: return launch<4>(who, which, p, s);
        case 8: return launch<8>(who, which, p, s);
        default: return launch<BEIT_MAX_T / 16>(who, which, p, s);
    }
}

}  // namespace

static_assert(walk_lds(BEIT_MAX_T / 16) <= BT_LDS_MAX, "the most tokens must fit the LDS");

int beit_attention(const BeitAttn& p, hipStream_t s) {
    const char* who = "beit_attention";
    if (const char* why = beit_attn_refusal(p, false)) return refuse(who, why);
    if (launch_for(who, 0, p, s)) return 1;
    __atomic_fetch_add(&g_stat_beit, 1, __ATOMIC_RELAXED);
    return vit_launch_check(who);
}

int beit_attention_bwd(const BeitAttn& p, hipStream_t s) {
    const char* who = "beit_attention_bwd";
    if (const char* why = beit_attn_refusal(p, true)) return refuse(who, why);
    if (launch_for(who, 1, p, s) || launch_for(who, 2, p, s)) return 1;
    __atomic_fetch_add(&g_stat_beit, 2, __ATOMIC_RELAXED);
    return vit_launch_check(who);
}

int beit_bias_add(float* S, const float* bias, int F, int64_t per_frame, hipStream_t s) {
    if (const char* why = beit_bias_add_refusal(S, bias, F, per_frame)) return refuse("beit_bias_add", why);
    const int64_t n = (int64_t)F * (per_frame / 4);
    hipLaunchKernelGGL(beit_bias_add_kernel, dim3((unsigned)std::min<int64_t>((n + 255) / 256, 65536)), dim3(256), 0, s, S, bias, n, per_frame / 4);
    return vit_launch_check("beit_bias_add");
}
