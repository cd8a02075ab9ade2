// The PiT launches for gfx950 (i2v_pit_kernels.h): streaming attention for sequences of any length, forward with the row log-sum-exp and
// input gradient; the depthwise pooling convolution between PiT's stages, token-major, forward and input gradient; the overlapping patch
// gather and its transpose.
//
// STREAMING ATTENTION.  Heads up to 64 wide, any T.  A workgroup is 4 waves and owns one (frame, head, tile of 64 rows): wave w owns the
// rows 16 w .. 16 w + 15 of the tile, kept in registers as MFMA operands for the whole launch, and the OTHER side streams through LDS in
// tiles of 64 rows.  The kernels are compiled per KC = ceil(dh / 16) in 1 .. 4 (the width of the staged tile, of the operand arrays and of
// the output accumulators): no register array is sized or updated under a run-time condition.  Columns past dh and rows past T are zero
// operands in LDS and in registers, never in memory: every load is issued unconditionally at a clamped, valid address and masked after.
// LDS LAYOUT (chosen): two tiles (K and V; or q and dout) of 64 rows x 16 KC columns at row stride 16 KC + 4 floats, single-buffered, the
// next tile prefetched into registers (KC quads per thread and matrix) while the current one is consumed, written between two barriers.
// 34 816 B at KC = 4 (+ 512 B of row statistics in the dk / dv launch).  The fp32 MFMA (v_mfma_f32_16x16x4_f32) forms every product.  As
// in i2v_beit.hip a wave forms the TRANSPOSED score tile of its 16 rows against 16 staged rows (A from the LDS rows, B from the wave's
// rows): lane (r, g) then holds [staged row 16 nt + 4 g + i][own row r] in register i of accumulator nt, which is already the A operand
// of the next product over the staged rows -- the probabilities never touch LDS.
//   FORWARD, grid (query tiles, heads, frames): per key tile  S^T = K q^T, s = S scale (keys past T: -inf), tile maximum, m' = max(m, .),
//     alpha = exp(m - m'), p = exp(s - m'), l = l alpha + rowsum(p), out = out alpha + p v.  The output is rescaled in EVERY tile: where
//     the maximum has not moved alpha is exp(0) = 1 exactly, so this is "rescale when the maximum moves" without a branch and without a
//     threshold.  A row's m, l live on the lanes r, r + 16, r + 32, r + 48; the accumulator rows are 4 g + i, so alpha (and at the end l)
//     reach them by a lane read from lane 4 g + i.  At the end out = out / l and lse = m + log(l).
//   BACKWARD, three launches:
//     0. delta = rowsum(dout o out), one thread per (frame, head, token).
//     1. dq, same ownership as the forward, streaming K and V: P^T = exp(scale K q^T - lse), dP^T = V dout^T,
//        dS = scale P (dP - delta), dq += dS k.  No row reduction: the statistics come from lse and delta.
//     2. dk / dv, grid (KEY tiles, heads, frames): the wave's 16 key rows of K and V are its register operands and the q and dout rows
//        stream through LDS in increasing order with their lse and delta: S = q k^T and dP = dout v^T with [query 16 nt + 4 g + i][key r],
//        dv += P^T dout, dk += dS^T q, the accumulators live across the whole walk.
//     7 products for the algorithm's 5 (S and dP are formed twice).
// ORDER OF EVERY SUM (include/i2v_pit.h states it; -ffp-contract=off):
//   * an element of q k^T or dout v^T is one fp32 fma chain from 0 over the head index in chunks of 16, inside a chunk in the order
//     0 4 8 12 | 1 5 9 13 | 2 6 10 14 | 3 7 11 15 -- the same chain in all three launches that form it; then one product with the scale;
//   * per key tile of 64 the tile maximum and rowsum(p): lane group g takes its keys 16 nt + 4 g + i in increasing order (nt, then i),
//     then a butterfly over lane distances 16 and 32; m, l and out are updated once per tile, tiles in increasing order;
//   * inside a tile an element of p v, dS k, P^T dout or dS^T q adds its 64 staged rows to the running accumulator in the order
//     16 nt + {0 4 8 12 | 1 5 9 13 | 2 6 10 14 | 3 7 11 15}, nt increasing; the tiles come in increasing order;
//   * delta: one fma chain from 0 over the head index in the order of the first item.
// Nothing depends on the grid; a workgroup reads its own frame and head only; every output element has one owner, no atomics, no sum split
// across workgroups, vector-unit stores only: reruns repeat the bits and frame 0 of an n-frame call has the bits of a 1-frame call.
//
// POOL and PATCH launches: one thread per output element (pool forward: per input channel, its two output channels), grid-stride, the
// taps / patches in the fixed order i2v_pit_kernels.h states.
#include <algorithm>

#include "i2v_be.h"
#include "i2v_pit_kernels.h"
#include "i2v_vit_kernels.h"     // vit_launch_check

long long g_stat_pit = 0;

namespace {

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

constexpr int TR = 64, NT = TR / 16;                     // rows of a staged tile; its 16-row sub-tiles
template <int KC> constexpr int ldm() { return 16 * KC + 4; }
static_assert(TR == PIT_QT && TR == PIT_KT, "one tile size for the owned and the staged side");

// rows row0 .. row0 + 64 of X (row stride sx), columns 0 .. 16 KC, into registers: thread t takes the quads t, t + 256, ...; zero past T and dh
template <int KC>
__device__ __forceinline__ void load_tile(const float* __restrict__ X, int64_t sx, int row0, int T, int dh, float4 (&v)[KC]) {
#pragma unroll
    for (int j = 0; j < KC; ++j) {
        const int e = j * 256 + (int)threadIdx.x, row = row0 + e / (4 * KC), c = 4 * (e % (4 * KC));
        v[j] = keep4(ld4(X + (int64_t)min(row, T - 1) * sx + min(c, dh - 4)), row < T && c < dh);      // (dh % 4 == 0: a quad is whole or absent)
    }
}
template <int KC>
__device__ __forceinline__ void write_tile(float* tile, const float4 (&v)[KC]) {
#pragma unroll
    for (int j = 0; j < KC; ++j) {
        const int e = j * 256 + (int)threadIdx.x;
        *reinterpret_cast<float4*>(tile + (e / (4 * KC)) * ldm<KC>() + 4 * (e % (4 * KC))) = v[j];
    }
}

// this lane's operand quads of row `row` of X (a row past T: zeros): x[kc] = columns 16 kc + 4 g .. + 3
template <int KC>
__device__ __forceinline__ void row_frag(const float* X, int64_t sx, int row, int T, int dh, float4 (&x)[KC]) {
    const int g = (threadIdx.x >> 4) & 3;
    const float* p = X + (int64_t)min(row, T - 1) * sx;
#pragma unroll
    for (int kc = 0; kc < KC; ++kc) {
        const int c = 16 * kc + 4 * g;
        x[kc] = keep4(ld4(p + min(c, dh - 4)), row < T && c < dh);
    }
}

// acc[nt][i] = (M X^T)[row 16 nt + 4 g + i of M][row r of X]: M the staged tile, X the wave's 16 rows as row_frag leaves them
template <int KC>
__device__ __forceinline__ void m_times_rows_t(const float4 (&x)[KC], const float* M, f32x4 (&acc)[NT]) {
    const int r = threadIdx.x & 15, g = (threadIdx.x >> 4) & 3;
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
        acc[nt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int kc = 0; kc < KC; ++kc) acc[nt] = mfma4(ld4(M + (16 * nt + r) * ldm<KC>() + 16 * kc + 4 * g), x[kc], acc[nt]);
    }
}

// o[dt][i] += (P M)[own row 4 g + i][column 16 dt + r]: P^T in registers as m_times_rows_t lays it out, M the staged tile.  MFMA i of
// sub-tile nt takes the staged rows 16 nt + 4 g' + i in its four k-slots g'; the KC column tiles are independent chains
template <int KC>
__device__ __forceinline__ void p_times_m(const f32x4 (&p)[NT], const float* M, f32x4 (&o)[KC]) {
    const int r = threadIdx.x & 15, g = (threadIdx.x >> 4) & 3;
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float* b = M + (16 * nt + 4 * g + i) * ldm<KC>() + r;
#pragma unroll
            for (int dt = 0; dt < KC; ++dt) o[dt] = __builtin_amdgcn_mfma_f32_16x16x4f32(p[nt][i], b[16 * dt], o[dt], 0, 0, 0);
        }
}

// rows q0 .. q0 + 16 of dst (row stride ld), columns 0 .. dh
template <int KC>
__device__ __forceinline__ void store_rows(const f32x4 (&o)[KC], float* dst, int64_t ld, int q0, int T, int dh) {
    const int r = threadIdx.x & 15, g = (threadIdx.x >> 4) & 3;
#pragma unroll
    for (int dt = 0; dt < KC; ++dt) {
        const int col = 16 * dt + r;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int t = q0 + 4 * g + i;
            if (t < T && col < dh) dst[(int64_t)t * ld + col] = o[dt][i];
        }
    }
}

template <int KC>
__global__ void __launch_bounds__(256) pit_attn_fwd_kernel(const PitAttn p) {
    __shared__ __attribute__((aligned(16))) float lds[2 * TR * ldm<KC>()];
    float *Ks = lds, *Vs = lds + TR * ldm<KC>();
    const int h = blockIdx.y, f = blockIdx.z, T = p.T, dh = p.dh, C = p.H * dh;
    const int wave = threadIdx.x >> 6, r = threadIdx.x & 15, g = (threadIdx.x >> 4) & 3, q0 = TR * (int)blockIdx.x + 16 * wave;
    const float* qkv = p.qkv + (int64_t)f * T * 3 * C + h * dh;
    const int NKT = (T + TR - 1) / TR;
    float4 xq[KC], pk[KC], pv[KC];
    row_frag<KC>(qkv, 3 * C, q0 + r, T, dh, xq);
    load_tile<KC>(qkv + C, 3 * C, 0, T, dh, pk);
    load_tile<KC>(qkv + 2 * C, 3 * C, 0, T, dh, pv);
    write_tile<KC>(Ks, pk);
    write_tile<KC>(Vs, pv);
    __syncthreads();
    float m = -INFINITY, l = 0.f;
    f32x4 o[KC];
#pragma unroll
    for (int dt = 0; dt < KC; ++dt) o[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int kt = 0; kt < NKT; ++kt) {
        const int nxt = TR * min(kt + 1, NKT - 1);                         // (the last pass stages its own tile once more: unconditional loads)
        load_tile<KC>(qkv + C, 3 * C, nxt, T, dh, pk);
        load_tile<KC>(qkv + 2 * C, 3 * C, nxt, T, dh, pv);
        f32x4 acc[NT];
        m_times_rows_t<KC>(xq, Ks, acc);
        float tm = -INFINITY;
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float s = acc[nt][i] * p.scale;
                acc[nt][i] = TR * kt + 16 * nt + 4 * g + i < T ? s : -INFINITY;
                tm = fmaxf(tm, acc[nt][i]);
            }
        tm = quad_max(tm);                                                 // (every tile has a real key: finite)
        const float mn = fmaxf(m, tm), alpha = expf(m - mn);               // (first tile: exp(-inf) = 0 against l = 0 and out = 0)
        float ts = 0.f;
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                acc[nt][i] = expf(acc[nt][i] - mn);
                ts = ts + acc[nt][i];
            }
        ts = quad_sum(ts);
        l = l * alpha + ts;
        m = mn;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float a = __shfl(alpha, 4 * g + i);                      // row 4 g + i's factor lives on lane 4 g + i
#pragma unroll
            for (int dt = 0; dt < KC; ++dt) o[dt][i] = o[dt][i] * a;
        }
        p_times_m<KC>(acc, Vs, o);
        __syncthreads();
        write_tile<KC>(Ks, pk);
        write_tile<KC>(Vs, pv);
        __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const float li = __shfl(l, 4 * g + i);
#pragma unroll
        for (int dt = 0; dt < KC; ++dt) o[dt][i] = o[dt][i] / li;
    }
    store_rows<KC>(o, p.out + (int64_t)f * T * C + h * dh, C, q0, T, dh);
    if (g == 0 && q0 + r < T) p.lse[((int64_t)f * p.H + h) * T + q0 + r] = m + logf(l);
}

template <int KC>
__global__ void __launch_bounds__(256) pit_attn_dq_kernel(const PitAttn p) {
    __shared__ __attribute__((aligned(16))) float lds[2 * TR * ldm<KC>()];
    float *Ks = lds, *Vs = lds + TR * ldm<KC>();
    const int h = blockIdx.y, f = blockIdx.z, T = p.T, dh = p.dh, C = p.H * dh;
    const int wave = threadIdx.x >> 6, r = threadIdx.x & 15, g = (threadIdx.x >> 4) & 3, q0 = TR * (int)blockIdx.x + 16 * wave;
    const float* qkv = p.qkv + (int64_t)f * T * 3 * C + h * dh;
    const int NKT = (T + TR - 1) / TR;
    float4 xq[KC], xg[KC], pk[KC], pv[KC];
    row_frag<KC>(qkv, 3 * C, q0 + r, T, dh, xq);
    row_frag<KC>(p.dout + (int64_t)f * T * C + h * dh, C, q0 + r, T, dh, xg);
    const int64_t st = ((int64_t)f * p.H + h) * T + min(q0 + r, T - 1);
    const float lse = p.lse[st], delta = p.delta[st];
    load_tile<KC>(qkv + C, 3 * C, 0, T, dh, pk);
    load_tile<KC>(qkv + 2 * C, 3 * C, 0, T, dh, pv);
    write_tile<KC>(Ks, pk);
    write_tile<KC>(Vs, pv);
    __syncthreads();
    f32x4 o[KC];
#pragma unroll
    for (int dt = 0; dt < KC; ++dt) o[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int kt = 0; kt < NKT; ++kt) {
        const int nxt = TR * min(kt + 1, NKT - 1);
        load_tile<KC>(qkv + C, 3 * C, nxt, T, dh, pk);
        load_tile<KC>(qkv + 2 * C, 3 * C, nxt, T, dh, pv);
        f32x4 acc[NT], dp[NT];
        m_times_rows_t<KC>(xq, Ks, acc);
        m_times_rows_t<KC>(xg, Vs, dp);
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float P = expf(acc[nt][i] * p.scale - lse);
                const float dS = p.scale * (P * (dp[nt][i] - delta));
                dp[nt][i] = TR * kt + 16 * nt + 4 * g + i < T ? dS : 0.f;  // a key past T takes no part
            }
        p_times_m<KC>(dp, Ks, o);
        __syncthreads();
        write_tile<KC>(Ks, pk);
        write_tile<KC>(Vs, pv);
        __syncthreads();
    }
    store_rows<KC>(o, p.dqkv + (int64_t)f * T * 3 * C + h * dh, 3 * C, q0, T, dh);
}

template <int KC>
__global__ void __launch_bounds__(256) pit_attn_dkv_kernel(const PitAttn p) {
    __shared__ __attribute__((aligned(16))) float lds[2 * TR * ldm<KC>() + 2 * TR];
    float *Qs = lds, *Gs = lds + TR * ldm<KC>(), *St = lds + 2 * TR * ldm<KC>();      // St: [lse | delta] of the staged queries
    const int h = blockIdx.y, f = blockIdx.z, T = p.T, dh = p.dh, C = p.H * dh;
    const int wave = threadIdx.x >> 6, r = threadIdx.x & 15, g = (threadIdx.x >> 4) & 3, k0 = TR * (int)blockIdx.x + 16 * wave;
    const float* qkv = p.qkv + (int64_t)f * T * 3 * C + h * dh;
    const float* dout = p.dout + (int64_t)f * T * C + h * dh;
    const float* stat = ((threadIdx.x >> 6) & 1 ? p.delta : p.lse) + ((int64_t)f * p.H + h) * T;      // threads 0..63 lse, 64..127 delta (128.. again, not written)
    const int NQT = (T + TR - 1) / TR;
    float4 xk[KC], xv[KC], pq[KC], pg[KC];
    row_frag<KC>(qkv + C, 3 * C, k0 + r, T, dh, xk);
    row_frag<KC>(qkv + 2 * C, 3 * C, k0 + r, T, dh, xv);
    load_tile<KC>(qkv, 3 * C, 0, T, dh, pq);
    load_tile<KC>(dout, C, 0, T, dh, pg);
    float ps = stat[min((int)(threadIdx.x & 63), T - 1)];
    write_tile<KC>(Qs, pq);
    write_tile<KC>(Gs, pg);
    if (threadIdx.x < 2 * TR) St[threadIdx.x] = ps;
    __syncthreads();
    f32x4 aK[KC], aV[KC];
#pragma unroll
    for (int dt = 0; dt < KC; ++dt) aK[dt] = aV[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int qt = 0; qt < NQT; ++qt) {                                     // ALL the queries, in increasing order
        const int nxt = TR * min(qt + 1, NQT - 1);
        load_tile<KC>(qkv, 3 * C, nxt, T, dh, pq);
        load_tile<KC>(dout, C, nxt, T, dh, pg);
        ps = stat[min(nxt + (int)(threadIdx.x & 63), T - 1)];
        f32x4 acc[NT], dp[NT];
        m_times_rows_t<KC>(xk, Qs, acc);
        m_times_rows_t<KC>(xv, Gs, dp);
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int j = 16 * nt + 4 * g + i;
                const bool ok = TR * qt + j < T;                           // a query past T takes no part
                const float P = expf(acc[nt][i] * p.scale - St[j]);
                const float dS = p.scale * (P * (dp[nt][i] - St[TR + j]));
                acc[nt][i] = ok ? P : 0.f;
                dp[nt][i] = ok ? dS : 0.f;
            }
        p_times_m<KC>(acc, Gs, aV);
        p_times_m<KC>(dp, Qs, aK);
        __syncthreads();
        write_tile<KC>(Qs, pq);
        write_tile<KC>(Gs, pg);
        if (threadIdx.x < 2 * TR) St[threadIdx.x] = ps;
        __syncthreads();
    }
    float* dk = p.dqkv + (int64_t)f * T * 3 * C + C + h * dh;
    store_rows<KC>(aK, dk, 3 * C, k0, T, dh);
    store_rows<KC>(aV, dk + C, 3 * C, k0, T, dh);
}

// delta[f][h][t] = sum over the head index of dout o out, in the order of the score chain
__global__ void __launch_bounds__(256) pit_attn_delta_kernel(const PitAttn p) {
    const int T = p.T, dh = p.dh, H = p.H, C = H * dh;
    const int64_t n = (int64_t)p.F * H * T;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < n; e += (int64_t)gridDim.x * 256) {
        const int t = (int)(e % T), h = (int)((e / T) % H);
        const int64_t f = e / ((int64_t)T * H), at = (f * T + t) * C + h * dh;
        float acc = 0.f;
        for (int c0 = 0; c0 < dh; c0 += 16) {
            float a[16], b[16];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int c = c0 + 4 * q;
                const float4 va = keep4(ld4(p.dout + at + min(c, dh - 4)), c < dh), vb = keep4(ld4(p.out + at + min(c, dh - 4)), c < dh);
                a[4 * q] = va.x; a[4 * q + 1] = va.y; a[4 * q + 2] = va.z; a[4 * q + 3] = va.w;
                b[4 * q] = vb.x; b[4 * q + 1] = vb.y; b[4 * q + 2] = vb.z; b[4 * q + 3] = vb.w;
            }
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int q = 0; q < 4; ++q) acc = fmaf(a[4 * q + j], b[4 * q + j], acc);
        }
        p.delta[e] = acc;
    }
}

__global__ void __launch_bounds__(256) pit_pool_kernel(const PitPool p) {
    const int g = p.g, C = p.C, go = (g - 1) / 2 + 1;
    const int64_t n = (int64_t)p.F * go * go * C;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < n; e += (int64_t)gridDim.x * 256) {
        const int c = (int)(e % C), ox = (int)((e / C) % go), oy = (int)((e / ((int64_t)C * go)) % go);
        const int64_t f = e / ((int64_t)C * go * go);
        const float* x = p.x + f * p.xs + c;
        const float *w0 = p.w + (int64_t)(2 * c) * 9, *w1 = w0 + 9;
        float a0 = p.b ? p.b[2 * c] : 0.f, a1 = p.b ? p.b[2 * c + 1] : 0.f;
#pragma unroll
        for (int ky = 0; ky < 3; ++ky)
#pragma unroll
            for (int kx = 0; kx < 3; ++kx) {
                const int iy = 2 * oy - 1 + ky, ix = 2 * ox - 1 + kx;
                const bool ok = iy >= 0 && iy < g && ix >= 0 && ix < g;
                const float v = x[(int64_t)(min(max(iy, 0), g - 1) * g + min(max(ix, 0), g - 1)) * C];
                if (ok) {                                                  // a tap on the padding takes no part
                    a0 = fmaf(w0[3 * ky + kx], v, a0);
                    a1 = fmaf(w1[3 * ky + kx], v, a1);
                }
            }
        float* y = p.y + f * p.ys + ((int64_t)oy * go + ox) * 2 * C + 2 * c;
        y[0] = a0;
        y[1] = a1;
    }
}

__global__ void __launch_bounds__(256) pit_pool_bwd_kernel(const PitPool p) {
    const int g = p.g, C = p.C, go = (g - 1) / 2 + 1;
    const int64_t n = (int64_t)p.F * g * g * C;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < n; e += (int64_t)gridDim.x * 256) {
        const int c = (int)(e % C), ix = (int)((e / C) % g), iy = (int)((e / ((int64_t)C * g)) % g);
        const int64_t f = e / ((int64_t)C * g * g);
        const float* dy = p.x + f * p.ys + 2 * c;                         // (dy is the output-side stream: ys)
        const float *w0 = p.w + (int64_t)(2 * c) * 9, *w1 = w0 + 9;
        float acc = 0.f;
#pragma unroll
        for (int ky = 0; ky < 3; ++ky)
#pragma unroll
            for (int kx = 0; kx < 3; ++kx) {
                const int ty = iy + 1 - ky, tx = ix + 1 - kx;              // 2 oy, 2 ox
                const bool ok = ty >= 0 && tx >= 0 && !(ty & 1) && !(tx & 1) && ty / 2 < go && tx / 2 < go;
                const int oy = min(max(ty, 0) / 2, go - 1), ox = min(max(tx, 0) / 2, go - 1);
                const float* d = dy + ((int64_t)oy * go + ox) * 2 * C;
                const float d0 = d[0], d1 = d[1];
                if (ok) {
                    acc = fmaf(w0[3 * ky + kx], d0, acc);
                    acc = fmaf(w1[3 * ky + kx], d1, acc);
                }
            }
        float* dx = p.y + f * p.xs + ((int64_t)iy * g + ix) * C + c;
        *dx = p.accumulate ? *dx + acc : acc;
    }
}

__global__ void __launch_bounds__(256) pit_patch_gather_kernel(const PitPatch p) {
    const int P = p.p, S = p.s, side = p.side, g = (side - P) / S + 1, KP = p.Cin * P * P;
    const int64_t n = (int64_t)p.F * g * g * KP;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < n; e += (int64_t)gridDim.x * 256) {
        const int col = (int)(e % KP), dx = col % P, dy = (col / P) % P, c = col / (P * P);
        const int64_t row = e / KP;
        const int px = (int)(row % g), py = (int)((row / g) % g);
        const int64_t f = row / ((int64_t)g * g);
        p.dst[e] = p.src[((f * p.Cin + c) * side + py * S + dy) * side + px * S + dx];
    }
}

__global__ void __launch_bounds__(256) pit_patch_scatter_kernel(const PitPatch p) {
    const int P = p.p, S = p.s, side = p.side, g = (side - P) / S + 1, KP = p.Cin * P * P;
    const int64_t n = (int64_t)p.F * p.Cin * side * side;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < n; e += (int64_t)gridDim.x * 256) {
        const int x = (int)(e % side), y = (int)((e / side) % side), c = (int)((e / ((int64_t)side * side)) % p.Cin);
        const int64_t f = e / ((int64_t)side * side * p.Cin);
        const int py0 = max(0, (y - P + S) / S), py1 = min(g - 1, y / S), px0 = max(0, (x - P + S) / S), px1 = min(g - 1, x / S);      // (y - P + S >= 0 or the range is clipped at 0: S <= P)
        float acc = 0.f;
        for (int py = py0; py <= py1; ++py)
            for (int px = px0; px <= px1; ++px)
                acc = acc + p.src[((f * g + py) * g + px) * KP + (c * P + (y - py * S)) * P + (x - px * S)];
        p.dst[e] = p.accumulate ? p.dst[e] + acc : acc;
    }
}

int refuse(const char* who, const char* why) {
    char buf[256];
    snprintf(buf, sizeof buf, "%s: %s: %s", who, hipGetErrorName(hipErrorInvalidValue), why);
    return i2v_api_fail(buf);
}

unsigned blocks_for(int64_t n) { return (unsigned)std::min<int64_t>((n + 255) / 256, 65535); }

// which: 0 forward, 1 dq, 2 dk / dv
template <int KC>
void launch(int which, const PitAttn& p, hipStream_t s) {
    const dim3 grid((unsigned)((p.T + TR - 1) / TR), (unsigned)p.H, (unsigned)p.F);
    if (which == 0) hipLaunchKernelGGL(pit_attn_fwd_kernel<KC>, grid, dim3(256), 0, s, p);
    else if (which == 1) hipLaunchKernelGGL(pit_attn_dq_kernel<KC>, grid, dim3(256), 0, s, p);
    else hipLaunchKernelGGL(pit_attn_dkv_kernel<KC>, grid, dim3(256), 0, s, p);
}

void launch_for(int which, const PitAttn& p, hipStream_t s) {
    switch ((p.dh + 15) / 16) {
        case 1: return launch<1>(which, p, s);
        case 2: return launch<2>(which, p, s);
        case 3: return launch<3>(which, p, s);
        default: return launch<4>(which, p, s);
    }
}

}  // namespace

int pit_attention(const PitAttn& p, hipStream_t s) {
    const char* who = "pit_attention";
    if (const char* why = pit_attn_refusal(p, false)) return refuse(who, why);
    launch_for(0, p, s);
    __atomic_fetch_add(&g_stat_pit, 1, __ATOMIC_RELAXED);
    return vit_launch_check(who);
}

int pit_attention_bwd(const PitAttn& p, hipStream_t s) {
    const char* who = "pit_attention_bwd";
    if (const char* why = pit_attn_refusal(p, true)) return refuse(who, why);
    hipLaunchKernelGGL(pit_attn_delta_kernel, dim3(blocks_for((int64_t)p.F * p.H * p.T)), dim3(256), 0, s, p);
    launch_for(1, p, s);
    launch_for(2, p, s);
    __atomic_fetch_add(&g_stat_pit, 3, __ATOMIC_RELAXED);
    return vit_launch_check(who);
}

int pit_pool(const PitPool& p, hipStream_t s) {
    if (const char* why = pit_pool_refusal(p)) return refuse("pit_pool", why);
    const int64_t go = (p.g - 1) / 2 + 1;
    hipLaunchKernelGGL(pit_pool_kernel, dim3(blocks_for(p.F * go * go * p.C)), dim3(256), 0, s, p);
    return vit_launch_check("pit_pool");
}

int pit_pool_bwd(const PitPool& p, hipStream_t s) {
    if (const char* why = pit_pool_refusal(p)) return refuse("pit_pool_bwd", why);
    hipLaunchKernelGGL(pit_pool_bwd_kernel, dim3(blocks_for((int64_t)p.F * p.g * p.g * p.C)), dim3(256), 0, s, p);
    return vit_launch_check("pit_pool_bwd");
}

int pit_patch_gather(const PitPatch& p, hipStream_t s) {
    if (const char* why = pit_patch_refusal(p)) return refuse("pit_patch_gather", why);
    const int64_t g = (p.side - p.p) / p.s + 1;
    hipLaunchKernelGGL(pit_patch_gather_kernel, dim3(blocks_for(p.F * g * g * p.Cin * p.p * p.p)), dim3(256), 0, s, p);
    return vit_launch_check("pit_patch_gather");
}

int pit_patch_scatter(const PitPatch& p, hipStream_t s) {
    if (const char* why = pit_patch_refusal(p)) return refuse("pit_patch_scatter", why);
    hipLaunchKernelGGL(pit_patch_scatter_kernel, dim3(blocks_for((int64_t)p.F * p.Cin * p.side * p.side)), dim3(256), 0, s, p);
    return vit_launch_check("pit_patch_scatter");
}
