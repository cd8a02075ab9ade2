// The CoaT launches for gfx950 (i2v_coat_kernels.h): factorized attention -- a softmax DOWN the token axis of k, the dh x dh product
// G = softmax(k)^T v per head, and its application to q -- forward with G and the column statistics saved, and the input gradient; a
// token-major depthwise convolution whose window (3, 5 or 7) depends on the channel, forward and input gradient; the cell gather behind
// a class row and its inverse.
//
// FACTORIZED ATTENTION.  Heads up to 64 wide, any T.  A HEAD GROUP is the run of max(1, 64 / dh) whole heads, at most 64 contiguous
// columns of q, k or v: all loads of a group are runs of up to 256 bytes of a row, whatever dh is.  A workgroup is 4 waves.
//   REDUCE (forward and backward), grid (head groups, frames): the workgroup walks ALL tokens of its frame in tiles of 64 in increasing
//     order.  Two operands (k and v; backward q and dout), 64 tokens x the group's columns each, are staged in LDS at a row stride of 80
//     floats, the next tile prefetched into registers (4 quads per thread and operand) while the current one is consumed.  The product
//     over tokens runs on the fp32 MFMA (v_mfma_f32_16x16x4_f32): A[a][t] = e[t][a] (or q), B[t][b] = v[t][b] (or dout), 16 MFMAs of 4
//     tokens per tile.  Per head the dh x dh block is KC x KC tiles of 16 x 16, KC = ceil(dh / 16), re-based at the head's first column
//     (at dh 8 a tile holds one head in its upper left quarter; the rest is discarded -- the launch is byte-bound); the group's
//     nh KC^2 <= 16 tiles are dealt to the waves round-robin, 4 accumulators per wave whatever the shape (a slot past the last tile
//     recomputes the last one and stores nothing).  Forward, ONE sweep under an online rescale: per tile the column maxima of k
//     (thread = column x quarter of the tile, then 64 threads), alpha = exp(m - m'), e = exp(k - m') written over k in LDS with the
//     quarter sums, l = l alpha + sum, every accumulator row multiplied by its alpha (exactly 1 where the maximum has not moved), then
//     the MFMAs.  At the end gram = G / l, kstat = (m, log l).  Backward: dgram = scale q^T dout, no rescale.
//   APPLY (forward and backward), grid (token tiles of 64, head groups, frames): the group's G (backward also dG) is staged in LDS per
//     head at row stride dh + 1 (read straight and transposed); wave w owns the rows 16 w .. 16 w + 15 of the tile and, head by head,
//     loads its rows as MFMA operands straight from memory (quads at column 16 kc + 4 g of the head: inside a chunk of 16 the products
//     come in the order 0 4 8 12 1 5 9 13 ...).  Forward out = scale q G + q o E.  Backward dq = scale dout G^T + dout o E, dE = dout o q,
//     dv = Ks dG, dk = Ks o (v dG^T - c) with Ks = exp((k - max) - logsum) from kstat and c[a] = sum_b G[a][b] dG[a][b] formed by 64
//     threads from the staged matrices, b in the order of the chain v dG^T (the C ABI has no array for c; every workgroup forms the same bits).
// The kernels are compiled per KC in 1 .. 4: no register array is sized or updated under a run-time condition.  Columns past dh and
// rows past T are zero operands in registers and LDS, never in memory: every load goes to a clamped, valid address and is masked after.
// Nothing depends on the grid beyond the ownership above; every output element has one owner, no atomics, no sum split across
// workgroups, vector-unit stores only: reruns repeat the bits and frame 0 of an n-frame call has the bits of a 1-frame call.
// include/i2v_coat.h states the order of every sum (-ffp-contract=off).
//
// DWMIX and the CELL launches: one thread per 4 channels of an output row (the window groups are multiples of 4 wide, so a quad has one
// window), grid-stride, the taps in the fixed order i2v_coat_kernels.h states.
#include <algorithm>

#include "i2v_be.h"
#include "i2v_coat_kernels.h"
#include "i2v_vit_kernels.h"     // vit_launch_check

long long g_stat_coat = 0;

namespace {

__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ void st4(float* p, float4 v) { *reinterpret_cast<float4*>(p) = v; }
__device__ __forceinline__ float4 keep4(float4 v, bool ok) { return ok ? v : make_float4(0.f, 0.f, 0.f, 0.f); }
__device__ __forceinline__ f32x4 mfma(float a, float b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }

constexpr int TT = 64, LDT = 80;                         // tokens of a tile; LDS row stride of a staged operand tile
constexpr int GMAX = 64 * 65;                            // floats of a group's staged G: nh dh (dh + 1) <= 64 * 65
static_assert(TT == COAT_TT && COAT_GW == 64, "one tile size, 64 columns a group");

struct Grp { int h0, nh, c0, W; };                       // first head, heads, first column, columns of a head group
__device__ __forceinline__ Grp group_of(int gi, int H, int dh) {
    const int hpg = max(1, COAT_GW / dh), h0 = gi * hpg, nh = min(hpg, H - h0);
    return {h0, nh, h0 * dh, nh * dh};
}
int groups_of(int H, int dh) { const int hpg = std::max(1, COAT_GW / dh); return (H + hpg - 1) / hpg; }

// rows row0 .. row0 + 64 of X (row stride sx), the group's columns 0 .. W: thread t takes the quads t, t + 256, ...; a row past T is `fill`
// (columns past W repeat the last quad: they are staged and never read)
__device__ __forceinline__ void load_tile(const float* __restrict__ X, int64_t sx, int row0, int T, int W, float fill, float4 (&v)[4]) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int e = j * 256 + (int)threadIdx.x, row = row0 + (e >> 4), c = 4 * (e & 15);
        const float4 x = ld4(X + (int64_t)min(row, T - 1) * sx + min(c, W - 4));
        v[j] = row < T ? x : make_float4(fill, fill, fill, fill);
    }
}
__device__ __forceinline__ void write_tile(float* tile, const float4 (&v)[4]) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int e = j * 256 + (int)threadIdx.x;
        st4(tile + (e >> 4) * LDT + 4 * (e & 15), v[j]);
    }
}

// SM: the forward (A = k under the online column softmax, B = v, writes gram and kstat); else the backward (A = q, B = dout, writes dgram)
template <int KC, bool SM>
__global__ void __launch_bounds__(256) coat_reduce_kernel(const CoatAttn p) {
    __shared__ __attribute__((aligned(16))) float As[TT * LDT];
    __shared__ __attribute__((aligned(16))) float Bs[TT * LDT];
    __shared__ float part[4 * 64], ms[64], ls[64], al[64];
    const int tid = threadIdx.x, wave = tid >> 6, r = tid & 15, g = (tid >> 4) & 3;
    const int f = blockIdx.y, T = p.T, dh = p.dh, C = p.H * dh;
    const Grp G = group_of(blockIdx.x, p.H, dh);
    const float* A = p.qkv + (int64_t)f * T * 3 * C + (SM ? C : 0) + G.c0;
    const float* B = SM ? p.qkv + (int64_t)f * T * 3 * C + 2 * C + G.c0 : p.dout + (int64_t)f * T * C + G.c0;
    const int64_t sa = 3 * C, sb = SM ? 3 * C : C;
    const float fill = SM ? -INFINITY : 0.f;
    // this wave's four tiles: slot s is tile wave + 4 s of the group's nh KC^2, as (head, row tile, column tile)
    const int ntile = G.nh * KC * KC;
    int hs[4], ti[4], tj[4], ca[4], cb[4];
    bool ok[4];
    f32x4 acc[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        const int id = wave + 4 * s, idc = min(id, ntile - 1);
        ok[s] = id < ntile;
        hs[s] = idc / (KC * KC); ti[s] = (idc / KC) % KC; tj[s] = idc % KC;
        ca[s] = min(hs[s] * dh + 16 * ti[s] + r, G.W - 1);
        cb[s] = min(hs[s] * dh + 16 * tj[s] + r, G.W - 1);
        acc[s] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    if (tid < 64) { ms[tid] = -INFINITY; ls[tid] = 0.f; }
    float4 pa[4], pb[4];
    load_tile(A, sa, 0, T, G.W, fill, pa);
    load_tile(B, sb, 0, T, G.W, 0.f, pb);
    const int NT = (T + TT - 1) / TT;
    for (int kt = 0; kt < NT; ++kt) {
        __syncthreads();                                                   // the tile before is consumed
        write_tile(As, pa);
        write_tile(Bs, pb);
        const int nxt = TT * min(kt + 1, NT - 1);                          // (the last pass loads its own tile once more: unconditional loads)
        load_tile(A, sa, nxt, T, G.W, fill, pa);
        load_tile(B, sb, nxt, T, G.W, 0.f, pb);
        __syncthreads();
        if (SM) {
            const int col = tid & 63, q4 = tid >> 6;
            float pm = -INFINITY;
#pragma unroll
            for (int i = 0; i < 16; ++i) pm = fmaxf(pm, As[(16 * q4 + i) * LDT + col]);
            part[q4 * 64 + col] = pm;
            __syncthreads();
            if (tid < 64) {                                                // (every tile has a real token: the new maximum is finite)
                const float tm = fmaxf(fmaxf(part[tid], part[64 + tid]), fmaxf(part[128 + tid], part[192 + tid]));
                const float mo = ms[tid], mn = fmaxf(mo, tm);
                al[tid] = expf(mo - mn);                                   // (first tile: exp(-inf) = 0 against l = 0 and G = 0)
                ms[tid] = mn;
            }
            __syncthreads();
            const float mn = ms[col];
            float ps = 0.f;
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const float e = expf(As[(16 * q4 + i) * LDT + col] - mn);  // (a token past T: exp(-inf) = 0)
                As[(16 * q4 + i) * LDT + col] = e;
                ps = ps + e;
            }
            part[q4 * 64 + col] = ps;
            __syncthreads();
            if (tid < 64) ls[tid] = ls[tid] * al[tid] + (((part[tid] + part[64 + tid]) + part[128 + tid]) + part[192 + tid]);
#pragma unroll
            for (int s = 0; s < 4; ++s)
#pragma unroll
                for (int i = 0; i < 4; ++i) acc[s][i] = acc[s][i] * al[min(hs[s] * dh + 16 * ti[s] + 4 * g + i, G.W - 1)];
        }
#pragma unroll
        for (int s = 0; s < 4; ++s)
#pragma unroll
            for (int n = 0; n < TT / 4; ++n) acc[s] = mfma(As[(4 * n + g) * LDT + ca[s]], Bs[(4 * n + g) * LDT + cb[s]], acc[s]);
    }
    __syncthreads();                                                       // ms and ls are final
    float* dst = (SM ? p.gram : p.dgram) + ((int64_t)f * p.H + G.h0) * dh * dh;
#pragma unroll
    for (int s = 0; s < 4; ++s)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int a = 16 * ti[s] + 4 * g + i, b = 16 * tj[s] + r;
            if (ok[s] && a < dh && b < dh) {
                const float v = SM ? acc[s][i] / ls[hs[s] * dh + a] : acc[s][i] * p.scale;
                dst[((int64_t)hs[s] * dh + a) * dh + b] = v;
            }
        }
    if (SM && tid < G.W) {
        const int hh = tid / dh, a = tid - hh * dh;
        float* st = p.kstat + ((int64_t)f * p.H + G.h0 + hh) * 2 * dh;
        st[a] = ms[tid];
        st[dh + a] = logf(ls[tid]);
    }
}

// the group's nh matrices (dh, dh), contiguous in memory, into LDS at row stride dh + 1
__device__ __forceinline__ void stage_gram(const float* __restrict__ src, int nh, int dh, float* Gs) {
    const int n = nh * dh * dh;
    for (int e = threadIdx.x; e < n; e += 256) {
        const int row = e / dh, b = e - row * dh;                          // row = hh dh + a
        Gs[row * (dh + 1) + b] = src[e];
    }
}

// this lane's operand quads of row `row` of X (a row past T: zeros): x[kc] = columns 16 kc + 4 g .. + 3 of the head
template <int KC>
__device__ __forceinline__ void row_frag(const float* X, int64_t sx, int row, int T, int dh, float4 (&x)[KC]) {
    const int g = (threadIdx.x >> 4) & 3;
    const float* p = X + (int64_t)min(row, T - 1) * sx;
#pragma unroll
    for (int kc = 0; kc < KC; ++kc) {
        const int c = 16 * kc + 4 * g;
        x[kc] = keep4(ld4(p + min(c, dh - 4)), row < T && c < dh);         // (dh % 4 == 0: a quad is whole or absent)
    }
}

// o[j][i] = sum over k of X[own row 4 g + i][k] M'[k][16 j + r], M' = M (dh, dh at row stride ld) or, with TR, its transpose; one fma
// chain from 0 over k in chunks of 16, inside a chunk 0 4 8 12 1 5 9 13 ...; indices past dh are clamped (their X operand is zero)
template <int KC, bool TR>
__device__ __forceinline__ void rows_times_m(const float4 (&x)[KC], const float* M, int ld, int dh, f32x4 (&o)[KC]) {
    const int r = threadIdx.x & 15, g = (threadIdx.x >> 4) & 3;
#pragma unroll
    for (int j = 0; j < KC; ++j) {
        const int n = min(16 * j + r, dh - 1);
        o[j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int kc = 0; kc < KC; ++kc) {
            const int k0 = min(16 * kc + 4 * g, dh - 4);
            const float* m = TR ? M + n * ld + k0 : M + k0 * ld + n;
            const int ks = TR ? 1 : ld;
            o[j] = mfma(x[kc].x, m[0], o[j]);
            o[j] = mfma(x[kc].y, m[ks], o[j]);
            o[j] = mfma(x[kc].z, m[2 * ks], o[j]);
            o[j] = mfma(x[kc].w, m[3 * ks], o[j]);
        }
    }
}

template <int KC>
__global__ void __launch_bounds__(256) coat_apply_kernel(const CoatAttn p) {
    __shared__ float Gs[GMAX];
    const int tid = threadIdx.x, wave = tid >> 6, r = tid & 15, g = (tid >> 4) & 3;
    const int f = blockIdx.z, T = p.T, dh = p.dh, C = p.H * dh, ld = dh + 1, t0 = TT * (int)blockIdx.x + 16 * wave;
    const Grp G = group_of(blockIdx.y, p.H, dh);
    stage_gram(p.gram + ((int64_t)f * p.H + G.h0) * dh * dh, G.nh, dh, Gs);
    __syncthreads();
    const float *qf = p.qkv + (int64_t)f * T * 3 * C, *Ef = p.E + (int64_t)f * T * C;
    float* of = p.out + (int64_t)f * T * C;
    for (int hh = 0; hh < G.nh; ++hh) {
        const int hc = (G.h0 + hh) * dh;
        float4 xq[KC];
        f32x4 o[KC];
        row_frag<KC>(qf + hc, 3 * C, t0 + r, T, dh, xq);
        rows_times_m<KC, false>(xq, Gs + hh * dh * ld, ld, dh, o);
#pragma unroll
        for (int j = 0; j < KC; ++j) {
            const int col = 16 * j + r, cc = hc + min(col, dh - 1);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int t = t0 + 4 * g + i, tc = min(t, T - 1);
                const float qv = qf[(int64_t)tc * 3 * C + cc], ev = Ef[(int64_t)tc * C + cc];
                if (t < T && col < dh) of[(int64_t)t * C + hc + col] = o[j][i] * p.scale + qv * ev;
            }
        }
    }
}

template <int KC>
__global__ void __launch_bounds__(256) coat_apply_bwd_kernel(const CoatAttn p) {
    __shared__ float Gs[GMAX], Ds[GMAX], cs[64], km[64], kl[64];
    const int tid = threadIdx.x, wave = tid >> 6, r = tid & 15, g = (tid >> 4) & 3;
    const int f = blockIdx.z, T = p.T, dh = p.dh, C = p.H * dh, ld = dh + 1, t0 = TT * (int)blockIdx.x + 16 * wave;
    const Grp G = group_of(blockIdx.y, p.H, dh);
    stage_gram(p.gram + ((int64_t)f * p.H + G.h0) * dh * dh, G.nh, dh, Gs);
    stage_gram(p.dgram + ((int64_t)f * p.H + G.h0) * dh * dh, G.nh, dh, Ds);
    __syncthreads();
    if (tid < G.W) {                                                       // c[a] = sum_b G[a][b] dG[a][b]; the column statistics
        const int hh = tid / dh, a = tid - hh * dh;
        float c = 0.f;                                                     // b in the order of the chain v dG^T below, which c is subtracted from:
#pragma unroll                                                             // where a softmax column is one-hot, G's row is that token's v and the two cancel exactly
        for (int kc = 0; kc < KC; ++kc)
#pragma unroll
            for (int s = 0; s < 4; ++s)
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int b = 16 * kc + 4 * q + s;
                    if (b < dh) c = fmaf(Gs[tid * ld + b], Ds[tid * ld + b], c);
                }
        cs[tid] = c;
        const float* st = p.kstat + ((int64_t)f * p.H + G.h0 + hh) * 2 * dh;
        km[tid] = st[a];
        kl[tid] = st[dh + a];
    }
    __syncthreads();
    const float *qf = p.qkv + (int64_t)f * T * 3 * C, *Ef = p.E + (int64_t)f * T * C, *gf = p.dout + (int64_t)f * T * C;
    float *dqf = p.dqkv + (int64_t)f * T * 3 * C, *dEf = p.dE + (int64_t)f * T * C;
    for (int hh = 0; hh < G.nh; ++hh) {
        const int hc = (G.h0 + hh) * dh, lc = hh * dh;                     // the head's first column in a row and in the group
        float4 xd[KC], xv[KC], xk[KC];
        f32x4 oq[KC], ov[KC], ok[KC];
        row_frag<KC>(gf + hc, C, t0 + r, T, dh, xd);
        row_frag<KC>(qf + 2 * C + hc, 3 * C, t0 + r, T, dh, xv);
        row_frag<KC>(qf + C + hc, 3 * C, t0 + r, T, dh, xk);
#pragma unroll
        for (int kc = 0; kc < KC; ++kc) {                                  // Ks = exp((k - max) - logsum); zero past T and dh
            const int c = 16 * kc + 4 * g, cc = lc + min(c, dh - 4);
            const bool in = t0 + r < T && c < dh;
            xk[kc] = keep4(make_float4(expf((xk[kc].x - km[cc]) - kl[cc]), expf((xk[kc].y - km[cc + 1]) - kl[cc + 1]),
                                       expf((xk[kc].z - km[cc + 2]) - kl[cc + 2]), expf((xk[kc].w - km[cc + 3]) - kl[cc + 3])), in);
        }
        rows_times_m<KC, true>(xd, Gs + lc * ld, ld, dh, oq);              // dout G^T
        rows_times_m<KC, false>(xk, Ds + lc * ld, ld, dh, ov);             // Ks dG
        rows_times_m<KC, true>(xv, Ds + lc * ld, ld, dh, ok);              // v dG^T
#pragma unroll
        for (int j = 0; j < KC; ++j) {
            const int col = 16 * j + r, cl = min(col, dh - 1), cc = hc + cl;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int t = t0 + 4 * g + i, tc = min(t, T - 1);
                const float dv = gf[(int64_t)tc * C + cc], ev = Ef[(int64_t)tc * C + cc];
                const float qv = qf[(int64_t)tc * 3 * C + cc], kv = qf[(int64_t)tc * 3 * C + C + cc];
                const float Ks = expf((kv - km[lc + cl]) - kl[lc + cl]);
                if (t < T && col < dh) {
                    float* d = dqf + (int64_t)t * 3 * C + hc + col;
                    d[0] = oq[j][i] * p.scale + dv * ev;
                    d[C] = Ks * (ok[j][i] - cs[lc + cl]);
                    d[2 * C] = ov[j][i];
                    dEf[(int64_t)t * C + hc + col] = dv * qv;
                }
            }
        }
    }
}

// one quad of channels of the plane position (py, px): the K x K taps in increasing (ky, kx) onto acc; MIRROR: the backward's gather
template <int K, bool MIRROR>
__device__ __forceinline__ float4 dw_taps(const float* __restrict__ plane, int64_t rs, const float* __restrict__ w, int n, int g, int py, int px, float4 acc) {
#pragma unroll
    for (int ky = 0; ky < K; ++ky)
#pragma unroll
        for (int kx = 0; kx < K; ++kx) {
            const int iy = MIRROR ? py + K / 2 - ky : py + ky - K / 2, ix = MIRROR ? px + K / 2 - kx : px + kx - K / 2;
            const bool in = iy >= 0 && iy < g && ix >= 0 && ix < g;
            const float4 x = ld4(plane + (int64_t)(min(max(iy, 0), g - 1) * g + min(max(ix, 0), g - 1)) * rs);
            const float4 wv = ld4(w + (int64_t)(ky * K + kx) * n);
            if (in) {                                                      // a tap on the padding takes no part
                acc.x = fmaf(wv.x, x.x, acc.x); acc.y = fmaf(wv.y, x.y, acc.y);
                acc.z = fmaf(wv.z, x.z, acc.z); acc.w = fmaf(wv.w, x.w, acc.w);
            }
        }
    return acc;
}

template <bool BWD>
__global__ void __launch_bounds__(256) coat_dwmix_kernel(const CoatDw p) {
    const int g = p.g, C4 = p.C / 4, R = p.prefix + g * g, n7 = p.C - p.n3 - p.n5;
    const int64_t n = (int64_t)p.F * R * C4;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < n; e += (int64_t)gridDim.x * 256) {
        const int c = 4 * (int)(e % C4), t = (int)((e / C4) % R);
        const int64_t f = e / ((int64_t)C4 * R);
        const float4 xc = ld4(p.x + (f * R + t) * p.xrs + c);
        float* y = p.y + (f * R + t) * p.yrs + c;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (t < p.prefix) {
            if (BWD && p.accumulate && !p.residual) continue;
            if (p.residual) v = xc;
        } else {
            const int py = (t - p.prefix) / g, px = (t - p.prefix) % g;
            const float* plane = p.x + (f * R + p.prefix) * p.xrs + c;
            if (!BWD && p.b) v = ld4(p.b + c);
            if (c < p.n3) v = dw_taps<3, BWD>(plane, p.xrs, p.w3 + c, p.n3, g, py, px, v);
            else if (c < p.n3 + p.n5) v = dw_taps<5, BWD>(plane, p.xrs, p.w5 + (c - p.n3), p.n5, g, py, px, v);
            else v = dw_taps<7, BWD>(plane, p.xrs, p.w7 + (c - p.n3 - p.n5), n7, g, py, px, v);
            if (p.residual) v = make_float4(xc.x + v.x, xc.y + v.y, xc.z + v.z, xc.w + v.w);
        }
        if (BWD && p.accumulate) {
            const float4 o = ld4(y);
            v = make_float4(o.x + v.x, o.y + v.y, o.z + v.z, o.w + v.w);
        }
        st4(y, v);
    }
}

template <bool SCATTER>
__global__ void __launch_bounds__(256) coat_cells_kernel(const CoatCells p) {
    const int g = p.g, C4 = p.C / 4, s = p.s, go = g / s, R = p.prefix + g * g;
    const int64_t n = (int64_t)p.F * R * C4;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < n; e += (int64_t)gridDim.x * 256) {
        const int c = 4 * (int)(e % C4), t = (int)((e / C4) % R);
        const int64_t f = e / ((int64_t)C4 * R), at = (f * R + t) * p.C + c;
        if (t < p.prefix) {
            if (SCATTER && !p.accumulate) st4(p.dst + at, make_float4(0.f, 0.f, 0.f, 0.f));
            continue;
        }
        const int py = (t - p.prefix) / g, px = (t - p.prefix) % g;
        const int64_t cell = ((f * go + py / s) * go + px / s) * s * s * p.C + (int64_t)((py % s) * s + px % s) * p.C + c;
        if (!SCATTER) {
            st4(p.dst + cell, ld4(p.src + at));
        } else {
            float4 v = ld4(p.src + cell);
            if (p.accumulate) {
                const float4 o = ld4(p.dst + at);
                v = make_float4(o.x + v.x, o.y + v.y, o.z + v.z, o.w + v.w);
            }
            st4(p.dst + at, v);
        }
    }
}

int refuse(const char* who, const char* why) {
    char buf[256];
    snprintf(buf, sizeof buf, "%s: %s: %s", who, hipGetErrorName(hipErrorInvalidValue), why);
    return i2v_api_fail(buf);
}

unsigned blocks_for(int64_t n) { return (unsigned)std::min<int64_t>((n + 255) / 256, 65535); }

// which: 0 reduce forward, 1 apply forward, 2 reduce backward, 3 apply backward
template <int KC>
void launch(int which, const CoatAttn& p, hipStream_t s) {
    const unsigned ng = (unsigned)groups_of(p.H, p.dh);
    const dim3 red(ng, (unsigned)p.F), app((unsigned)((p.T + TT - 1) / TT), ng, (unsigned)p.F);
    if (which == 0) hipLaunchKernelGGL((coat_reduce_kernel<KC, true>), red, dim3(256), 0, s, p);
    else if (which == 1) hipLaunchKernelGGL(coat_apply_kernel<KC>, app, dim3(256), 0, s, p);
    else if (which == 2) hipLaunchKernelGGL((coat_reduce_kernel<KC, false>), red, dim3(256), 0, s, p);
    else hipLaunchKernelGGL(coat_apply_bwd_kernel<KC>, app, dim3(256), 0, s, p);
}

void launch_for(int which, const CoatAttn& p, hipStream_t s) {
    switch ((p.dh + 15) / 16) {
        case 1: return launch<1>(which, p, s);
        case 2: return launch<2>(which, p, s);
        case 3: return launch<3>(which, p, s);
        default: return launch<4>(which, p, s);
    }
}

}  // namespace

int coat_attention(const CoatAttn& p, hipStream_t s) {
    const char* who = "coat_attention";
    if (const char* why = coat_attn_refusal(p, false)) return refuse(who, why);
    launch_for(0, p, s);
    launch_for(1, p, s);
    __atomic_fetch_add(&g_stat_coat, 2, __ATOMIC_RELAXED);
    return vit_launch_check(who);
}

int coat_attention_bwd(const CoatAttn& p, hipStream_t s) {
    const char* who = "coat_attention_bwd";
    if (const char* why = coat_attn_refusal(p, true)) return refuse(who, why);
    launch_for(2, p, s);
    launch_for(3, p, s);
    __atomic_fetch_add(&g_stat_coat, 2, __ATOMIC_RELAXED);
    return vit_launch_check(who);
}

int coat_dwmix(const CoatDw& p, hipStream_t s) {
    if (const char* why = coat_dw_refusal(p)) return refuse("coat_dwmix", why);
    hipLaunchKernelGGL(coat_dwmix_kernel<false>, dim3(blocks_for((int64_t)p.F * (p.prefix + p.g * p.g) * (p.C / 4))), dim3(256), 0, s, p);
    return vit_launch_check("coat_dwmix");
}

int coat_dwmix_bwd(const CoatDw& p, hipStream_t s) {
    if (const char* why = coat_dw_refusal(p)) return refuse("coat_dwmix_bwd", why);
    hipLaunchKernelGGL(coat_dwmix_kernel<true>, dim3(blocks_for((int64_t)p.F * (p.prefix + p.g * p.g) * (p.C / 4))), dim3(256), 0, s, p);
    return vit_launch_check("coat_dwmix_bwd");
}

int coat_cell_gather(const CoatCells& p, hipStream_t s) {
    if (const char* why = coat_cells_refusal(p)) return refuse("coat_cell_gather", why);
    hipLaunchKernelGGL(coat_cells_kernel<false>, dim3(blocks_for((int64_t)p.F * (p.prefix + p.g * p.g) * (p.C / 4))), dim3(256), 0, s, p);
    return vit_launch_check("coat_cell_gather");
}

int coat_cell_scatter(const CoatCells& p, hipStream_t s) {
    if (const char* why = coat_cells_refusal(p)) return refuse("coat_cell_scatter", why);
    hipLaunchKernelGGL(coat_cells_kernel<true>, dim3(blocks_for((int64_t)p.F * (p.prefix + p.g * p.g) * (p.C / 4))), dim3(256), 0, s, p);
    return vit_launch_check("coat_cell_scatter");
}
