// The TNT launches for gfx950 (i2v_tnt_kernels.h): attention over very many very short sequences -- TNT's inner transformer runs over
// the 16 pixel tokens of every patch, 25 088 sequences x 4 heads of a 16 x 16 score matrix over heads 6 or 10 floats wide at 128
// frames -- forward and input gradient, one launch each; the pixel embedding's row gather and its transpose; a row-periodic add.
//
// ATTENTION.  Up to 16 tokens, heads up to 16 wide (ANY width: 6 and 10 are the real ones), up to 8 heads, H dh a multiple of 4.  Per
// sequence the problem reads 4.6 KB, writes 1.5 KB and does about 25 kflop: far below the machine balance, byte-bound, and the fp32
// vector rate equals the fp32 MFMA rate on this chip, so there is no MFMA here.  A workgroup of 256 threads owns
// ns = tnt_group(T, H, dh) WHOLE sequences, as many as give every thread at most one (sequence, head, row) and fit 64 KB of LDS:
//   - the ns sequences' qkv are one contiguous run of memory: staged into LDS with float4 loads, every byte read once;
//   - thread (sequence, head, row i) holds q_i in registers, forms its row of scores against the T keys out of LDS (lanes of one
//     (sequence, head) read the same k_j and v_j: broadcasts), the softmax in registers, and the row of out;
//   - out_i is written over q_i in LDS (no other thread reads that slot) and, after a barrier, the workgroup's rows of out -- again one
//     contiguous run -- leave with float4 stores.  Nothing of the score matrix is written anywhere.
//   BACKWARD, from qkv and dout alone (the forward saves nothing): pass A, thread = row i: P and dS of the row as above, dq_i kept in
//   registers, (m, l, delta) of the row to LDS.  Pass B, the same thread as key j: k_j and v_j in registers; for i increasing the score
//   s[i][j], P[i][j] and dS[i][j] are formed AGAIN from the row's (m, l, delta) -- the same expressions in the same order as pass A,
//   so the same bits -- and dk_j, dv_j accumulate.  After a barrier dq, dk and dv are written over q, k and v in LDS and the
//   workgroup's dqkv leaves as one contiguous run.  One owner per output element, no atomics.
// The kernels are compiled per head width 1 .. 16 and run straight-line over all 16 keys: register arrays are indexed by unrolled
// constants only and there is no branch in the arithmetic; a key past T reads the last key's row with its score forced to -inf, so
// its e is exactly 0 and it takes no part in any sum.  A sequence's arithmetic does not depend on S nor on which sequences share its workgroup:
// sequence 0 of an n-sequence call has the bits of a 1-sequence call, and reruns repeat the bits.  include/i2v_tnt.h states the order
// of every sum (-ffp-contract=off).
//
// PIXEL GATHER / SCATTER: one thread per 4 columns of a row (gather) or per pixel (scatter, at most 2 x 2 contributions summed in a
// fixed order), grid-stride.  ROW ADD: one thread per 4 floats.
#include <algorithm>

#include "i2v_be.h"
#include "i2v_tnt_kernels.h"
#include "i2v_vit_kernels.h"     // vit_launch_check

long long g_stat_tnt = 0;

namespace {

__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ void st4(float* p, float4 v) { *reinterpret_cast<float4*>(p) = v; }

constexpr int NT = TNT_THREADS, MT = TNT_MAX_T;

// x . y over the head's DH columns, increasing from 0; x in registers, y in LDS
template <int DH>
__device__ __forceinline__ float dot_reg_lds(const float (&x)[DH], const float* __restrict__ y) {
    float acc = 0.f;
#pragma unroll
    for (int d = 0; d < DH; ++d) acc = fmaf(x[d], y[d], acc);
    return acc;
}

// row i of one (sequence, head) staged at `base` (q at 0, k at C, v at 2 C, row stride C3): e[j] = exp(s[j] - m), and (m, l).  The code
// is straight-line over all 16 keys: a key past T reads the last key's row and its score is set to -inf, so that its e is exactly 0
// and takes no part in any sum (x + 0 = x, fma(0, y, x) = x).
template <int DH>
__device__ __forceinline__ void score_row(const float (&q)[DH], const float* __restrict__ base, int C, int C3, int T, float scale, float (&e)[MT],
                                          float& m, float& l) {
    m = -INFINITY;
#pragma unroll
    for (int j = 0; j < MT; ++j) {
        const float sc = dot_reg_lds<DH>(q, base + min(j, T - 1) * C3 + C) * scale;
        e[j] = j < T ? sc : -INFINITY;
        m = fmaxf(m, e[j]);
    }
    l = 0.f;
#pragma unroll
    for (int j = 0; j < MT; ++j) {
        e[j] = expf(e[j] - m);
        l = l + e[j];
    }
}

template <int DH>
__global__ void __launch_bounds__(NT) tnt_attn_kernel(const TntAttn p, const int ns) {
    extern __shared__ float4 tnt_lds4[];
    float* L = reinterpret_cast<float*>(tnt_lds4);
    const int T = p.T, H = p.H, C = H * DH, C3 = 3 * C, tid = (int)threadIdx.x;
    const int64_t s0 = (int64_t)blockIdx.x * ns;
    const int n = (int)min((int64_t)ns, p.S - s0);               // sequences of this workgroup: the last one may hold fewer
    const float* src = p.qkv + s0 * T * C3;
    for (int e = tid; e < n * T * C3 / 4; e += NT) st4(L + 4 * e, ld4(src + 4 * e));
    __syncthreads();
    const int per = H * T;
    if (tid < n * per) {
        const int seq = tid / per, h = (tid % per) / T, i = tid % T;
        float* base = L + seq * T * C3 + h * DH;
        float q[DH], e[MT], o[DH], m, l;
#pragma unroll
        for (int d = 0; d < DH; ++d) q[d] = base[i * C3 + d];
        score_row<DH>(q, base, C, C3, T, p.scale, e, m, l);
#pragma unroll
        for (int d = 0; d < DH; ++d) o[d] = 0.f;
#pragma unroll
        for (int j = 0; j < MT; ++j) {
            const float P = e[j] / l;
            const float* v = base + min(j, T - 1) * C3 + 2 * C;
#pragma unroll
            for (int d = 0; d < DH; ++d) o[d] = fmaf(P, v[d], o[d]);
        }
#pragma unroll
        for (int d = 0; d < DH; ++d) base[i * C3 + d] = o[d];    // over q_i: only this thread reads that slot
    }
    __syncthreads();
    float* dst = p.out + s0 * T * C;
    const int C4 = C / 4;
    for (int e = tid; e < n * T * C4; e += NT) {
        const int row = e / C4, c = 4 * (e % C4);
        st4(dst + (int64_t)row * C + c, ld4(L + row * C3 + c));
    }
}

template <int DH>
__global__ void __launch_bounds__(NT) tnt_attn_bwd_kernel(const TntAttn p, const int ns) {
    extern __shared__ float4 tnt_lds4[];
    float* L = reinterpret_cast<float*>(tnt_lds4);
    const int T = p.T, H = p.H, C = H * DH, C3 = 3 * C, tid = (int)threadIdx.x;
    float* LG = L + ns * T * C3;                                   // dout (n, T, C)
    float* LS = LG + ns * T * C;                                   // (m, l, delta) per (sequence, head, row)
    const int64_t s0 = (int64_t)blockIdx.x * ns;
    const int n = (int)min((int64_t)ns, p.S - s0);
    const float *src = p.qkv + s0 * T * C3, *gsrc = p.dout + s0 * T * C;
    for (int e = tid; e < n * T * C3 / 4; e += NT) st4(L + 4 * e, ld4(src + 4 * e));
    for (int e = tid; e < n * T * C / 4; e += NT) st4(LG + 4 * e, ld4(gsrc + 4 * e));
    __syncthreads();
    const int per = H * T;
    const bool on = tid < n * per;
    const int seq = on ? tid / per : 0, h = on ? (tid % per) / T : 0, i = on ? tid % T : 0;
    float* base = L + seq * T * C3 + h * DH;
    const float* gbase = LG + seq * T * C + h * DH;
    float* st = LS + (seq * H + h) * T * 3;
    float dq[DH], dk[DH], dv[DH];
    if (on) {                                                      // pass A: the thread is row i
        float q[DH], g[DH], e[MT], m, l, delta = 0.f;
#pragma unroll
        for (int d = 0; d < DH; ++d) {
            q[d] = base[i * C3 + d];
            g[d] = gbase[i * C + d];
        }
        score_row<DH>(q, base, C, C3, T, p.scale, e, m, l);
        asm volatile("" ::: "memory");                             // (k and v are read again from LDS below, not kept in registers across the passes:
        float dP[MT];                                              //  256 values at dh 16)
#pragma unroll
        for (int j = 0; j < MT; ++j) {                             // e[j] becomes P[j]; a key past T: 0
            e[j] = e[j] / l;
            dP[j] = dot_reg_lds<DH>(g, base + min(j, T - 1) * C3 + 2 * C);
            delta = fmaf(e[j], dP[j], delta);
        }
        asm volatile("" ::: "memory");
#pragma unroll
        for (int d = 0; d < DH; ++d) dq[d] = 0.f;
#pragma unroll
        for (int j = 0; j < MT; ++j) {
            const float* k = base + min(j, T - 1) * C3 + C;
            const float dS = e[j] * (dP[j] - delta);
#pragma unroll
            for (int d = 0; d < DH; ++d) dq[d] = fmaf(dS, k[d], dq[d]);
        }
        st[3 * i] = m; st[3 * i + 1] = l; st[3 * i + 2] = delta;
    }
    __syncthreads();
    if (on) {                                                      // pass B: the same thread is key j = i
        float k[DH], v[DH];
#pragma unroll
        for (int d = 0; d < DH; ++d) {
            k[d] = base[i * C3 + C + d];
            v[d] = base[i * C3 + 2 * C + d];
            dk[d] = dv[d] = 0.f;
        }
#pragma unroll 2
        for (int r = 0; r < T; ++r) {
            const float *qr = base + r * C3, *gr = gbase + r * C;
            float qv[DH], gv[DH], sc = 0.f, dP = 0.f;
#pragma unroll
            for (int d = 0; d < DH; ++d) {
                qv[d] = qr[d];
                gv[d] = gr[d];
                sc = fmaf(qv[d], k[d], sc);                        // (q_r . k_j and dout_r . v_j in pass A's order)
                dP = fmaf(gv[d], v[d], dP);
            }
            const float P = expf(sc * p.scale - st[3 * r]) / st[3 * r + 1], dS = P * (dP - st[3 * r + 2]);
#pragma unroll
            for (int d = 0; d < DH; ++d) {
                dk[d] = fmaf(dS, qv[d], dk[d]);
                dv[d] = fmaf(P, gv[d], dv[d]);
            }
        }
    }
    __syncthreads();                                               // every read of q, k and v is done
    if (on) {
#pragma unroll
        for (int d = 0; d < DH; ++d) {
            base[i * C3 + d] = dq[d] * p.scale;
            base[i * C3 + C + d] = dk[d] * p.scale;
            base[i * C3 + 2 * C + d] = dv[d];
        }
    }
    __syncthreads();
    float* dst = p.dqkv + s0 * T * C3;
    for (int e = tid; e < n * T * C3 / 4; e += NT) st4(dst + 4 * e, ld4(L + 4 * e));
}

__global__ void __launch_bounds__(256) tnt_gather_kernel(const TntPixels p) {
    const int side = p.side, g = side / 16, K = p.Cin * 49, Kp = tnt_pixel_cols(p.Cin), Kp4 = Kp / 4;
    const int64_t n = (int64_t)p.F * g * g * 16 * Kp4;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < n; e += (int64_t)gridDim.x * 256) {
        const int q4 = (int)(e % Kp4);
        const int64_t r = e / Kp4, f = r / (16 * g * g);
        const int pix = (int)(r % 16), px = (int)((r / 16) % g), py = (int)((r / 16 / g) % g);
        const int oy = 4 * py + pix / 4, ox = 4 * px + pix % 4;
        float v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int col = 4 * q4 + u, c = col / 49, ky = (col % 49) / 7, kx = col % 7, y = 4 * oy + ky - 3, x = 4 * ox + kx - 3;
            v[u] = 0.f;
            if (col < K && y >= 0 && y < side && x >= 0 && x < side) v[u] = p.src[((f * p.Cin + c) * side + y) * side + x];
        }
        st4(p.dst + r * Kp + 4 * q4, make_float4(v[0], v[1], v[2], v[3]));
    }
}

__global__ void __launch_bounds__(256) tnt_scatter_kernel(const TntPixels p) {
    const int side = p.side, g = side / 16, Kp = tnt_pixel_cols(p.Cin), no = side / 4;
    const int64_t n = (int64_t)p.F * p.Cin * side * side;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < n; e += (int64_t)gridDim.x * 256) {
        const int x = (int)(e % side), y = (int)((e / side) % side), c = (int)((e / side / side) % p.Cin);
        const int64_t f = e / side / side / p.Cin;
        float acc = 0.f;
        for (int oy = y / 4; oy <= (y + 3) / 4 && oy < no; ++oy)          // 0 <= ky = y + 3 - 4 oy <= 6
            for (int ox = x / 4; ox <= (x + 3) / 4 && ox < no; ++ox) {
                const int ky = y + 3 - 4 * oy, kx = x + 3 - 4 * ox;
                const int64_t row = ((f * g + oy / 4) * g + ox / 4) * 16 + (oy % 4) * 4 + ox % 4;
                acc = acc + p.src[row * Kp + c * 49 + ky * 7 + kx];
            }
        p.dst[e] = p.accumulate ? p.dst[e] + acc : acc;
    }
}

__global__ void __launch_bounds__(256) tnt_row_add_kernel(float* __restrict__ x, const float* __restrict__ table, int64_t rows, int C4, int64_t period) {
    const int64_t n = rows * C4;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < n; e += (int64_t)gridDim.x * 256) {
        const int64_t r = e / C4;
        const int c = 4 * (int)(e % C4);
        const float4 a = ld4(x + r * 4 * C4 + c), b = ld4(table + (r % period) * 4 * C4 + c);
        st4(x + r * 4 * C4 + c, make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w));
    }
}

int refuse(const char* who, const char* why) {
    char buf[256];
    snprintf(buf, sizeof buf, "%s: %s: %s", who, hipGetErrorName(hipErrorInvalidValue), why);
    return i2v_api_fail(buf);
}

unsigned blocks_for(int64_t n) { return (unsigned)std::min<int64_t>((n + 255) / 256, 65535); }

template <int DH>
void launch(bool bwd, const TntAttn& p, hipStream_t s) {
    const int ns = tnt_group(p.T, p.H, p.dh);
    const dim3 grid((unsigned)((p.S + ns - 1) / ns));
    if (!bwd) hipLaunchKernelGGL(tnt_attn_kernel<DH>, grid, dim3(NT), (size_t)ns * p.T * 3 * p.H * p.dh * 4, s, p, ns);
    else hipLaunchKernelGGL(tnt_attn_bwd_kernel<DH>, grid, dim3(NT), (size_t)tnt_lds_floats(ns, p.T, p.H, p.dh) * 4, s, p, ns);
}

void launch_for(bool bwd, const TntAttn& p, hipStream_t s) {
    switch (p.dh) {
#define TNT_DH(n) case n: return launch<n>(bwd, p, s);
        TNT_DH(1) TNT_DH(2) TNT_DH(3) TNT_DH(4) TNT_DH(5) TNT_DH(6) TNT_DH(7) TNT_DH(8) TNT_DH(9) TNT_DH(10) TNT_DH(11) TNT_DH(12) TNT_DH(13)
        TNT_DH(14) TNT_DH(15) TNT_DH(16)
#undef TNT_DH
    }
}

}  // namespace

int tnt_attention(const TntAttn& p, hipStream_t s) {
    if (const char* why = tnt_attn_refusal(p, false)) return refuse("tnt_attention", why);
    launch_for(false, p, s);
    __atomic_fetch_add(&g_stat_tnt, 1, __ATOMIC_RELAXED);
    return vit_launch_check("tnt_attention");
}

int tnt_attention_bwd(const TntAttn& p, hipStream_t s) {
    if (const char* why = tnt_attn_refusal(p, true)) return refuse("tnt_attention_bwd", why);
    launch_for(true, p, s);
    __atomic_fetch_add(&g_stat_tnt, 1, __ATOMIC_RELAXED);
    return vit_launch_check("tnt_attention_bwd");
}

int tnt_pixel_gather(const TntPixels& p, hipStream_t s) {
    if (const char* why = tnt_pixels_refusal(p)) return refuse("tnt_pixel_gather", why);
    const int g = p.side / 16;
    hipLaunchKernelGGL(tnt_gather_kernel, dim3(blocks_for((int64_t)p.F * g * g * 16 * (tnt_pixel_cols(p.Cin) / 4))), dim3(256), 0, s, p);
    return vit_launch_check("tnt_pixel_gather");
}

int tnt_pixel_scatter(const TntPixels& p, hipStream_t s) {
    if (const char* why = tnt_pixels_refusal(p)) return refuse("tnt_pixel_scatter", why);
    hipLaunchKernelGGL(tnt_scatter_kernel, dim3(blocks_for((int64_t)p.F * p.Cin * p.side * p.side)), dim3(256), 0, s, p);
    return vit_launch_check("tnt_pixel_scatter");
}

int tnt_row_add(float* x, const float* table, int64_t rows, int C, int64_t period, hipStream_t s) {
    if (const char* why = tnt_row_add_refusal(x, table, rows, C, period)) return refuse("tnt_row_add", why);
    hipLaunchKernelGGL(tnt_row_add_kernel, dim3(blocks_for(rows * (C / 4))), dim3(256), 0, s, x, table, rows, C / 4, period);
    return vit_launch_check("tnt_row_add");
}
