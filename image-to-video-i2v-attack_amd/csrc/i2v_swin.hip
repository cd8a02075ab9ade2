// Kernels of the Swin surrogates (include/i2v_swin.h).  Activations are TOKEN-MAJOR as in i2v_vit.hip: a frame is a
// (H*W, C) row-major matrix over the stage's grid, so the linear layers, the LayerNorms and the patch rows are the ViT kernels.
//
//   swin_attn_fwd_kernel   the whole attention core of a block in one launch.  One WAVE per (window, head) problem: T = ws*ws tokens of
//                          dh floats.  k and v of the problem are staged in LDS by coalesced float4 loads (a token's head slice is one
//                          contiguous dh-float run of its qkv row); lane i keeps query row i, its T scores and its output row in
//                          REGISTERS, and every k / v operand is a broadcast LDS read (all lanes the same address: no bank conflict),
//                          so the softmax needs no cross-lane step at all.  Products are fp32 FMAs (exact fp32 inputs, as everywhere).
//                          The cyclic shift and the window partition are index arithmetic on the token rows read and written; the
//                          relative-position bias is read from the head's (2 ws - 1)^2-entry table in LDS at index base_i - const_j;
//                          the shift mask is the closed-form region test (-100 where the two tokens' regions differ).
//   swin_attn_bwd_kernel   dqkv from dout with the probabilities RECOMPUTED (nothing but qkv is saved by the forward).  Lane i first
//                          works on row i (P, dP, dS, dq); then P and dS go through LDS once each so that lane j sums column j
//                          (dv = P^T dout, dk = dS^T q), with q and dout taking the LDS place of k and v.
//   swin_merge_kernel      patch merging's 2 x 2 gather and its adjoint scatter: a permutation, float4, no atomics.
#include <algorithm>

#include "i2v_be.h"
#include "i2v_swin_kernels.h"
#include "i2v_vit_kernels.h"

namespace {

// token i (row-major in the window) of window (wy, wx) of the grid rolled by (-shift, -shift): its rolled coordinates (y, x) and its
// place in the unrolled grid, rolled[y][x] = grid[(y + shift) % H][(x + shift) % W]
template <int WS>
__device__ __forceinline__ int win_token(int i, int wy, int wx, int H, int W, int shift, int& y, int& x) {
    const int r = i / WS, c = i - r * WS;
    y = wy * WS + r;
    x = wx * WS + c;
    int oy = y + shift, ox = x + shift;
    if (oy >= H) oy -= H;
    if (ox >= W) ox -= W;
    return oy * W + ox;
}

// region of a rolled coordinate under the slices [0, -ws), [-ws, -shift), [-shift, end)
__device__ __forceinline__ int shift_region(int y, int H, int ws, int shift) { return y < H - ws ? 0 : (y < H - shift ? 1 : 2); }

struct WinProblem {
    int f, h, wy, wx;
};
__device__ __forceinline__ WinProblem win_problem(int p, int heads, int H, int W, int ws) {
    WinProblem o;
    o.h = p % heads;
    const int fw = p / heads, nwx = W / ws, nwin = (H / ws) * nwx, w = fw % nwin;
    o.f = fw / nwin;
    o.wy = w / nwx;
    o.wx = w - o.wy * nwx;
    return o;
}

// scores of row i against the T keys in LDS (row stride RS), bias and mask added, then softmax over the keys in place
template <int WS, int DH, int RS>
__device__ __forceinline__ void win_probs(const float (&q)[DH], const float* __restrict__ Ks, const float* __restrict__ Bs, int i, int reg,
                                          int shift, float (&s)[WS * WS]) {
    constexpr int T = WS * WS, NB = 2 * WS - 1;
    const int bi = (i / WS + WS - 1) * NB + (i % WS) + WS - 1;
    float m = -INFINITY;
#pragma unroll
    for (int j = 0; j < T; ++j) {
        float a0 = 0.f, a1 = 0.f;
#pragma unroll
        for (int d = 0; d < DH; d += 4) {
            const float4 kk = *reinterpret_cast<const float4*>(Ks + j * RS + d);
            a0 = fmaf(q[d], kk.x, a0); a1 = fmaf(q[d + 1], kk.y, a1);
            a0 = fmaf(q[d + 2], kk.z, a0); a1 = fmaf(q[d + 3], kk.w, a1);
        }
        float a = __fadd_rn(__fadd_rn(a0, a1), Bs[bi - ((j / WS) * NB + (j % WS))]);
        if (shift) {
            const int rj = __builtin_amdgcn_readlane(reg, j);
            a = __fadd_rn(a, rj != reg ? -100.f : 0.f);
        }
        s[j] = a;
        m = fmaxf(m, a);
    }
    float sum = 0.f;
#pragma unroll
    for (int j = 0; j < T; ++j) {
        s[j] = expf(__fsub_rn(s[j], m));
        sum = __fadd_rn(sum, s[j]);
    }
    const float inv = __fdiv_rn(1.f, sum);
#pragma unroll
    for (int j = 0; j < T; ++j) s[j] = __fmul_rn(s[j], inv);
}

// k and v of the problem into LDS rows of stride RS (coalesced: D4 consecutive lanes read one token's dh-float slice), the head's bias table
template <int WS, int DH, int RS>
__device__ __forceinline__ void win_stage_kv(const float* __restrict__ base, int C, const float* __restrict__ table, int heads,
                                             const WinProblem& pr, int H, int W, int shift, int lane, float* __restrict__ Ks,
                                             float* __restrict__ Vs, float* __restrict__ Bs) {
    constexpr int T = WS * WS, D4 = DH / 4, NI = (2 * WS - 1) * (2 * WS - 1);
    for (int e = lane; e < T * D4; e += 64) {
        const int t = e / D4, part = e - t * D4;
        int y, x;
        const int64_t tok = win_token<WS>(t, pr.wy, pr.wx, H, W, shift, y, x);
        const float* row = base + tok * 3 * C + part * 4;
        *reinterpret_cast<float4*>(Ks + t * RS + part * 4) = *reinterpret_cast<const float4*>(row + C);
        *reinterpret_cast<float4*>(Vs + t * RS + part * 4) = *reinterpret_cast<const float4*>(row + 2 * C);
    }
    for (int e = lane; e < NI; e += 64) Bs[e] = table[e * heads + pr.h];
}

template <int WS, int DH, int WAVES>
__global__ void __launch_bounds__(64 * WAVES) swin_attn_fwd_kernel(const float* __restrict__ qkv, const float* __restrict__ table,
                                                                   float* __restrict__ out, int nprob, int H, int W, int shift, int heads,
                                                                   float scale) {
    constexpr int T = WS * WS, NI = (2 * WS - 1) * (2 * WS - 1);
    __shared__ __attribute__((aligned(16))) float Ks[WAVES][T * DH], Vs[WAVES][T * DH];
    __shared__ float Bs[WAVES][NI];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int p = blockIdx.x * WAVES + wave;
    const bool live = p < nprob;                                   // a spare wave of the last block works on the last problem and stores nothing
    const WinProblem pr = win_problem(live ? p : nprob - 1, heads, H, W, WS);
    const int C = heads * DH;
    const float* base = qkv + (int64_t)pr.f * H * W * 3 * C + pr.h * DH;
    win_stage_kv<WS, DH, DH>(base, C, table, heads, pr, H, W, shift, lane, Ks[wave], Vs[wave], Bs[wave]);
    const int i = lane < T ? lane : T - 1;                         // lanes past the window repeat its last row and store nothing
    int y, x;
    const int64_t tok = win_token<WS>(i, pr.wy, pr.wx, H, W, shift, y, x);
    const int reg = shift ? shift_region(y, H, WS, shift) * 3 + shift_region(x, W, WS, shift) : 0;
    float q[DH];
#pragma unroll
    for (int d = 0; d < DH; d += 4) {
        const float4 v = *reinterpret_cast<const float4*>(base + tok * 3 * C + d);
        q[d] = __fmul_rn(v.x, scale); q[d + 1] = __fmul_rn(v.y, scale); q[d + 2] = __fmul_rn(v.z, scale); q[d + 3] = __fmul_rn(v.w, scale);
    }
    __syncthreads();
    float s[T];
    win_probs<WS, DH, DH>(q, Ks[wave], Bs[wave], i, reg, shift, s);
    float o[DH];
#pragma unroll
    for (int d = 0; d < DH; ++d) o[d] = 0.f;
#pragma unroll
    for (int j = 0; j < T; ++j)
#pragma unroll
        for (int d = 0; d < DH; d += 4) {
            const float4 vv = *reinterpret_cast<const float4*>(&Vs[wave][j * DH + d]);
            o[d] = fmaf(s[j], vv.x, o[d]); o[d + 1] = fmaf(s[j], vv.y, o[d + 1]);
            o[d + 2] = fmaf(s[j], vv.z, o[d + 2]); o[d + 3] = fmaf(s[j], vv.w, o[d + 3]);
        }
    if (live && lane < T) {
        float* orow = out + ((int64_t)pr.f * H * W + tok) * C + pr.h * DH;
#pragma unroll
        for (int d = 0; d < DH; d += 4) *reinterpret_cast<float4*>(orow + d) = make_float4(o[d], o[d + 1], o[d + 2], o[d + 3]);
    }
}

template <int WS, int DH, int WAVES>
__global__ void __launch_bounds__(64 * WAVES) __attribute__((amdgpu_waves_per_eu(2))) swin_attn_bwd_kernel(const float* __restrict__ qkv, const float* __restrict__ dout,
                                                                   const float* __restrict__ table, float* __restrict__ dqkv, int nprob, int H,
                                                                   int W, int shift, int heads, float scale) {
    constexpr int T = WS * WS, NI = (2 * WS - 1) * (2 * WS - 1);
    constexpr int RS = DH + 4;      // row stride of the token rows in LDS: the per-lane row writes of the second phase spread over the banks
    __shared__ __attribute__((aligned(16))) float As[WAVES][T * RS], Bv[WAVES][T * RS];     // k, then scaled q;  v, then dout
    __shared__ float Ps[WAVES][T * T], Bs[WAVES][NI];              // P, then dS, row i at i * T (T odd or tiny: column reads are consecutive)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int p = blockIdx.x * WAVES + wave;
    const bool live = p < nprob;
    const WinProblem pr = win_problem(live ? p : nprob - 1, heads, H, W, WS);
    const int C = heads * DH;
    const float* base = qkv + (int64_t)pr.f * H * W * 3 * C + pr.h * DH;
    win_stage_kv<WS, DH, RS>(base, C, table, heads, pr, H, W, shift, lane, As[wave], Bv[wave], Bs[wave]);
    const int i = lane < T ? lane : T - 1;
    const bool mine = live && lane < T;
    int y, x;
    const int64_t tok = win_token<WS>(i, pr.wy, pr.wx, H, W, shift, y, x);
    const int reg = shift ? shift_region(y, H, WS, shift) * 3 + shift_region(x, W, WS, shift) : 0;
    float q[DH], g[DH];
    const float* grow = dout + ((int64_t)pr.f * H * W + tok) * C + pr.h * DH;
#pragma unroll
    for (int d = 0; d < DH; d += 4) {
        const float4 v = *reinterpret_cast<const float4*>(base + tok * 3 * C + d);
        q[d] = __fmul_rn(v.x, scale); q[d + 1] = __fmul_rn(v.y, scale); q[d + 2] = __fmul_rn(v.z, scale); q[d + 3] = __fmul_rn(v.w, scale);
        const float4 u = *reinterpret_cast<const float4*>(grow + d);
        g[d] = u.x; g[d + 1] = u.y; g[d + 2] = u.z; g[d + 3] = u.w;
    }
    __syncthreads();
    float s[T], ds[T];
    win_probs<WS, DH, RS>(q, As[wave], Bs[wave], i, reg, shift, s);
    if (lane < T) {                                                // P leaves the registers here: row i is re-read below, columns in phase two
#pragma unroll
        for (int j = 0; j < T; ++j) Ps[wave][i * T + j] = s[j];
    }
    float delta = 0.f;                                             // sum_j dP_ij P_ij
#pragma unroll
    for (int j = 0; j < T; ++j) {
        float a0 = 0.f, a1 = 0.f;
#pragma unroll
        for (int d = 0; d < DH; d += 4) {
            const float4 vv = *reinterpret_cast<const float4*>(&Bv[wave][j * RS + d]);
            a0 = fmaf(g[d], vv.x, a0); a1 = fmaf(g[d + 1], vv.y, a1);
            a0 = fmaf(g[d + 2], vv.z, a0); a1 = fmaf(g[d + 3], vv.w, a1);
        }
        ds[j] = __fadd_rn(a0, a1);
        delta = fmaf(ds[j], s[j], delta);
    }
    float* drow = dqkv + ((int64_t)pr.f * H * W + tok) * 3 * C + pr.h * DH;
    {
        float dq[DH];
#pragma unroll
        for (int d = 0; d < DH; ++d) dq[d] = 0.f;
#pragma unroll
        for (int j = 0; j < T; ++j) {
            ds[j] = __fmul_rn(Ps[wave][i * T + j], __fsub_rn(ds[j], delta));     // dS_ij = P_ij (dP_ij - delta_i)
#pragma unroll
            for (int d = 0; d < DH; d += 4) {
                const float4 kk = *reinterpret_cast<const float4*>(&As[wave][j * RS + d]);
                dq[d] = fmaf(ds[j], kk.x, dq[d]); dq[d + 1] = fmaf(ds[j], kk.y, dq[d + 1]);
                dq[d + 2] = fmaf(ds[j], kk.z, dq[d + 2]); dq[d + 3] = fmaf(ds[j], kk.w, dq[d + 3]);
            }
        }
        if (mine) {
#pragma unroll
            for (int d = 0; d < DH; d += 4)
                *reinterpret_cast<float4*>(drow + d) = make_float4(__fmul_rn(dq[d], scale), __fmul_rn(dq[d + 1], scale),
                                                                   __fmul_rn(dq[d + 2], scale), __fmul_rn(dq[d + 3], scale));
        }
    }
    __syncthreads();                                               // k and v have been read by every lane: their rows now take q and dout
    if (lane < T) {
#pragma unroll
        for (int d = 0; d < DH; d += 4) {                          // q is read again (a cache hit) rather than held through phase one
            const float4 v = *reinterpret_cast<const float4*>(base + tok * 3 * C + d);
            *reinterpret_cast<float4*>(&As[wave][i * RS + d]) = make_float4(__fmul_rn(v.x, scale), __fmul_rn(v.y, scale), __fmul_rn(v.z, scale),
                                                                            __fmul_rn(v.w, scale));
            *reinterpret_cast<float4*>(&Bv[wave][i * RS + d]) = make_float4(g[d], g[d + 1], g[d + 2], g[d + 3]);
        }
    }
    __syncthreads();
    float acc[DH];                                                 // lane j: dv_j = sum_i P_ij dout_i
#pragma unroll
    for (int d = 0; d < DH; ++d) acc[d] = 0.f;
#pragma unroll 7
    for (int r = 0; r < T; ++r) {
        const float pij = Ps[wave][r * T + i];
#pragma unroll
        for (int d = 0; d < DH; d += 4) {
            const float4 u = *reinterpret_cast<const float4*>(&Bv[wave][r * RS + d]);
            acc[d] = fmaf(pij, u.x, acc[d]); acc[d + 1] = fmaf(pij, u.y, acc[d + 1]);
            acc[d + 2] = fmaf(pij, u.z, acc[d + 2]); acc[d + 3] = fmaf(pij, u.w, acc[d + 3]);
        }
    }
    if (mine) {
#pragma unroll
        for (int d = 0; d < DH; d += 4) *reinterpret_cast<float4*>(drow + 2 * C + d) = make_float4(acc[d], acc[d + 1], acc[d + 2], acc[d + 3]);
    }
    __syncthreads();
    if (lane < T) {
#pragma unroll
        for (int j = 0; j < T; ++j) Ps[wave][i * T + j] = ds[j];
    }
    __syncthreads();
#pragma unroll
    for (int d = 0; d < DH; ++d) acc[d] = 0.f;                     // lane j: dk_j = sum_i dS_ij (scale q_i)
#pragma unroll 7
    for (int r = 0; r < T; ++r) {
        const float sij = Ps[wave][r * T + i];
#pragma unroll
        for (int d = 0; d < DH; d += 4) {
            const float4 u = *reinterpret_cast<const float4*>(&As[wave][r * RS + d]);
            acc[d] = fmaf(sij, u.x, acc[d]); acc[d + 1] = fmaf(sij, u.y, acc[d + 1]);
            acc[d + 2] = fmaf(sij, u.z, acc[d + 2]); acc[d + 3] = fmaf(sij, u.w, acc[d + 3]);
        }
    }
    if (mine) {
#pragma unroll
        for (int d = 0; d < DH; d += 4) *reinterpret_cast<float4*>(drow + C + d) = make_float4(acc[d], acc[d + 1], acc[d + 2], acc[d + 3]);
    }
}

// fine token (f, y, x) of (F, H, W, C) <-> quarter (y & 1) + 2 (x & 1) of merged row (f, y / 2, x / 2) of (F, H/2, W/2, 4C); one thread per
// four channels.  scatter = 0: out[merged] = x[fine];  scatter = 1: out[fine] = x[merged] (+ add[fine])
__global__ void __launch_bounds__(256) swin_merge_kernel(const float* __restrict__ in, float* out, int F, int H, int W, int C, const float* add,
                                                         int scatter) {        // `add` may be `out` itself (each element: same thread)
    const int c4n = C / 4;
    const int64_t total = (int64_t)F * H * W * c4n;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
        const int c = (int)(e % c4n) * 4;
        int64_t rest = e / c4n;
        const int x = (int)(rest % W); rest /= W;
        const int y = (int)(rest % H);
        const int64_t f = rest / H;
        const int64_t fine = ((f * H + y) * W + x) * C + c;
        const int64_t merged = ((f * (H / 2) + y / 2) * (W / 2) + x / 2) * (4LL * C) + ((y & 1) + 2 * (x & 1)) * C + c;
        if (scatter) {
            float4 v = *reinterpret_cast<const float4*>(in + merged);
            if (add) {
                const float4 a = *reinterpret_cast<const float4*>(add + fine);
                v.x = __fadd_rn(v.x, a.x); v.y = __fadd_rn(v.y, a.y); v.z = __fadd_rn(v.z, a.z); v.w = __fadd_rn(v.w, a.w);
            }
            *reinterpret_cast<float4*>(out + fine) = v;
        } else {
            *reinterpret_cast<float4*>(out + merged) = *reinterpret_cast<const float4*>(in + fine);
        }
    }
}

inline bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

int attn_args(const char* who, const void* a, const void* b, const void* c, const void* table, int F, int H, int W, int ws, int shift,
              int heads, int dh) {
    char buf[256];
    if (!a || !b || !c || !table) {
        snprintf(buf, sizeof buf, "%s: null argument", who);
        return i2v_api_fail(buf);
    }
    if (F <= 0 || heads <= 0 || H <= 0 || W <= 0 || H % ws != 0 || W % ws != 0 || shift < 0 || shift >= ws ||
        (shift != 0 && (H <= ws || W <= ws)) || !((ws == 7 && dh == 32) || (ws == 4 && dh == 16)) ||
        (int64_t)F * (H / ws) * (W / ws) * heads > 0x7fffffff) {
        snprintf(buf, sizeof buf, "%s: unsupported shape (frames %d grid %d x %d window %d shift %d heads %d head width %d): window 7 with "
                 "head width 32 or window 4 with head width 16, a grid of whole windows, 0 <= shift < window, no shift on a one-window grid",
                 who, F, H, W, ws, shift, heads, dh);
        return i2v_api_fail(buf);
    }
    if (!al16(a) || !al16(b) || !al16(c)) {
        snprintf(buf, sizeof buf, "%s: 16-byte alignment needed", who);
        return i2v_api_fail(buf);
    }
    return 0;
}

constexpr int FWD_WAVES = 4, BWD_WAVES = 2;

}  // namespace

int swin_window_attention(const float* qkv, int F, int H, int W, int ws, int shift, int heads, int dh, const float* table, float* out,
                          hipStream_t s) {
    if (attn_args("swin_window_attention", qkv, out, out, table, F, H, W, ws, shift, heads, dh) != 0) return 1;
    const int nprob = F * (H / ws) * (W / ws) * heads;
    const dim3 grid((unsigned)((nprob + FWD_WAVES - 1) / FWD_WAVES)), block(64 * FWD_WAVES);
    const float scale = 1.f / sqrtf((float)dh);
    if (ws == 7) hipLaunchKernelGGL((swin_attn_fwd_kernel<7, 32, FWD_WAVES>), grid, block, 0, s, qkv, table, out, nprob, H, W, shift, heads, scale);
    else hipLaunchKernelGGL((swin_attn_fwd_kernel<4, 16, FWD_WAVES>), grid, block, 0, s, qkv, table, out, nprob, H, W, shift, heads, scale);
    return vit_launch_check("swin_window_attention");
}

int swin_window_attention_bwd(const float* qkv, const float* dout, int F, int H, int W, int ws, int shift, int heads, int dh,
                              const float* table, float* dqkv, hipStream_t s) {
    if (attn_args("swin_window_attention_bwd", qkv, dout, dqkv, table, F, H, W, ws, shift, heads, dh) != 0) return 1;
    const int nprob = F * (H / ws) * (W / ws) * heads;
    const dim3 grid((unsigned)((nprob + BWD_WAVES - 1) / BWD_WAVES)), block(64 * BWD_WAVES);
    const float scale = 1.f / sqrtf((float)dh);
    if (ws == 7) hipLaunchKernelGGL((swin_attn_bwd_kernel<7, 32, BWD_WAVES>), grid, block, 0, s, qkv, dout, table, dqkv, nprob, H, W, shift, heads, scale);
    else hipLaunchKernelGGL((swin_attn_bwd_kernel<4, 16, BWD_WAVES>), grid, block, 0, s, qkv, dout, table, dqkv, nprob, H, W, shift, heads, scale);
    return vit_launch_check("swin_window_attention_bwd");
}

static int merge_launch(const char* who, const float* in, float* out, int F, int H, int W, int C, const float* add, int scatter, hipStream_t s) {
    char buf[160];
    if (!in || !out) {
        snprintf(buf, sizeof buf, "%s: null argument", who);
        return i2v_api_fail(buf);
    }
    if (F <= 0 || H <= 0 || W <= 0 || H % 2 != 0 || W % 2 != 0 || C <= 0 || C % 4 != 0 || !al16(in) || !al16(out) || (add && !al16(add))) {
        snprintf(buf, sizeof buf, "%s: an even grid, C %% 4 == 0 and 16-byte alignment needed", who);
        return i2v_api_fail(buf);
    }
    const int64_t n = (int64_t)F * H * W * (C / 4);
    const unsigned grid = (unsigned)std::min<int64_t>((n + 255) / 256, 65536);
    hipLaunchKernelGGL(swin_merge_kernel, dim3(grid), dim3(256), 0, s, in, out, F, H, W, C, add, scatter);
    return vit_launch_check(who);
}

int swin_merge_gather(const float* x, int F, int H, int W, int C, float* out, hipStream_t s) {
    return merge_launch("swin_merge_gather", x, out, F, H, W, C, nullptr, 0, s);
}

int swin_merge_scatter(const float* dout, int F, int H, int W, int C, const float* add, float* dx, hipStream_t s) {
    return merge_launch("swin_merge_scatter", dout, dx, F, H, W, C, add, 1, s);
}
