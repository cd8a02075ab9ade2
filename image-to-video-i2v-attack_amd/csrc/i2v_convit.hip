// Gated positional self-attention of a ConViT block for gfx950 (timm's `GPSA`; ConvitAttn, i2v_convit_kernels.h), forward and input
// gradient, and the two launches that let the class token join the stream in mid-stack.
//
// FORWARD, one launch.  One workgroup (4 waves) owns one frame, ONE head and one tile of 16 query rows.  Its LDS holds that head's score
// tile, 16 rows x ldk floats (ldk = T rounded up to 16, plus 4: 212 for 196 keys, 13.5 KiB, so many workgroups share a CU), and every
// step works on it in place -- the scores never reach memory:
//   1. S = (scale q) k^T by v_mfma_f32_16x16x4_f32 into LDS, one wave per 16 x 16 key tile, operands straight from qkv
//   2. Ppatch = softmax over the keys, one wave per row; Ppatch goes to memory here
//   3. P = fma(c_h, Ppatch, table_h[row][key]) in place, in the same pass of the same lane (no table: P = Ppatch)
//   4. out = P v by the same MFMA, A from LDS, B from qkv
// Rows and keys beyond T are zero operands: the tail tile is padded in LDS, never in memory.  Nothing is divided: the table carries
// sigma(g) Ppos and c = 1 - sigma(g), so a row of P sums to one and timm's renormalisation is a division by one.
//
// BACKWARD, two launches, no atomics and no sum split across workgroups: every output element has one owner.
//   row-tile launch (same ownership as the forward):
//     1. dP = dout v^T into LDS | 2. dS = Ppatch * (c dP - sum_j c dP Ppatch), one wave per row, in place and -> dS | 3. dq = scale * (dS k)
//   key-tile launch (one frame, one head, 16 keys): dk = scale * (dS^T q), dv = P^T dout with P re-formed from Ppatch, c and the table as
//   it is read, A read down the columns.
//
// ORDER OF EVERY SUM (include/i2v_convit.h states it as the contract; -ffp-contract=off, every fma written out):
//   * a product element is ONE fp32 fma chain from 0 (the fp32 MFMA is bitwise an fmaf chain, four k per instruction in order).  Over the
//     head width (steps 1 of both passes) and over the keys (out, dq) the contracted index is walked in chunks of 16, and inside a chunk in
//     the order 0 4 8 12 | 1 5 9 13 | 2 6 10 14 | 3 7 11 15 -- a lane loads four consecutive floats and feeds one to each of four MFMAs;
//     a chunk that reaches past the end is filled with zero operands.  Over the query rows (key-tile launch) the order is increasing.
//   * a row sum (softmax denominator, sum_j c dP Ppatch): lane l adds its keys l, l + 64, l + 128, ... in increasing order from 0, then the
//     64 partial sums meet in a butterfly over lane distances 32, 16, 8, 4, 2, 1.  Ppatch = exp(S - max) * (1 / sum).
//   * the blend is one fma(c, Ppatch, table) per element; c dP is one rounded product, taken before the row sum.
//   * q is multiplied by scale when it is loaded; dq and dk are scale * the finished chain.
// A workgroup reads and writes its own frame only, and nothing depends on the grid: frame 0 of an n-frame call has the bits of a
// 1-frame call, and reruns repeat the bits.  Stores to memory are vector stores, each element by the one lane that owns it.
#include "i2v_be.h"
#include "i2v_convit_kernels.h"
#include "i2v_vit_kernels.h"     // vit_launch_check

long long g_stat_convit = 0;

namespace {

constexpr int RT = CONVIT_TILE;

__device__ __forceinline__ float cv_wsum(float v) {
    for (int o = 32; o > 0; o >>= 1) v = __fadd_rn(v, __shfl_xor(v, o));
    return v;
}
__device__ __forceinline__ float cv_wmax(float v) {
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    return v;
}

struct Geom {
    int T, dh, Tp, ldk, row0, wave, r, g;      // r = lane & 15, g = lane >> 4
};

__device__ __forceinline__ Geom geom(const ConvitAttn& p) {
    Geom q;
    q.T = p.T; q.dh = p.dh;
    q.Tp = (p.T + RT - 1) / RT * RT;
    q.ldk = q.Tp + 4;
    q.row0 = blockIdx.x * RT;
    q.wave = threadIdx.x >> 6;
    q.r = threadIdx.x & 15;
    q.g = (threadIdx.x >> 4) & 3;
    return q;
}

__device__ __forceinline__ float4 load4_or_zero(const float* p, bool ok) {
    return ok ? *reinterpret_cast<const float4*>(p) : make_float4(0.f, 0.f, 0.f, 0.f);
}

// LDS tile (16 rows, keys 0 .. Tp) = (alpha * A) B^T over the head width: A, B point at this head's columns of token rows of this frame at
// row strides sa, sb; rows of A from row0, rows of B are the keys
__device__ __forceinline__ void scores_to_lds(const float* __restrict__ A, int64_t sa, const float* __restrict__ B, int64_t sb, float alpha,
                                              float* S, const Geom& q) {
    const int NT = q.Tp / RT;
    const int arow = q.row0 + q.r;
    const bool aok = arow < q.T;
    const float* ap = A + (int64_t)(aok ? arow : 0) * sa;
    for (int n = q.wave; n < NT; n += 4) {
        const int key = n * RT + q.r;
        const bool bok = key < q.T;
        const float* bp = B + (int64_t)(bok ? key : 0) * sb;
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        for (int c0 = 0; c0 < q.dh; c0 += 16) {
            const int k = c0 + 4 * q.g;                                   // (dh % 4 == 0: the quad is whole or absent)
            float4 a = load4_or_zero(ap + k, aok && k < q.dh);
            const float4 b = load4_or_zero(bp + k, bok && k < q.dh);
            a.x = __fmul_rn(alpha, a.x); a.y = __fmul_rn(alpha, a.y); a.z = __fmul_rn(alpha, a.z); a.w = __fmul_rn(alpha, a.w);
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, b.x, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, b.y, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, b.z, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, b.w, acc, 0, 0, 0);
        }
        float* o = S + (4 * q.g) * q.ldk + n * RT + q.r;                  // acc[i]: row 4 g + i, key n * 16 + r
#pragma unroll
        for (int i = 0; i < 4; ++i) o[i * q.ldk] = bok ? acc[i] : 0.f;    // keys T .. Tp hold zeros
    }
}

// O (16 rows from row0, dh columns) = alpha * (LDS tile . B) over the keys: B points at this head's columns, rows are the keys of this frame
// at row stride sb; written to O (this head's columns) at row stride so.  The LDS tile must hold zeros at keys T .. Tp.
__device__ __forceinline__ void lds_times_rows(const float* S, const float* __restrict__ B, int64_t sb, float alpha, float* __restrict__ O,
                                               int64_t so, const Geom& q) {
    const int ND = (q.dh + RT - 1) / RT;
    for (int t = q.wave; t < ND; t += 4) {
        const int d0 = t * RT;
        const bool dok = d0 + q.r < q.dh;
        const float* sp = S + q.r * q.ldk + 4 * q.g;
        const float* bp = B + d0 + (dok ? q.r : 0);
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        for (int k0 = 0; k0 < q.Tp; k0 += 16) {
            const float4 a = *reinterpret_cast<const float4*>(sp + k0);
            const int key = k0 + 4 * q.g;
            const float b0 = (dok && key < q.T) ? bp[(int64_t)key * sb] : 0.f;
            const float b1 = (dok && key + 1 < q.T) ? bp[(int64_t)(key + 1) * sb] : 0.f;
            const float b2 = (dok && key + 2 < q.T) ? bp[(int64_t)(key + 2) * sb] : 0.f;
            const float b3 = (dok && key + 3 < q.T) ? bp[(int64_t)(key + 3) * sb] : 0.f;
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, b0, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, b1, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, b2, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, b3, acc, 0, 0, 0);
        }
        if (!dok) continue;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int row = q.row0 + 4 * q.g + i;
            if (row < q.T) O[(int64_t)row * so + d0 + q.r] = __fmul_rn(alpha, acc[i]);
        }
    }
}

__global__ void __launch_bounds__(256) convit_attn_fwd_kernel(const ConvitAttn p) {
    extern __shared__ __attribute__((aligned(16))) float convit_lds[];
    const Geom q = geom(p);
    const int f = blockIdx.y, h = blockIdx.z, C = p.H * p.dh, ld = convit_probs_ld(p.T);
    const float* qkv = p.qkv + (int64_t)f * p.T * 3 * C + h * p.dh;
    float* S = convit_lds;
    scores_to_lds(qkv, 3 * C, qkv + C, 3 * C, p.scale, S, q);
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const float cv = p.c ? p.c[h] : 1.f;
    for (int rl = q.wave; rl < RT; rl += 4) {
        const int row = q.row0 + rl;
        if (row >= p.T) continue;                                        // (the row holds zeros: zero operands; uniform over the wave)
        float* x = S + rl * q.ldk;
        float m = -INFINITY;
        for (int c = lane; c < p.T; c += 64) m = fmaxf(m, x[c]);
        m = cv_wmax(m);
        float s = 0.f;
        for (int c = lane; c < p.T; c += 64) {
            const float e = expf(__fsub_rn(x[c], m));
            x[c] = e;
            s = __fadd_rn(s, e);
        }
        const float inv = __fdiv_rn(1.f, cv_wsum(s));
        float* pr = p.P + (((int64_t)f * p.H + h) * p.T + row) * ld;
        const float* tb = p.table ? p.table + ((int64_t)h * p.T + row) * ld : nullptr;
        for (int c = lane; c < p.T; c += 64) {
            const float v = __fmul_rn(x[c], inv);
            pr[c] = v;
            x[c] = tb ? __builtin_fmaf(cv, v, tb[c]) : v;
        }
    }
    __syncthreads();
    lds_times_rows(S, qkv + 2 * C, 3 * C, 1.f, p.out + (int64_t)f * p.T * C + h * p.dh, C, q);
}

__global__ void __launch_bounds__(256) convit_attn_bwd_rows_kernel(const ConvitAttn p) {
    extern __shared__ __attribute__((aligned(16))) float convit_lds[];
    const Geom q = geom(p);
    const int f = blockIdx.y, h = blockIdx.z, C = p.H * p.dh, ld = convit_probs_ld(p.T);
    const float* qkv = p.qkv + (int64_t)f * p.T * 3 * C + h * p.dh;
    const int64_t ho = ((int64_t)f * p.H + h) * p.T * ld;               // this frame's and head's offset in P and dS
    float* S = convit_lds;
    scores_to_lds(p.dout + (int64_t)f * p.T * C + h * p.dh, C, qkv + 2 * C, 3 * C, 1.f, S, q);        // dP
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const float cv = p.c ? p.c[h] : 1.f;
    for (int rl = q.wave; rl < RT; rl += 4) {                            // dS = Ppatch (c dP - sum_j c dP Ppatch) in place and -> dS
        const int row = q.row0 + rl;
        if (row >= p.T) continue;                                        // (the row holds zeros already; uniform over the wave)
        float* x = S + rl * q.ldk;
        const float* pr = p.P + ho + (int64_t)row * ld;
        float* ds = p.dS + ho + (int64_t)row * ld;
        float s = 0.f;
        for (int c = lane; c < p.T; c += 64) {
            const float d = __fmul_rn(cv, x[c]);
            x[c] = d;
            s = __fadd_rn(s, __fmul_rn(d, pr[c]));
        }
        s = cv_wsum(s);
        for (int c = lane; c < p.T; c += 64) {
            const float v = __fmul_rn(pr[c], __fsub_rn(x[c], s));
            x[c] = v;
            ds[c] = v;
        }
    }
    __syncthreads();
    lds_times_rows(S, qkv + C, 3 * C, p.scale, p.dqkv + (int64_t)f * p.T * 3 * C + h * p.dh, 3 * C, q);   // dq
}

// dk = scale * (dS^T q) and dv = P^T dout for 16 keys of one frame and head: one wave per (which, 16 columns) tile, the whole row index
// walked by that wave in increasing order; P = fma(c, Ppatch, table) re-formed as it is read
__global__ void __launch_bounds__(256) convit_attn_bwd_keys_kernel(const ConvitAttn p) {
    const int f = blockIdx.y, h = blockIdx.z, C = p.H * p.dh, ld = convit_probs_ld(p.T);
    const int key0 = blockIdx.x * RT, wave = threadIdx.x >> 6, r = threadIdx.x & 15, g = (threadIdx.x >> 4) & 3;
    const int ND = (p.dh + RT - 1) / RT;
    const int64_t ho = ((int64_t)f * p.H + h) * p.T * ld;
    const float* qkv = p.qkv + (int64_t)f * p.T * 3 * C + h * p.dh;
    const float* dout = p.dout + (int64_t)f * p.T * C + h * p.dh;
    float* dqkv = p.dqkv + (int64_t)f * p.T * 3 * C + h * p.dh;
    const bool kok = key0 + r < p.T;
    const int kc = kok ? key0 + r : 0;
    const float cv = p.c ? p.c[h] : 1.f;
    const float* tb = p.table ? p.table + (int64_t)h * p.T * ld + kc : nullptr;
    for (int t = wave; t < 2 * ND; t += 4) {
        const int which = t / ND, d0 = (t - which * ND) * RT;
        const bool dok = d0 + r < p.dh;
        const float* ap = (which ? p.P : p.dS) + ho + kc;                                   // A[m = key][k = row]: down a column
        const float* bp = (which ? dout : qkv) + d0 + (dok ? r : 0);                        // B[k = row][n = column]
        const int64_t sb = which ? C : 3 * C;
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        for (int k0 = 0; k0 < p.T; k0 += 4) {
            const int row = k0 + g;
            const bool rok = row < p.T;
            float a = (rok && kok) ? ap[(int64_t)row * ld] : 0.f;
            if (which && tb && rok && kok) a = __builtin_fmaf(cv, a, tb[(int64_t)row * ld]);
            const float b = (rok && dok) ? bp[(int64_t)row * sb] : 0.f;
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, acc, 0, 0, 0);
        }
        if (!dok) continue;
        const float alpha = which ? 1.f : p.scale;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int key = key0 + 4 * g + i;
            if (key < p.T) dqkv[(int64_t)key * 3 * C + (which ? 2 * C : C) + d0 + r] = __fmul_rn(alpha, acc[i]);
        }
    }
}

// out (F, T + 1, C): row 0 of a frame is cls, rows 1 .. T are x's.  BWD: dx row t = dout row t + 1 (+ add row t)
template <bool BWD>
__global__ void __launch_bounds__(256) convit_join_kernel(const float* __restrict__ x, const float* __restrict__ extra, float* __restrict__ out,
                                                          int F, int T, int C) {
    const int c4n = C / 4, To = BWD ? T : T + 1;
    const int64_t total = (int64_t)F * To * c4n;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
        const int c4 = (int)(e % c4n);
        const int64_t rowo = e / c4n, f = rowo / To;
        const int t = (int)(rowo - f * To);
        float4 v;
        if (BWD) {
            v = *reinterpret_cast<const float4*>(x + ((f * (T + 1) + t + 1) * C + 4 * c4));
            if (extra) {
                const float4 a = *reinterpret_cast<const float4*>(extra + (rowo * C + 4 * c4));
                v = make_float4(__fadd_rn(v.x, a.x), __fadd_rn(v.y, a.y), __fadd_rn(v.z, a.z), __fadd_rn(v.w, a.w));
            }
        } else {
            v = t == 0 ? *reinterpret_cast<const float4*>(extra + 4 * c4) : *reinterpret_cast<const float4*>(x + ((f * T + t - 1) * C + 4 * c4));
        }
        *reinterpret_cast<float4*>(out + (rowo * C + 4 * c4)) = v;
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
    const hipError_t e = hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, CONVIT_LDS_MAX);
    if (e == hipSuccess) return 0;
    char buf[256];
    snprintf(buf, sizeof buf, "%s: hipFuncSetAttribute(MaxDynamicSharedMemorySize): %s", who, hipGetErrorString(e));
    return i2v_api_fail(buf);
}

}  // namespace

int convit_attention(const ConvitAttn& p, hipStream_t s) {
    const char* who = "convit_attention";
    if (const char* why = convit_attn_refusal(p, false)) return refuse(who, why);
    const int64_t lds = convit_lds_bytes(p.T);
    const dim3 grid((unsigned)((p.T + RT - 1) / RT), (unsigned)p.F, (unsigned)p.H);
    if (raise_lds(convit_attn_fwd_kernel, lds, who)) return 1;
    __atomic_fetch_add(&g_stat_convit, 1, __ATOMIC_RELAXED);
    hipLaunchKernelGGL(convit_attn_fwd_kernel, grid, dim3(256), (size_t)lds, s, p);
    return vit_launch_check(who);
}

int convit_attention_bwd(const ConvitAttn& p, hipStream_t s) {
    const char* who = "convit_attention_bwd";
    if (const char* why = convit_attn_refusal(p, true)) return refuse(who, why);
    const int64_t lds = convit_lds_bytes(p.T);
    const dim3 grid((unsigned)((p.T + RT - 1) / RT), (unsigned)p.F, (unsigned)p.H);
    if (raise_lds(convit_attn_bwd_rows_kernel, lds, who)) return 1;
    __atomic_fetch_add(&g_stat_convit, 2, __ATOMIC_RELAXED);
    hipLaunchKernelGGL(convit_attn_bwd_rows_kernel, grid, dim3(256), (size_t)lds, s, p);
    if (vit_launch_check(who)) return 1;
    hipLaunchKernelGGL(convit_attn_bwd_keys_kernel, grid, dim3(256), 0, s, p);
    return vit_launch_check(who);
}

static int join_ok(const void* a, const void* b, const void* c, int F, int T, int C) {
    return a && c && F > 0 && T > 0 && C > 0 && C % 4 == 0 && (int64_t)F * (T + 1) * C < (1ll << 31) &&
           !(((uintptr_t)a | (uintptr_t)b | (uintptr_t)c) & 15);
}

int convit_join_cls(const float* x, const float* cls, float* out, int F, int T, int C, hipStream_t s) {
    if (!cls || !join_ok(x, cls, out, F, T, C)) return refuse("convit_join_cls", "C % 4 == 0, fewer than 2^31 elements and 16-byte alignment needed");
    const int64_t n = (int64_t)F * (T + 1) * (C / 4);
    hipLaunchKernelGGL(convit_join_kernel<false>, dim3((unsigned)std::min<int64_t>((n + 255) / 256, 65536)), dim3(256), 0, s, x, cls, out, F, T, C);
    return vit_launch_check("convit_join_cls");
}

int convit_join_cls_bwd(const float* dout, const float* add, float* dx, int F, int T, int C, hipStream_t s) {
    if (!join_ok(dout, add, dx, F, T, C)) return refuse("convit_join_cls_bwd", "C % 4 == 0, fewer than 2^31 elements and 16-byte alignment needed");
    const int64_t n = (int64_t)F * T * (C / 4);
    hipLaunchKernelGGL(convit_join_kernel<true>, dim3((unsigned)std::min<int64_t>((n + 255) / 256, 65536)), dim3(256), 0, s, dout, add, dx, F, T, C);
    return vit_launch_check("convit_join_cls_bwd");
}
