// Talking-heads attention of a CaiT self-attention block for gfx950 (timm's `TalkingHeadAttn`; CaitAttn, i2v_cait_kernels.h), forward and
// input gradient, and the plain `+ pos_embed` launch of the CaiT stem.
//
// FORWARD, one launch.  One workgroup (4 waves) owns one frame, one tile of 16 query rows and ALL H heads.  Its LDS holds the H score
// tiles, H x 16 rows x ldk floats (ldk = T rounded up to 16, plus 4: 212 for 196 keys, 106 KiB at 8 heads), and every step works on them
// in place -- the scores never reach memory:
//   1. S_h = (scale q_h) k_h^T by v_mfma_f32_16x16x4_f32 into LDS, one 16 x 16 tile per (head, key tile), operands straight from qkv
//   2. S'_g = sum_h wl[g][h] S_h + bl[g]: the thread that owns a (row, key) position reads its H values and writes H back
//   3. P_g = softmax over the keys, one wave per (head, row); P goes to memory here, post-softmax and pre-mix
//   4. P'_g = sum_h ww[g][h] P_h + bw[g], as step 2
//   5. out_g = P'_g v_g by the same MFMA, A from LDS, B from qkv
// Rows and keys beyond T are zero operands: the tail tile is padded in LDS, never in memory.
//
// BACKWARD, two launches, no atomics and no sum split across workgroups: every output element has one owner.
//   row-tile launch (same ownership as the forward):
//     1. dP'_g = dout_g v_g^T into LDS | 2. dP_h = sum_g ww[g][h] dP'_g in place, and P'_g (as forward step 4, from P in memory) -> Pm
//     3. dS'_g = P_g * (dP_g - sum_j dP_g P_g), one wave per (head, row) | 4. dS_h = sum_g wl[g][h] dS'_g in place and -> dS
//     5. dq_h = scale * (dS_h k_h)
//   key-tile launch (one frame, 16 keys, all heads): dk_h = scale * (dS_h^T q_h), dv_g = Pm_g^T dout_g, A read down the columns of dS / Pm.
//
// ORDER OF EVERY SUM (include/i2v_cait.h states it as the contract; -ffp-contract=off, every fma written out):
//   * a product element is ONE fp32 fma chain from 0 (the fp32 MFMA is bitwise an fmaf chain, four k per instruction in order).  Over the
//     head width (steps 1 of both passes) and over the keys (steps 5) the contracted index is walked in chunks of 16, and inside a chunk in
//     the order 0 4 8 12 | 1 5 9 13 | 2 6 10 14 | 3 7 11 15 -- a lane loads four consecutive floats and feeds one to each of four MFMAs;
//     a chunk that reaches past the end is filled with zero operands.  Over the query rows (key-tile launch) the order is increasing.
//   * a head mix is acc = 0, acc = fma(w[g][h], x_h, acc) for h (backward: g) increasing, then + bias[g].
//   * a row sum (softmax denominator, sum_j dP P): lane l adds its keys l, l + 64, l + 128, ... in increasing order from 0, then the 64
//     partial sums meet in a butterfly over lane distances 32, 16, 8, 4, 2, 1.  P = exp(S' - max) * (1 / sum).
//   * q is multiplied by scale when it is loaded; dq and dk are scale * the finished chain.
// A workgroup reads and writes its own frame only, and nothing depends on the grid: frame 0 of an n-frame call has the bits of a
// 1-frame call, and reruns repeat the bits.
//
// LDS traffic: score tiles are written by ds_write_b32 (16 consecutive keys per quarter-wave; rows 4 apart land 16 banks apart because
// ldk = 4 mod 8), mixed by ds_read_b32 / ds_write_b32 with consecutive lanes on consecutive keys, and read as MFMA operands by
// ds_read_b128.  Stores to memory are vector stores, each element by the one lane that owns it.
#include "i2v_be.h"
#include "i2v_cait_kernels.h"
#include "i2v_vit_kernels.h"     // vit_launch_check

long long g_stat_cait = 0;

namespace {

constexpr int RT = CAIT_TILE;

__device__ __forceinline__ float cait_wsum(float v) {
    for (int o = 32; o > 0; o >>= 1) v = __fadd_rn(v, __shfl_xor(v, o));
    return v;
}
__device__ __forceinline__ float cait_wmax(float v) {
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    return v;
}

struct Geom {
    int T, H, dh, Tp, ldk, row0, wave, r, g;      // r = lane & 15, g = lane >> 4
};

__device__ __forceinline__ Geom geom(const CaitAttn& p) {
    Geom q;
    q.T = p.T; q.H = p.H; q.dh = p.dh;
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

// LDS tile h (16 rows, keys 0 .. Tp) = (alpha * A_h) B_h^T over the head width: A, B are token rows of this frame at row strides sa, sb
// with head h at column h dh; rows of A from row0, rows of B are the keys
__device__ __forceinline__ void scores_to_lds(const float* __restrict__ A, int64_t sa, const float* __restrict__ B, int64_t sb, float alpha,
                                              float* S, const Geom& q) {
    const int NT = q.Tp / RT;
    const int arow = q.row0 + q.r;
    const bool aok = arow < q.T;
    for (int t = q.wave; t < q.H * NT; t += 4) {
        const int h = t / NT, n = t - h * NT;
        const int key = n * RT + q.r;
        const bool bok = key < q.T;
        const float* ap = A + (int64_t)(aok ? arow : 0) * sa + h * q.dh;
        const float* bp = B + (int64_t)(bok ? key : 0) * sb + h * q.dh;
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
        float* o = S + (h * RT + 4 * q.g) * q.ldk + n * RT + q.r;         // acc[i]: row 4 g + i, key n * 16 + r
#pragma unroll
        for (int i = 0; i < 4; ++i) o[i * q.ldk] = acc[i];
    }
}

// O_h (16 rows from row0, dh columns) = alpha * (LDS tile h . B_h) over the keys: B rows are the keys of this frame at row stride sb;
// written to O at row stride so, head h at column h dh.  The LDS tile must hold zeros at keys T .. Tp.
__device__ __forceinline__ void lds_times_rows(const float* S, const float* __restrict__ B, int64_t sb, float alpha, float* __restrict__ O,
                                               int64_t so, const Geom& q) {
    const int ND = (q.dh + RT - 1) / RT;
    for (int t = q.wave; t < q.H * ND; t += 4) {
        const int h = t / ND, d0 = (t - h * ND) * RT;
        const bool dok = d0 + q.r < q.dh;
        const float* sp = S + (h * RT + q.r) * q.ldk + 4 * q.g;
        const float* bp = B + h * q.dh + d0 + q.r;
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
            if (row < q.T) O[(int64_t)row * so + h * q.dh + d0 + q.r] = __fmul_rn(alpha, acc[i]);
        }
    }
}

// y_g = sum_h w[g][h] x_h (+ bias[g]); TR: y_h = sum_g w[g][h] x_g (the transposed mix of the backward pass, no bias)
template <int HM, bool TR>
__device__ __forceinline__ void head_mix(const float (&x)[HM], int H, const float* __restrict__ w, const float* __restrict__ bias, float (&y)[HM]) {
#pragma unroll
    for (int g = 0; g < HM; ++g) {
        y[g] = 0.f;
        if (g < H) {
            float acc = 0.f;
#pragma unroll
            for (int h = 0; h < HM; ++h)
                if (h < H) acc = __builtin_fmaf(TR ? w[h * H + g] : w[g * H + h], x[h], acc);
            y[g] = bias ? __fadd_rn(acc, bias[g]) : acc;
        }
    }
}

// the H tiles mixed in place, position by position; keys T .. Tp become zeros
template <int HM, bool TR>
__device__ __forceinline__ void mix_lds(float* S, const float* __restrict__ w, const float* __restrict__ bias, const Geom& q) {
    for (int pos = threadIdx.x; pos < RT * q.Tp; pos += 256) {
        const int row = pos / q.Tp, key = pos - row * q.Tp;
        float* sp = S + row * q.ldk + key;
        float x[HM], y[HM];
#pragma unroll
        for (int h = 0; h < HM; ++h) x[h] = h < q.H ? sp[h * RT * q.ldk] : 0.f;
        head_mix<HM, TR>(x, q.H, w, bias, y);
#pragma unroll
        for (int h = 0; h < HM; ++h)
            if (h < q.H) sp[h * RT * q.ldk] = key < q.T ? y[h] : 0.f;
    }
}

template <int HM>
__global__ void __launch_bounds__(256) cait_attn_fwd_kernel(const CaitAttn p) {
    extern __shared__ __attribute__((aligned(16))) float cait_lds[];
    const Geom q = geom(p);
    const int f = blockIdx.y, C = p.H * p.dh, ld = cait_probs_ld(p.T);
    const float* qkv = p.qkv + (int64_t)f * p.T * 3 * C;
    float* S = cait_lds;
    scores_to_lds(qkv, 3 * C, qkv + C, 3 * C, p.scale, S, q);
    __syncthreads();
    mix_lds<HM, false>(S, p.wl, p.bl, q);
    __syncthreads();
    const int lane = threadIdx.x & 63;
    for (int rr = q.wave; rr < p.H * RT; rr += 4) {                      // rr = head * 16 + row
        float* x = S + rr * q.ldk;
        float m = -INFINITY;
        for (int c = lane; c < p.T; c += 64) m = fmaxf(m, x[c]);
        m = cait_wmax(m);
        float s = 0.f;
        for (int c = lane; c < p.T; c += 64) {
            const float e = expf(__fsub_rn(x[c], m));
            x[c] = e;
            s = __fadd_rn(s, e);
        }
        const float inv = __fdiv_rn(1.f, cait_wsum(s));
        const int h = rr / RT, row = q.row0 + (rr - h * RT);
        float* pr = p.P + (((int64_t)f * p.H + h) * p.T + (row < p.T ? row : 0)) * ld;
        for (int c = lane; c < p.T; c += 64) {
            const float v = __fmul_rn(x[c], inv);
            x[c] = v;
            if (row < p.T) pr[c] = v;
        }
    }
    __syncthreads();
    mix_lds<HM, false>(S, p.ww, p.bw, q);
    __syncthreads();
    lds_times_rows(S, qkv + 2 * C, 3 * C, 1.f, p.out + (int64_t)f * p.T * C, C, q);
}

template <int HM>
__global__ void __launch_bounds__(256) cait_attn_bwd_rows_kernel(const CaitAttn p) {
    extern __shared__ __attribute__((aligned(16))) float cait_lds[];
    const Geom q = geom(p);
    const int f = blockIdx.y, C = p.H * p.dh, ld = cait_probs_ld(p.T);
    const float* qkv = p.qkv + (int64_t)f * p.T * 3 * C;
    const int64_t hs = (int64_t)p.T * ld, fo = (int64_t)f * p.H * hs;   // a head's and this frame's offset in P, Pm and dS
    float* S = cait_lds;
    scores_to_lds(p.dout + (int64_t)f * p.T * C, C, qkv + 2 * C, 3 * C, 1.f, S, q);        // dP'
    __syncthreads();
    for (int pos = threadIdx.x; pos < RT * q.Tp; pos += 256) {           // dP in place; P' -> Pm
        const int rl = pos / q.Tp, key = pos - rl * q.Tp, row = q.row0 + rl;
        const bool ok = row < p.T && key < p.T;
        float* sp = S + rl * q.ldk + key;
        const int64_t o = fo + (int64_t)(ok ? row : 0) * ld + (ok ? key : 0);
        float x[HM], y[HM], pv[HM], pm[HM];
#pragma unroll
        for (int h = 0; h < HM; ++h) {
            x[h] = h < p.H ? sp[h * RT * q.ldk] : 0.f;
            pv[h] = (h < p.H && ok) ? p.P[o + h * hs] : 0.f;
        }
        head_mix<HM, true>(x, p.H, p.ww, nullptr, y);
        head_mix<HM, false>(pv, p.H, p.ww, p.bw, pm);
#pragma unroll
        for (int h = 0; h < HM; ++h)
            if (h < p.H) {
                sp[h * RT * q.ldk] = ok ? y[h] : 0.f;
                if (ok) p.Pm[o + h * hs] = pm[h];
            }
    }
    __syncthreads();
    const int lane = threadIdx.x & 63;
    for (int rr = q.wave; rr < p.H * RT; rr += 4) {                      // dS' = P (dP - sum_j dP P) in place
        float* x = S + rr * q.ldk;
        const int h = rr / RT, row = q.row0 + (rr - h * RT);
        if (row >= p.T) continue;                                        // (the row holds zeros already; uniform over the wave)
        const float* pr = p.P + fo + h * hs + (int64_t)row * ld;
        float s = 0.f;
        for (int c = lane; c < p.T; c += 64) s = __fadd_rn(s, __fmul_rn(x[c], pr[c]));
        s = cait_wsum(s);
        for (int c = lane; c < p.T; c += 64) x[c] = __fmul_rn(pr[c], __fsub_rn(x[c], s));
    }
    __syncthreads();
    for (int pos = threadIdx.x; pos < RT * q.Tp; pos += 256) {           // dS in place and -> dS
        const int rl = pos / q.Tp, key = pos - rl * q.Tp, row = q.row0 + rl;
        const bool ok = row < p.T && key < p.T;
        float* sp = S + rl * q.ldk + key;
        const int64_t o = fo + (int64_t)(ok ? row : 0) * ld + (ok ? key : 0);
        float x[HM], y[HM];
#pragma unroll
        for (int h = 0; h < HM; ++h) x[h] = h < p.H ? sp[h * RT * q.ldk] : 0.f;
        head_mix<HM, true>(x, p.H, p.wl, nullptr, y);
#pragma unroll
        for (int h = 0; h < HM; ++h)
            if (h < p.H) {
                sp[h * RT * q.ldk] = ok ? y[h] : 0.f;
                if (ok) p.dS[o + h * hs] = y[h];
            }
    }
    __syncthreads();
    lds_times_rows(S, qkv + C, 3 * C, p.scale, p.dqkv + (int64_t)f * p.T * 3 * C, 3 * C, q);   // dq
}

// dk_h = scale * (dS_h^T q_h) and dv_g = Pm_g^T dout_g for 16 keys of one frame: one wave per (which, head, 16 columns) tile, the
// whole row index walked by that wave in increasing order
__global__ void __launch_bounds__(256) cait_attn_bwd_keys_kernel(const CaitAttn p) {
    const int f = blockIdx.y, C = p.H * p.dh, ld = cait_probs_ld(p.T);
    const int key0 = blockIdx.x * RT, wave = threadIdx.x >> 6, r = threadIdx.x & 15, g = (threadIdx.x >> 4) & 3;
    const int ND = (p.dh + RT - 1) / RT;
    const int64_t hs = (int64_t)p.T * ld, fo = (int64_t)f * p.H * hs;
    const float* qkv = p.qkv + (int64_t)f * p.T * 3 * C;
    const float* dout = p.dout + (int64_t)f * p.T * C;
    float* dqkv = p.dqkv + (int64_t)f * p.T * 3 * C;
    const bool kok = key0 + r < p.T;
    for (int t = wave; t < 2 * p.H * ND; t += 4) {
        const int which = t / (p.H * ND), u = t - which * p.H * ND, h = u / ND, d0 = (u - h * ND) * RT;
        const bool dok = d0 + r < p.dh;
        const float* ap = (which ? p.Pm : p.dS) + fo + h * hs + (kok ? key0 + r : 0);      // A[m = key][k = row]: down a column
        const float* bp = (which ? dout : qkv) + h * p.dh + (dok ? d0 + r : 0);            // B[k = row][n = column]
        const int64_t sb = which ? C : 3 * C;
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        for (int k0 = 0; k0 < p.T; k0 += 4) {
            const int row = k0 + g;
            const bool rok = row < p.T;
            const float a = (rok && kok) ? ap[(int64_t)row * ld] : 0.f;
            const float b = (rok && dok) ? bp[(int64_t)row * sb] : 0.f;
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, acc, 0, 0, 0);
        }
        if (!dok) continue;
        const float alpha = which ? 1.f : p.scale;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int key = key0 + 4 * g + i;
            if (key < p.T) dqkv[(int64_t)key * 3 * C + (which ? 2 * C : C) + h * p.dh + d0 + r] = __fmul_rn(alpha, acc[i]);
        }
    }
}

__global__ void __launch_bounds__(256) cait_add_pos_kernel(float* __restrict__ x, const float* __restrict__ pos, int F, int T, int C) {
    const int c4n = C / 4;
    const int64_t per = (int64_t)T * c4n, total = (int64_t)F * per;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
        const float4 a = *reinterpret_cast<const float4*>(x + 4 * e), b = *reinterpret_cast<const float4*>(pos + 4 * (e % per));
        *reinterpret_cast<float4*>(x + 4 * e) = make_float4(__fadd_rn(a.x, b.x), __fadd_rn(a.y, b.y), __fadd_rn(a.z, b.z), __fadd_rn(a.w, b.w));
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
    const hipError_t e = hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, CAIT_LDS_MAX);
    if (e == hipSuccess) return 0;
    char buf[256];
    snprintf(buf, sizeof buf, "%s: hipFuncSetAttribute(MaxDynamicSharedMemorySize): %s", who, hipGetErrorString(e));
    return i2v_api_fail(buf);
}

}  // namespace

int cait_attention(const CaitAttn& p, hipStream_t s) {
    const char* who = "cait_attention";
    if (const char* why = cait_attn_refusal(p, false)) return refuse(who, why);
    const int64_t lds = cait_lds_bytes(p.T, p.H);
    const dim3 grid((unsigned)((p.T + RT - 1) / RT), (unsigned)p.F);
    __atomic_fetch_add(&g_stat_cait, 1, __ATOMIC_RELAXED);
    if (p.H <= 4) {
        if (raise_lds(cait_attn_fwd_kernel<4>, lds, who)) return 1;
        hipLaunchKernelGGL((cait_attn_fwd_kernel<4>), grid, dim3(256), (size_t)lds, s, p);
    } else if (p.H <= 8) {
        if (raise_lds(cait_attn_fwd_kernel<8>, lds, who)) return 1;
        hipLaunchKernelGGL((cait_attn_fwd_kernel<8>), grid, dim3(256), (size_t)lds, s, p);
    } else {
        if (raise_lds(cait_attn_fwd_kernel<16>, lds, who)) return 1;
        hipLaunchKernelGGL((cait_attn_fwd_kernel<16>), grid, dim3(256), (size_t)lds, s, p);
    }
    return vit_launch_check(who);
}

int cait_attention_bwd(const CaitAttn& p, hipStream_t s) {
    const char* who = "cait_attention_bwd";
    if (const char* why = cait_attn_refusal(p, true)) return refuse(who, why);
    const int64_t lds = cait_lds_bytes(p.T, p.H);
    const dim3 grid((unsigned)((p.T + RT - 1) / RT), (unsigned)p.F);
    __atomic_fetch_add(&g_stat_cait, 2, __ATOMIC_RELAXED);
    if (p.H <= 4) {
        if (raise_lds(cait_attn_bwd_rows_kernel<4>, lds, who)) return 1;
        hipLaunchKernelGGL((cait_attn_bwd_rows_kernel<4>), grid, dim3(256), (size_t)lds, s, p);
    } else if (p.H <= 8) {
        if (raise_lds(cait_attn_bwd_rows_kernel<8>, lds, who)) return 1;
        hipLaunchKernelGGL((cait_attn_bwd_rows_kernel<8>), grid, dim3(256), (size_t)lds, s, p);
    } else {
        if (raise_lds(cait_attn_bwd_rows_kernel<16>, lds, who)) return 1;
        hipLaunchKernelGGL((cait_attn_bwd_rows_kernel<16>), grid, dim3(256), (size_t)lds, s, p);
    }
    if (vit_launch_check(who)) return 1;
    hipLaunchKernelGGL(cait_attn_bwd_keys_kernel, grid, dim3(256), 0, s, p);
    return vit_launch_check(who);
}

int cait_add_pos(float* x, const float* pos, int F, int T, int C, hipStream_t s) {
    if (!x || !pos || F <= 0 || T <= 0 || C <= 0 || C % 4 != 0 || (((uintptr_t)x | (uintptr_t)pos) & 15))
        return refuse("cait_add_pos", "C % 4 == 0 and 16-byte alignment needed");
    const int64_t n = (int64_t)F * T * (C / 4);
    hipLaunchKernelGGL(cait_add_pos_kernel, dim3((unsigned)std::min<int64_t>((n + 255) / 256, 65536)), dim3(256), 0, s, x, pos, F, T, C);
    return vit_launch_check("cait_add_pos");
}
