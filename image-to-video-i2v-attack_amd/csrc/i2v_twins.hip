// The Twins launches for gfx950 (i2v_twins_kernels.h): sub-sampled attention (timm's `GlobalSubSampleAttn` between its Linears), forward
// and input gradient, and the s x s block gather / scatter pair that runs the sub-sampling convolution on the shared linear launches.
// Window attention at shift 0 (Twins-SVT's locally-grouped attention) is the Swin launch with a table of zeros.
//
// SUB-SAMPLED ATTENTION.  Many queries, at most 64 keys: one head's whole K and V (TKP = Tk rounded up to 16 rows of DP = dh rounded up to
// 16 columns, at row stride DP + 4) are staged in LDS once per workgroup; rows past Tk and columns past dh are zero operands in LDS, never
// in memory.  A workgroup is 4 waves; a wave owns 16 query rows at a time and the fp32 MFMA (v_mfma_f32_16x16x4_f32) forms every product.
//   FORWARD, grid (query tiles of 256 rows, heads, frames): per step of 64 rows, a wave reads its 16 query rows from memory straight into
//     the A operand (each element once), S = q k^T in up to 4 accumulator tiles (one per 16 keys), the softmax in registers (a row lives in
//     the 16 lanes of one lane group), P through a wave-private LDS tile into the A operand of out = P v.
//   BACKWARD, two launches, P recomputed as above (saving it would cost Tq x Tk floats per head and frame, 3136 x 49 at stage 0 -- more
//     than q and out together -- to spare one of five products):
//     1. dq, same grid: dP = dout v^T as S, dS = scale P (dP - rowsum(dP P)) in registers, dS through LDS, dq = dS k.
//     2. dk / dv, grid (heads, frames): ONE workgroup owns all of a (frame, head)'s dk and dv and walks the query rows in increasing
//        order, 64 per step, q and dout staged in LDS; P and dS of the step go through LDS as the A operands of dv += P^T dout and
//        dk += dS^T q, whose accumulators live across the whole walk (wave w owns the 16 x 16 tiles w, w + 4, ... of each, at most 4).
// ORDER OF EVERY SUM (include/i2v_twins.h states it; -ffp-contract=off):
//   * an element of S or dP is one fp32 fma chain from 0 over the head index in chunks of 16, inside a chunk in the order
//     0 4 8 12 | 1 5 9 13 | 2 6 10 14 | 3 7 11 15 (the fp32 MFMA is bitwise an fmaf chain)
//   * a row maximum, softmax denominator or rowsum(dP P): lane r of the row's group adds its keys r, r + 16, ... in increasing order, then
//     a butterfly over lane distances 8 .. 1;  P = exp(S - max) / sum
//   * an element of out or dq is one chain from 0 over the keys in increasing order; an element of dk or dv one chain from 0 over ALL
//     the queries in increasing order
// Nothing depends on the grid and a workgroup reads and writes its own frame and head only: reruns repeat the bits, and frame 0 of an
// n-frame call has the bits of a 1-frame call.  Every output element has one owner; no atomics; vector-unit stores only.
#include "i2v_be.h"
#include "i2v_swin_kernels.h"
#include "i2v_twins_kernels.h"
#include "i2v_vit_kernels.h"     // vit_launch_check

long long g_stat_twins = 0;

namespace {

constexpr int QROWS = 64, QSTEPS = 4, TW_LDS_MAX = 160 * 1024;
constexpr int pad16(int n) { return (n + 15) / 16 * 16; }

__device__ __forceinline__ float grp_sum(float v) {
    for (int o = 8; o > 0; o >>= 1) v = v + __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ float grp_max(float v) {
    for (int o = 8; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    return v;
}
__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }

// LDS tile (`rows` rows, DP columns at row stride ldm) = rows r0 .. r0 + rows of X (row stride sx), columns 0 .. dh; zero past R and dh
__device__ __forceinline__ void stage_rows(const float* __restrict__ X, int64_t sx, int r0, int R, int rows, int dh, int DP, int ldm,
                                           float* tile) {
    const int q4 = DP / 4;
    for (int e = threadIdx.x; e < rows * q4; e += 256) {
        const int row = e / q4, c = 4 * (e - row * q4);
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (r0 + row < R && c < dh) v = ld4(X + (int64_t)(r0 + row) * sx + c);      // (dh % 4 == 0: the quad is whole or absent)
        *reinterpret_cast<float4*>(tile + row * ldm + c) = v;
    }
}

// acc[nt] = the 16 x 16 tile nt of A M^T: row r of A is `arow` (this lane's row, dh floats; null: a row of zeros), M an LDS tile of
// 16 NT rows.  acc[nt][i]: row 4 g + i of the wave's 16, column 16 nt + r
__device__ __forceinline__ void rows_times_mt(const float* arow, const float* M, int NT, int dh, int DP, int ldm, f32x4 (&acc)[4]) {
    const int r = threadIdx.x & 15, g = (threadIdx.x >> 4) & 3;
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) acc[nt] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int k0 = 0; k0 < DP; k0 += 16) {
        const int c = k0 + 4 * g;
        const float4 a = (arow && c < dh) ? ld4(arow + c) : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) {
            if (nt >= NT) continue;                                        // (uniform over the workgroup)
            const float4 b = ld4(M + (16 * nt + r) * ldm + c);
            acc[nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, b.x, acc[nt], 0, 0, 0);
            acc[nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, b.y, acc[nt], 0, 0, 0);
            acc[nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, b.z, acc[nt], 0, 0, 0);
            acc[nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, b.w, acc[nt], 0, 0, 0);
        }
    }
}

// S (unscaled, as rows_times_mt leaves it) -> P = softmax over the Tk keys of scale S, in place; keys past Tk get 0
__device__ __forceinline__ void softmax_rows(f32x4 (&acc)[4], int NT, int Tk, float scale) {
    const int r = threadIdx.x & 15;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        float m = -INFINITY;
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) {
            if (nt >= NT) continue;
            acc[nt][i] = acc[nt][i] * scale;
            if (16 * nt + r < Tk) m = fmaxf(m, acc[nt][i]);
        }
        m = grp_max(m);                                                    // (Tk >= 1: key 0 is real, the maximum is finite)
        float sum = 0.f;
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) {
            if (nt >= NT) continue;
            acc[nt][i] = 16 * nt + r < Tk ? expf(acc[nt][i] - m) : 0.f;
            sum = sum + acc[nt][i];
        }
        sum = grp_sum(sum);
#pragma unroll
        for (int nt = 0; nt < 4; ++nt)
            if (nt < NT) acc[nt][i] = acc[nt][i] / sum;
    }
}

// P, dP -> dS = scale P (dP - rowsum(dP P)) into dp
__device__ __forceinline__ void softmax_bwd_rows(const f32x4 (&p)[4], f32x4 (&dp)[4], int NT, float scale) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        float d = 0.f;
#pragma unroll
        for (int nt = 0; nt < 4; ++nt)
            if (nt < NT) d = d + dp[nt][i] * p[nt][i];
        d = grp_sum(d);
#pragma unroll
        for (int nt = 0; nt < 4; ++nt)
            if (nt < NT) dp[nt][i] = scale * (p[nt][i] * (dp[nt][i] - d));
    }
}

// the wave's 16 x TKP tile (rows_times_mt's layout) -> LDS rows at `tile` (row stride ldp); rows at or past `live` are written as zeros
__device__ __forceinline__ void put_rows(const f32x4 (&acc)[4], int NT, int ldp, int live, float* tile) {
    const int r = threadIdx.x & 15, g = (threadIdx.x >> 4) & 3;
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
        if (nt >= NT) continue;
#pragma unroll
        for (int i = 0; i < 4; ++i) tile[(4 * g + i) * ldp + 16 * nt + r] = 4 * g + i < live ? acc[nt][i] : 0.f;
    }
}

// the 16 x 16 tile dt of P M: P the wave's LDS rows (row stride ldp, TKP columns), M an LDS tile of TKP rows (row stride ldm): one chain
// over the keys in increasing order.  [i]: row 4 g + i, column 16 dt + r
__device__ __forceinline__ f32x4 rows_times_m(const float* P, int ldp, const float* M, int ldm, int TKP, int dt) {
    const int r = threadIdx.x & 15, g = (threadIdx.x >> 4) & 3;
    const float* ap = P + r * ldp + g;
    const float* bp = M + g * ldm + 16 * dt + r;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int k = 0; k < TKP; k += 4) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(ap[k], bp[k * ldm], acc, 0, 0, 0);
    return acc;
}

constexpr int64_t tile_lds(int Tk, int dh) {      // the query-tiled launches: K, V, and 16 rows of P per wave
    return (int64_t)(2 * pad16(Tk) * (pad16(dh) + 4) + 4 * 16 * (pad16(Tk) + 4)) * 4;
}
constexpr int64_t walk_lds(int Tk, int dh) {      // the dk / dv launch: K, V, q, dout, and 64 rows each of P and dS
    return (int64_t)((2 * pad16(Tk) + 2 * QROWS) * (pad16(dh) + 4) + 2 * QROWS * (pad16(Tk) + 4)) * 4;
}

// BWD = false: out = softmax(scale q k^T) v.  BWD = true: dq = dS k
template <bool BWD>
__global__ void __launch_bounds__(256) twins_attn_tile_kernel(const TwinsAttn p) {
    extern __shared__ __attribute__((aligned(16))) float tw_lds[];
    const int h = blockIdx.y, f = blockIdx.z, Tq = p.Tq, Tk = p.Tk, dh = p.dh, C = p.H * dh;
    const int DP = pad16(dh), TKP = pad16(Tk), NT = TKP / 16, ND = DP / 16, ldm = DP + 4, ldp = TKP + 4;
    const int wave = threadIdx.x >> 6, r = threadIdx.x & 15, g = (threadIdx.x >> 4) & 3;
    float* Ks = tw_lds;
    float* Vs = Ks + TKP * ldm;
    float* Ps = Vs + TKP * ldm + wave * 16 * ldp;                          // this wave's rows
    const float* kv = p.kv + (int64_t)f * Tk * 2 * C + h * dh;
    stage_rows(kv, 2 * C, 0, Tk, TKP, dh, DP, ldm, Ks);
    stage_rows(kv + C, 2 * C, 0, Tk, TKP, dh, DP, ldm, Vs);
    const int64_t base = (int64_t)f * Tq * C + h * dh;
    const float* q = p.q + base;
    float* dst = (BWD ? p.dq : p.out) + base;
    for (int step = 0; step < QSTEPS; ++step) {
        const int s0 = (blockIdx.x * QSTEPS + step) * QROWS;
        if (s0 >= Tq) break;                                               // (uniform over the workgroup)
        const int q0 = s0 + 16 * wave, row = q0 + r;
        f32x4 acc[4];
        __syncthreads();                                                   // K and V are whole; the previous step's P is consumed
        rows_times_mt(row < Tq ? q + (int64_t)row * C : nullptr, Ks, NT, dh, DP, ldm, acc);
        softmax_rows(acc, NT, Tk, p.scale);
        if (BWD) {
            f32x4 dp[4];
            rows_times_mt(row < Tq ? p.dout + base + (int64_t)row * C : nullptr, Vs, NT, dh, DP, ldm, dp);
            softmax_bwd_rows(acc, dp, NT, p.scale);
            put_rows(dp, NT, ldp, 16, Ps);
        } else {
            put_rows(acc, NT, ldp, 16, Ps);
        }
        __syncthreads();
        for (int dt = 0; dt < ND; ++dt) {
            const f32x4 o = rows_times_m(Ps, ldp, BWD ? Ks : Vs, ldm, TKP, dt);
            const int col = 16 * dt + r;
            if (col >= dh) continue;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int t = q0 + 4 * g + i;
                if (t < Tq) dst[(int64_t)t * C + col] = o[i];
            }
        }
    }
}

__global__ void __launch_bounds__(256) twins_attn_dkv_kernel(const TwinsAttn p) {
    extern __shared__ __attribute__((aligned(16))) float tw_lds[];
    const int h = blockIdx.x, f = blockIdx.y, Tq = p.Tq, Tk = p.Tk, dh = p.dh, C = p.H * dh;
    const int DP = pad16(dh), TKP = pad16(Tk), NT = TKP / 16, ND = DP / 16, ldm = DP + 4, ldp = TKP + 4;
    const int wave = threadIdx.x >> 6, r = threadIdx.x & 15, g = (threadIdx.x >> 4) & 3;
    float* Ks = tw_lds;
    float* Vs = Ks + TKP * ldm;
    float* Qs = Vs + TKP * ldm;
    float* Gs = Qs + QROWS * ldm;
    float* Ps = Gs + QROWS * ldm;
    float* Ds = Ps + QROWS * ldp;
    const float* kv = p.kv + (int64_t)f * Tk * 2 * C + h * dh;
    stage_rows(kv, 2 * C, 0, Tk, TKP, dh, DP, ldm, Ks);
    stage_rows(kv + C, 2 * C, 0, Tk, TKP, dh, DP, ldm, Vs);
    const int64_t base = (int64_t)f * Tq * C + h * dh;
    f32x4 accK[4], accV[4];
#pragma unroll
    for (int n = 0; n < 4; ++n) accK[n] = accV[n] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int s0 = 0; s0 < Tq; s0 += QROWS) {
        __syncthreads();                                                   // the previous step's tiles are consumed
        stage_rows(p.q + base, C, s0, Tq, QROWS, dh, DP, ldm, Qs);
        stage_rows(p.dout + base, C, s0, Tq, QROWS, dh, DP, ldm, Gs);
        __syncthreads();
        f32x4 pr[4], dp[4];
        rows_times_mt(Qs + (16 * wave + r) * ldm, Ks, NT, dh, DP, ldm, pr);
        softmax_rows(pr, NT, Tk, p.scale);
        rows_times_mt(Gs + (16 * wave + r) * ldm, Vs, NT, dh, DP, ldm, dp);
        softmax_bwd_rows(pr, dp, NT, p.scale);
        const int live = Tq - (s0 + 16 * wave);                            // rows past Tq take no part: zeros
        put_rows(pr, NT, ldp, live, Ps + 16 * wave * ldp);
        put_rows(dp, NT, ldp, live, Ds + 16 * wave * ldp);
        __syncthreads();
#pragma unroll
        for (int n = 0; n < 4; ++n) {
            const int tile = wave + 4 * n;
            if (tile >= NT * ND) continue;                                 // (uniform over the wave)
            const int kt = tile / ND, dt = tile - kt * ND;
            const float *pa = Ps + g * ldp + 16 * kt + r, *da = Ds + g * ldp + 16 * kt + r;      // A[m = key][k = query]
            const float *gb = Gs + g * ldm + 16 * dt + r, *qb = Qs + g * ldm + 16 * dt + r;      // B[k = query][n = column]
            for (int k = 0; k < QROWS; k += 4) {
                accV[n] = __builtin_amdgcn_mfma_f32_16x16x4f32(pa[k * ldp], gb[k * ldm], accV[n], 0, 0, 0);
                accK[n] = __builtin_amdgcn_mfma_f32_16x16x4f32(da[k * ldp], qb[k * ldm], accK[n], 0, 0, 0);
            }
        }
    }
    float* dkv = p.dkv + (int64_t)f * Tk * 2 * C + h * dh;
#pragma unroll
    for (int n = 0; n < 4; ++n) {
        const int tile = wave + 4 * n;
        if (tile >= NT * ND) continue;
        const int kt = tile / ND, dt = tile - kt * ND, col = 16 * dt + r;
        if (col >= dh) continue;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int key = 16 * kt + 4 * g + i;
            if (key >= Tk) continue;
            dkv[(int64_t)key * 2 * C + col] = accK[n][i];
            dkv[(int64_t)key * 2 * C + C + col] = accV[n][i];
        }
    }
}

// one thread per channel quad of the plane: a copy (gather) or its inverse (scatter, which may add to what dx holds)
__global__ void __launch_bounds__(256) twins_block_kernel(const float* __restrict__ in, float* __restrict__ out, int F, int H, int W, int C,
                                                          int sr, int scatter, int accumulate) {
    const int c4n = C / 4, Ho = H / sr, Wo = W / sr;
    const int64_t total = (int64_t)F * H * W * c4n;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
        const int c = 4 * (int)(e % c4n);
        const int64_t pos = e / c4n;
        const int x = (int)(pos % W), y = (int)((pos / W) % H);
        const int64_t f = pos / ((int64_t)W * H);
        const int64_t full = pos * C + c, row = (f * Ho + y / sr) * Wo + x / sr;
        const int64_t cell = (row * sr * sr + (y % sr) * sr + x % sr) * C + c;
        if (!scatter) {
            *reinterpret_cast<float4*>(out + cell) = ld4(in + full);
        } else {
            float4 v = ld4(in + cell);
            if (accumulate) {
                const float4 o = ld4(out + full);
                v.x = o.x + v.x; v.y = o.y + v.y; v.z = o.z + v.z; v.w = o.w + v.w;
            }
            *reinterpret_cast<float4*>(out + full) = v;
        }
    }
}

int refuse(const char* who, const char* why) {
    char buf[256];
    snprintf(buf, sizeof buf, "%s: %s: %s", who, hipGetErrorName(hipErrorInvalidValue), why);
    return i2v_api_fail(buf);
}

// the dynamic LDS limit of the dk / dv kernel is raised past the default 64 KiB once per device (a host-side setting of that device),
// not per launch: the launch itself then makes no runtime call but the launch
int raise_walk_lds(const char* who) {
    static bool done[64] = {};      // by device ordinal; a racing second call sets the same attribute again, which is harmless
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) dev = -1;
    if (dev >= 0 && __atomic_load_n(&done[dev], __ATOMIC_ACQUIRE)) return 0;
    const hipError_t e = hipFuncSetAttribute((const void*)twins_attn_dkv_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, TW_LDS_MAX);
    if (e != hipSuccess) {
        char buf[256];
        snprintf(buf, sizeof buf, "%s: hipFuncSetAttribute(MaxDynamicSharedMemorySize): %s", who, hipGetErrorString(e));
        return i2v_api_fail(buf);
    }
    if (dev >= 0) __atomic_store_n(&done[dev], true, __ATOMIC_RELEASE);
    return 0;
}

dim3 tile_grid(const TwinsAttn& p) { return dim3((unsigned)((p.Tq + QROWS * QSTEPS - 1) / (QROWS * QSTEPS)), (unsigned)p.H, (unsigned)p.F); }

}  // namespace

static_assert(tile_lds(TWINS_MAX_TK, TWINS_MAX_DH) <= 64 * 1024, "the query-tiled launches stay under the default LDS limit");
static_assert(walk_lds(TWINS_MAX_TK, TWINS_MAX_DH) <= TW_LDS_MAX, "the widest head with the most keys must fit the LDS");

int twins_attention(const TwinsAttn& p, hipStream_t s) {
    if (const char* why = twins_attn_refusal(p, false)) return refuse("twins_attention", why);
    __atomic_fetch_add(&g_stat_twins, 1, __ATOMIC_RELAXED);
    hipLaunchKernelGGL(twins_attn_tile_kernel<false>, tile_grid(p), dim3(256), (size_t)tile_lds(p.Tk, p.dh), s, p);
    return vit_launch_check("twins_attention");
}

int twins_attention_bwd(const TwinsAttn& p, hipStream_t s) {
    const char* who = "twins_attention_bwd";
    if (const char* why = twins_attn_refusal(p, true)) return refuse(who, why);
    const int64_t lds = walk_lds(p.Tk, p.dh);
    if (lds > 64 * 1024 && raise_walk_lds(who)) return 1;
    __atomic_fetch_add(&g_stat_twins, 2, __ATOMIC_RELAXED);
    hipLaunchKernelGGL(twins_attn_tile_kernel<true>, tile_grid(p), dim3(256), (size_t)tile_lds(p.Tk, p.dh), s, p);
    hipLaunchKernelGGL(twins_attn_dkv_kernel, dim3((unsigned)p.H, (unsigned)p.F), dim3(256), (size_t)lds, s, p);
    return vit_launch_check(who);
}

static int block_launch(const char* who, const float* in, float* out, int F, int H, int W, int C, int sr, int scatter, int accumulate,
                        hipStream_t s) {
    if (const char* why = twins_block_refusal(in, out, F, H, W, C, sr)) return refuse(who, why);
    const int64_t n = (int64_t)F * H * W * (C / 4);
    hipLaunchKernelGGL(twins_block_kernel, dim3((unsigned)std::min<int64_t>((n + 255) / 256, 65536)), dim3(256), 0, s, in, out, F, H, W, C, sr,
                       scatter, accumulate);
    return vit_launch_check(who);
}

int twins_block_gather(const float* x, float* rows, int F, int H, int W, int C, int sr, hipStream_t s) {
    return block_launch("twins_block_gather", x, rows, F, H, W, C, sr, 0, 0, s);
}

int twins_block_scatter(const float* drows, float* dx, int F, int H, int W, int C, int sr, int accumulate, hipStream_t s) {
    return block_launch("twins_block_scatter", drows, dx, F, H, W, C, sr, 1, accumulate, s);
}

int twins_window_attention(const float* qkv, int F, int H, int W, int ws, int heads, int dh, const float* zero_table, float* out,
                           hipStream_t s) {
    const char* why = twins_window_refusal(qkv, out, zero_table, F, H, W, ws, heads, dh);
    if (why) return refuse("twins_window_attention", why);
    return swin_window_attention(qkv, F, H, W, ws, 0, heads, dh, zero_table, out, s);
}

int twins_window_attention_bwd(const float* qkv, const float* dout, int F, int H, int W, int ws, int heads, int dh, const float* zero_table,
                               float* dqkv, hipStream_t s) {
    const char* why = twins_window_refusal(qkv, dout, dqkv, F, H, W, ws, heads, dh);
    if (!why && !zero_table) why = "null argument";
    if (why) return refuse("twins_window_attention_bwd", why);
    return swin_window_attention_bwd(qkv, dout, F, H, W, ws, 0, heads, dh, zero_table, dqkv, s);
}
