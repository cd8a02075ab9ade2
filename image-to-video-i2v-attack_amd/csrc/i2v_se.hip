// Squeeze-and-excitation node (timm `SEModule`: global mean -> 1x1 conv + ReLU -> 1x1 conv + sigmoid -> channel scale) with the block's
// shortcut add and final ReLU, for gfx950 -- forward and input gradient, THREE launches per pass (I2VSeParams, i2v_params.h).
//
// The node is bound by memory: the two matrix products are 2 C rd products per frame next to 3 C HW floats moved, so the kernels are
// laid out for bytes, for a fixed summation order, and for the gate words:
//   * squeeze: ONE wave per (frame, channel) plane.  Lane l owns the elements e of the plane with (e / 4) % 64 == l -- one 16-byte load
//     per step where the planes are 16-byte aligned (HW a multiple of 4), four 4-byte loads otherwise, the SAME elements in the SAME
//     order either way -- adds them in increasing e, and the 64 partial sums fold in a shuffle-down tree.  The backward squeeze is the
//     same reduction over the product of two planes.  No atomics; a block is four such waves and nothing crosses them.
//   * excite: one block per frame.  A sum over the C channels (h forward, dh backward) is a wave's job: lane l runs one fma chain over
//     c = l, l + 64, .. (coalesced rows of w1 / w2t), the same tree folds the lanes; the waves of the block share the rd outputs.  A
//     sum over the rd squeezed channels (s forward, dm backward) is one thread's fma chain per channel c over j = 0 .. rd - 1, again
//     on coalesced rows (which is why fc2's weight is kept transposed).  h / dh pass through LDS between the two halves.
//   * scale: a block is (256 x V consecutive positions of the N x HW run) x (one channel), positions running LINEARLY over frames as in
//     i2v_dwconv.hip, so that a wave owns whole words of the channel's gate row -- V = 4 positions per lane (16-byte loads and stores,
//     eight words per wave, each assembled from eight lanes' nibbles by three xor-shuffles) where the planes are 16-byte aligned, else
//     V = 1 (the ballot is the two words).  No read-modify-write, the same bits whatever the path.
// Arithmetic (-ffp-contract=off: every fma is written, nothing else is contracted): see I2VSeParams.  Nothing depends on the frame
// count, the block size or the run; the scalar host code of i2v_se_host.h performs the same operations in the same order (its expf is
// another implementation, so the two agree to rounding, not bit for bit).
#include "i2v_be.h"

long long g_stat_se = 0;

typedef float se_f4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ float se_tree64(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = v + __shfl_down(v, o, 64);
    return v;
}

// ---- squeeze: out[n][c] = scale * sum_p a[n][c][p] (* b[n][c][p]) ----
template <bool V4, bool PROD>
__global__ void __launch_bounds__(256) se_squeeze_kernel(const I2VSeParams p) {
    const int lane = threadIdx.x & 63, c = blockIdx.x * 4 + (threadIdx.x >> 6), n = blockIdx.y;
    if (c >= p.C) return;                                   // (whole wave)
    const int HW = p.HW;
    const float* a = (PROD ? p.g + (int64_t)n * p.g_nstride : p.x + (int64_t)n * p.x_nstride) + (int64_t)c * HW;
    const float* b = p.x + (int64_t)n * p.x_nstride + (int64_t)c * HW;
    float acc = 0.f;
    for (int e = 4 * lane; e < HW; e += 256) {
        if (V4) {
            const se_f4 u = *(const se_f4*)(a + e);
            if (PROD) {
                const se_f4 w = *(const se_f4*)(b + e);
                acc = acc + u.x * w.x; acc = acc + u.y * w.y; acc = acc + u.z * w.z; acc = acc + u.w * w.w;
            } else { acc = acc + u.x; acc = acc + u.y; acc = acc + u.z; acc = acc + u.w; }
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (e + j < HW) acc = acc + (PROD ? a[e + j] * b[e + j] : a[e + j]);
        }
    }
    acc = se_tree64(acc);
    if (lane == 0) {
        if (PROD) p.t[(int64_t)n * p.C + c] = acc;
        else p.m[(int64_t)n * p.C + c] = acc * p.inv_hw;
    }
}

// ---- excite: one block per frame; dynamic LDS: rd floats ----
template <bool BWD>
__global__ void __launch_bounds__(256) se_excite_kernel(const I2VSeParams p) {
    extern __shared__ __attribute__((aligned(16))) float se_lds[];
    const int n = blockIdx.x, C = p.C, rd = p.rd, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nw = blockDim.x >> 6;
    const float* s = p.s + (int64_t)n * C;
    const float* h = p.h + (int64_t)n * rd;
    // sums over c: forward h[j] from w1 and m, backward dh[j] from w2t and dz2
    const float* v = BWD ? p.t + (int64_t)n * C : p.m + (int64_t)n * C;
    const float* W = BWD ? p.w2t : p.w1;
    for (int j = wave; j < rd; j += nw) {
        const float* row = W + (int64_t)j * C;
        float acc = 0.f;
        for (int c = lane; c < C; c += 64) {
            float f = v[c];
            if (BWD) { const float sc = s[c]; f = (f * sc) * (1.f - sc); }
            acc = __builtin_fmaf(row[c], f, acc);
        }
        acc = se_tree64(acc);
        if (lane == 0) {
            if (BWD) se_lds[j] = h[j] > 0.f ? acc : 0.f;
            else { const float hv = fmaxf(acc + p.b1[j], 0.f); se_lds[j] = hv; p.h[(int64_t)n * rd + j] = hv; }
        }
    }
    __syncthreads();
    // sums over j: forward s[c] from w2t and h, backward dmh[c] from w1 and dh
    const float* V = BWD ? p.w1 : p.w2t;
    for (int c = tid; c < C; c += blockDim.x) {
        float acc = 0.f;
        for (int j = 0; j < rd; ++j) acc = __builtin_fmaf(V[(int64_t)j * C + c], se_lds[j], acc);
        if (BWD) p.dmh[(int64_t)n * C + c] = acc * p.inv_hw;
        else p.s[(int64_t)n * C + c] = 1.f / (1.f + expf(-(acc + p.b2[c])));
    }
}

// ---- scale: dst = act(a * s[n][c] + (r | dmh[n][c])), a = x forward, g backward ----
template <bool V4>
__global__ void __launch_bounds__(256) se_scale_kernel(const I2VSeParams p) {
    constexpr int V = V4 ? 4 : 1;
    const int c = blockIdx.y, HW = p.HW, tid = threadIdx.x;
    const unsigned total = (unsigned)p.N * (unsigned)HW;
    const unsigned q = (blockIdx.x * 256u + (unsigned)tid) * V;        // (k_se_scale: the grid covers less than 2^31 positions)
    const bool valid = q < total;                                       // (V4: HW % 4 == 0, so the four positions are valid together and in one frame)
    const unsigned qq = valid ? q : 0u;
    const unsigned n = fastdiv(qq, p.dv_hw_m, p.dv_hw_s);
    const int pix = (int)(qq - n * (unsigned)HW);
    const int64_t nc = (int64_t)n * p.C + c, off = (int64_t)c * HW + pix;
    const float* a = (p.backward ? p.g + (int64_t)n * p.g_nstride : p.x + (int64_t)n * p.x_nstride) + off;
    float* d = p.dst + (int64_t)n * p.dst_nstride + off;
    const float sc = p.s[nc];
    const float addc = p.backward ? p.dmh[nc] : 0.f;
    const bool has_r = !p.backward && p.r;
    const float* r = has_r ? p.r + (int64_t)n * p.r_nstride + off : nullptr;
    unsigned bits = 0;
    if (V4) {
        se_f4 u = se_f4{0.f, 0.f, 0.f, 0.f};
        if (valid) {
            u = *(const se_f4*)a;
            u.x = u.x * sc; u.y = u.y * sc; u.z = u.z * sc; u.w = u.w * sc;
            if (has_r) { const se_f4 w = *(const se_f4*)r; u.x = u.x + w.x; u.y = u.y + w.y; u.z = u.z + w.z; u.w = u.w + w.w; }
            else if (p.backward) { u.x = u.x + addc; u.y = u.y + addc; u.z = u.z + addc; u.w = u.w + addc; }
            if (p.relu) { u.x = fmaxf(u.x, 0.f); u.y = fmaxf(u.y, 0.f); u.z = fmaxf(u.z, 0.f); u.w = fmaxf(u.w, 0.f); }
            *(se_f4*)d = u;
            bits = (u.x > 0.f ? 1u : 0u) | (u.y > 0.f ? 2u : 0u) | (u.z > 0.f ? 4u : 0u) | (u.w > 0.f ? 8u : 0u);
        }
        if (p.gate_out) {       // lanes 8 w .. 8 w + 7 of the wave hold the 32 bits q .. q + 31 of a word: q is a multiple of 32 at lane 8 w
            const int lane = tid & 63;
            unsigned word = bits << (4 * (lane & 7));
            word |= __shfl_xor(word, 1, 64); word |= __shfl_xor(word, 2, 64); word |= __shfl_xor(word, 4, 64);
            if (valid && (lane & 7) == 0) p.gate_out[(int64_t)c * p.gate_out_stride + (q >> 5)] = word;
        }
    } else {
        float u = 0.f;
        if (valid) {
            u = a[0] * sc;
            if (has_r) u = u + r[0]; else if (p.backward) u = u + addc;
            if (p.relu) u = fmaxf(u, 0.f);
            d[0] = u;
        }
        if (p.gate_out) {       // the wave's lanes are bits 64 w .. 64 w + 63 of row c
            const unsigned long long bal = __ballot(valid && u > 0.f);
            const int lane = tid & 63;
            if (valid && (lane & 31) == 0) p.gate_out[(int64_t)c * p.gate_out_stride + (q >> 5)] = (unsigned)(bal >> lane);
        }
    }
}

static bool se_al16(const void* q, int64_t nstride) { return ((uintptr_t)q & 15) == 0 && nstride % 4 == 0; }

int k_se_plan(I2VSeParams* p) {
    if (p->C < 1 || p->rd < 1 || p->HW < 1) return 1;
    fastdiv_magic((unsigned)p->HW, &p->dv_hw_m, &p->dv_hw_s);
    p->inv_hw = 1.f / (float)p->HW;
    return 0;
}

static int se_check(const I2VSeParams& p, const char* who) {
    uint32_t m, s; fastdiv_magic((unsigned)(p.HW > 0 ? p.HW : 1), &m, &s);
    if (p.C < 1 || p.rd < 1 || p.HW < 1 || p.N < 0 || m != p.dv_hw_m || s != p.dv_hw_s || !p.x || !p.s) {
        char b[96]; snprintf(b, sizeof b, "%s: launch not planned (k_se_plan)", who); return hip_fail(hipErrorInvalidValue, b);
    }
    if ((int64_t)p.N * p.HW >= (1ll << 31)) { char b[96]; snprintf(b, sizeof b, "%s: more than 2^31 positions", who); return hip_fail(hipErrorInvalidValue, b); }
    return 0;
}

int k_se_squeeze(const I2VSeParams& p, i2v_stream_t st) {
    if (se_check(p, "k_se_squeeze")) return 1;
    if (p.backward ? (!p.g || !p.t) : !p.m) return hip_fail(hipErrorInvalidValue, "k_se_squeeze: launch not planned (k_se_plan)");
    if (p.N == 0) return 0;
    const dim3 grid((unsigned)((p.C + 3) / 4), (unsigned)p.N);
    if (grid.y > 65535u) return hip_fail(hipErrorInvalidValue, "k_se_squeeze: more than 65535 frames");
    const bool v4 = p.HW % 4 == 0 && se_al16(p.x, p.x_nstride) && (!p.backward || se_al16(p.g, p.g_nstride));
    __atomic_fetch_add(&g_stat_se, 1, __ATOMIC_RELAXED);
    hipStream_t s = (hipStream_t)st;
    if (p.backward) { if (v4) hipLaunchKernelGGL((se_squeeze_kernel<true, true>), grid, dim3(256), 0, s, p); else hipLaunchKernelGGL((se_squeeze_kernel<false, true>), grid, dim3(256), 0, s, p); }
    else { if (v4) hipLaunchKernelGGL((se_squeeze_kernel<true, false>), grid, dim3(256), 0, s, p); else hipLaunchKernelGGL((se_squeeze_kernel<false, false>), grid, dim3(256), 0, s, p); }
    LAUNCH_CHECK("se_squeeze_kernel");
    return 0;
}

int k_se_excite(const I2VSeParams& p, i2v_stream_t st) {
    if (se_check(p, "k_se_excite")) return 1;
    if (!p.w1 || !p.w2t || !p.h || (p.backward ? (!p.t || !p.dmh) : (!p.m || !p.b1 || !p.b2)))
        return hip_fail(hipErrorInvalidValue, "k_se_excite: launch not planned (k_se_plan)");
    if (p.rd > 8192) return hip_fail(hipErrorInvalidValue, "k_se_excite: more than 8192 squeezed channels");
    if (p.N == 0) return 0;
    const dim3 grid((unsigned)p.N);
    const size_t lds = (size_t)p.rd * sizeof(float);
    __atomic_fetch_add(&g_stat_se, 1, __ATOMIC_RELAXED);
    hipStream_t s = (hipStream_t)st;
    if (p.backward) hipLaunchKernelGGL((se_excite_kernel<true>), grid, dim3(256), lds, s, p);
    else hipLaunchKernelGGL((se_excite_kernel<false>), grid, dim3(256), lds, s, p);
    LAUNCH_CHECK("se_excite_kernel");
    return 0;
}

int k_se_scale(const I2VSeParams& p, i2v_stream_t st) {
    if (se_check(p, "k_se_scale")) return 1;
    if (!p.dst || (p.backward && (!p.g || !p.dmh))) return hip_fail(hipErrorInvalidValue, "k_se_scale: launch not planned (k_se_plan)");
    if (p.gate_out && (!p.relu || p.backward)) return hip_fail(hipErrorInvalidValue, "k_se_scale: gate rows are written by forward launches with ReLU only");
    if (p.backward && p.relu) return hip_fail(hipErrorInvalidValue, "k_se_scale: a backward launch has no ReLU");
    if (p.N == 0) return 0;
    const float* a = p.backward ? p.g : p.x;
    const bool v4 = p.HW % 4 == 0 && se_al16(a, p.backward ? p.g_nstride : p.x_nstride) && se_al16(p.dst, p.dst_nstride) &&
                    (p.backward || !p.r || se_al16(p.r, p.r_nstride));
    const int64_t total = (int64_t)p.N * p.HW, per = 256 * (v4 ? 4 : 1);
    const dim3 grid((unsigned)((total + per - 1) / per), (unsigned)p.C);
    if (grid.y > 65535u) return hip_fail(hipErrorInvalidValue, "k_se_scale: more than 65535 channels");
    __atomic_fetch_add(&g_stat_se, 1, __ATOMIC_RELAXED);
    hipStream_t s = (hipStream_t)st;
    if (v4) hipLaunchKernelGGL((se_scale_kernel<true>), grid, dim3(256), 0, s, p);
    else hipLaunchKernelGGL((se_scale_kernel<false>), grid, dim3(256), 0, s, p);
    LAUNCH_CHECK("se_scale_kernel");
    return 0;
}
