// Depthwise k x k convolution (k = 3 or 5, pad k / 2, stride 1 or 2) for gfx950 -- the mobile nets' middle layer: MNASNet's
// `nn.Conv2d(C, C, k, stride, k // 2, groups=C)` -- forward and input gradient, ONE launch per node and pass.
//
// A depthwise layer moves 8 bytes per output element for 18 or 50 flops: it is bound by memory, never by arithmetic, so the kernel is
// laid out for bytes and for the gate words, on the arrangement of i2v_gconv.hip:
//   * a block is (64 x waves consecutive positions of the N x Hg x Wg grid) x (one channel) x (one stride-parity class); positions run
//     LINEARLY over frames, so a wave's 64 lanes are 64 consecutive bits of a gate row, aligned to 64: the ballot of (v > 0) IS the two
//     gate words, owned by this wave alone -- no atomics, no read-modify-write, the same bits every run whatever the block size;
//   * the block stages the source rows its positions touch -- `pad` zero columns either side, the `pad` zero rows above and below every
//     frame ("padded rows": frame n owns rows n (Hs + 2 pad) .. + Hs + 2 pad - 1) -- in LDS once, so every source element is fetched once
//     per block (16-byte loads where the plane's rows are 16-byte aligned: Ws a multiple of 4); the k x k taps of a lane are then plain
//     LDS reads at lbase + a pitch + b with no bounds checks, so planes smaller than the filter need nothing special;
//   * the k x k weights of the channel are read through the constant address space from a readfirstlane'd base: scalar loads, SGPR
//     operands of the FMAs (the trick of i2v_gconv.hip).
// Arithmetic: each output is ONE fp32 FMA chain acc = fma(w[a][b], x[a][b], acc) from acc = 0 over the slots (a, b) in row-major order,
// a = 0 .. k - 1 outer, b = 0 .. k - 1 inner, skipping the slots the class does not own; then + shift, ReLU, gate.  (-ffp-contract=off:
// the fma is written, nothing else is contracted.)  The order does not depend on the launch geometry, the batch or the run.
// The input gradient is the same kernel: source = the output's gradient read at stride 1, the filter mirrored, one class per stride
// parity (row parity, column parity) with the slots that parity owns (2 or 1 per axis for k = 3 at stride 2, 3 or 2 for k = 5; a
// uniform branch per slot), written at stride `os`.
#include "i2v_be.h"

long long g_stat_dwconv = 0;

typedef float dw_f4 __attribute__((ext_vector_type(4)));

template <int K, bool ALL, bool V4>
__global__ void __launch_bounds__(1024) dwconv_kernel(const I2VDwConvParams p) {
    extern __shared__ __attribute__((aligned(16))) float dw_lds[];
    constexpr int PAD = K / 2;
    const int cls = blockIdx.z, ch = blockIdx.y;
    const I2VDwConvClass c = p.cls[cls];
    const int HW = c.Hg * c.Wg;
    const unsigned total = (unsigned)p.N * (unsigned)HW;
    const int P = blockDim.x, tid = threadIdx.x;
    const unsigned q0 = blockIdx.x * (unsigned)P;
    if (q0 >= total) return;                               // (whole block: classes differ in size, the grid is the largest one's)
    const unsigned qlast = (q0 + P < total ? q0 + P : total) - 1;
    const int RP = p.Hs + 2 * PAD, pitch = p.pitch, S = p.S;
    // padded source rows this block touches
    const unsigned n0 = fastdiv(q0, c.dv_hw_m, c.dv_hw_s), n1 = fastdiv(qlast, c.dv_hw_m, c.dv_hw_s);
    const unsigned i0 = fastdiv(q0 - n0 * HW, c.dv_w_m, c.dv_w_s), i1 = fastdiv(qlast - n1 * HW, c.dv_w_m, c.dv_w_s);
    const int v_lo = (int)n0 * RP + (int)i0 * S;
    int nv = (int)n1 * RP + (int)i1 * S + K - 1 - v_lo + 1;
    if (nv > p.rows) nv = p.rows;                          // (k_dwconv_plan sized `rows` for the worst block: never taken)
    {   // stage: every element of the [nv][pitch] image is written (zeros outside the plane).  Plain: pitch = Ws + 2 PAD, source column 0
        // is image column PAD, one 4-byte load per element.  V4 (every source row 16-byte aligned): pitch = Ws + 8, source column 0 is
        // image column 4, a unit is four image columns = four source columns: one 16-byte load, one 16-byte LDS write
        const int64_t plane = (int64_t)p.Hs * p.Ws;
        const float* sch = p.src + (int64_t)ch * plane;
        if (V4) {
            const int upr = pitch >> 2;                    // units per row; unit u is image columns 4 u .. 4 u + 3: source columns 4 (u - 1) .. + 3
            for (int e = tid; e < nv * upr; e += P) {
                const unsigned v = fastdiv((unsigned)e, p.dv_u_m, p.dv_u_s);
                const int u = e - (int)v * upr;
                const unsigned va = (unsigned)(v_lo + (int)v);
                const unsigned n = fastdiv(va, p.dv_r_m, p.dv_r_s);
                const int y = (int)(va - n * RP) - PAD, x = 4 * (u - 1);
                const bool ok = y >= 0 && y < p.Hs && (int)n < p.N && x >= 0 && x < p.Ws;
                dw_f4 t = dw_f4{0.f, 0.f, 0.f, 0.f};
                if (ok) t = *(const dw_f4*)(sch + (int64_t)n * p.src_nstride + (int64_t)y * p.Ws + x);
                *(dw_f4*)(dw_lds + (int)v * pitch + 4 * u) = t;
            }
        } else {
            for (int e = tid; e < nv * pitch; e += P) {
                const unsigned v = fastdiv((unsigned)e, p.dv_u_m, p.dv_u_s);
                const int xi = e - (int)v * pitch;
                const unsigned va = (unsigned)(v_lo + (int)v);
                const unsigned n = fastdiv(va, p.dv_r_m, p.dv_r_s);
                const int y = (int)(va - n * RP) - PAD, x = xi - PAD;
                const bool ok = y >= 0 && y < p.Hs && (int)n < p.N && x >= 0 && x < p.Ws;
                dw_lds[e] = ok ? sch[(int64_t)n * p.src_nstride + (int64_t)y * p.Ws + x] : 0.f;
            }
        }
    }
    __syncthreads();
    const unsigned q = q0 + tid;
    const bool valid = q < total;
    const unsigned qq = valid ? q : q0;
    const unsigned n = fastdiv(qq, c.dv_hw_m, c.dv_hw_s);
    const unsigned rem = qq - n * HW;
    const unsigned i = fastdiv(rem, c.dv_w_m, c.dv_w_s), j = rem - i * c.Wg;
    // image column of source column x is x + xoff (V4: 4, so that source column 0 sits on a 16-byte boundary; else PAD)
    const int lbase = ((int)n * RP + (int)i * S - v_lo) * pitch + (int)j * S + (V4 ? 4 - PAD : 0);
    const int HoWo = p.Ho * p.Wo;
    const int opix = ((int)i * p.os + c.oh0) * p.Wo + (int)j * p.os + c.ow0;
    const unsigned gidx = n * (unsigned)HoWo + (unsigned)opix;
    // the channel's weights: the address is made of readfirstlane'd halves, so the compiler knows it is wave-uniform and the reads
    // through the constant address space are scalar loads, their values SGPR operands of the FMAs
    const __attribute__((address_space(4))) float* wr;
    {
        const uint64_t a = (uint64_t)(p.w + ((size_t)cls * p.C + ch) * (size_t)(K * K));
        const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)a), hi = __builtin_amdgcn_readfirstlane((uint32_t)(a >> 32));
        wr = (const __attribute__((address_space(4))) float*)(((uint64_t)hi << 32) | lo);
    }
    const int tapmask = c.tapmask;
    const float* xs = dw_lds + lbase;
    float acc = 0.f;
#pragma unroll
    for (int t = 0; t < K * K; ++t)
        if (ALL || ((tapmask >> t) & 1)) acc = __builtin_fmaf(wr[t], xs[(t / K) * pitch + (t % K)], acc);
    float v = acc;
    if (p.shift) v += p.shift[ch];
    if (p.relu) v = fmaxf(v, 0.f);
    if (p.gate) { if (!((p.gate[(int64_t)ch * p.gate_stride + (gidx >> 5)] >> (gidx & 31)) & 1u)) v = 0.f; }
    else if (p.mask) { if (!(p.mask[(int64_t)n * p.mask_nstride + (int64_t)ch * HoWo + opix] > 0.f)) v = 0.f; }
    if (valid) p.dst[(int64_t)n * p.dst_nstride + (int64_t)ch * HoWo + opix] = v;
    if (p.gate_out) {       // forward (os == 1, one class): gidx == q, the wave's lanes are bits 64 w .. 64 w + 63 of row ch
        const unsigned long long bal = __ballot(valid && v > 0.f);
        const int lane = tid & 63;
        if (valid && (lane & 31) == 0)
            p.gate_out[(int64_t)ch * p.gate_out_stride + (q >> 5)] = (unsigned)(bal >> lane);
    }
}

template <int K>
static const void* dwconv_fn_k(bool all, bool v4) {
    if (all) return v4 ? reinterpret_cast<const void*>(dwconv_kernel<K, true, true>) : reinterpret_cast<const void*>(dwconv_kernel<K, true, false>);
    return v4 ? reinterpret_cast<const void*>(dwconv_kernel<K, false, true>) : reinterpret_cast<const void*>(dwconv_kernel<K, false, false>);
}
static bool dwconv_all(const I2VDwConvParams& p) {
    for (int k = 0; k < p.ncls; ++k) if (p.cls[k].tapmask != (1 << (p.k * p.k)) - 1) return false;
    return true;
}
// 16-byte staging: every source row starts on a 16-byte boundary
static bool dwconv_v4(const I2VDwConvParams& p) {
    return p.Ws % 4 == 0 && p.src_nstride % 4 == 0 && ((uintptr_t)p.src & 15) == 0;
}
static int dwconv_pitch(const I2VDwConvParams& p, bool v4) {
    return v4 ? p.Ws + 8 : p.Ws + 2 * (p.k / 2);           // V4: four zero columns either side (of which `pad` are read)
}

// rows of padded source a block of `P` positions touches at most, over every block start of every class
static int dwconv_rows(const I2VDwConvParams& p, int P) {
    const int RP = p.Hs + 2 * (p.k / 2);
    int worst = p.k;
    for (int k = 0; k < p.ncls; ++k) {
        const I2VDwConvClass& c = p.cls[k];
        const int64_t HW = (int64_t)c.Hg * c.Wg;
        if (HW <= 0) continue;
        for (int64_t b = 0; b < HW; ++b) {              // the pattern of block starts repeats after at most HW blocks
            const int64_t q0 = b * P, q1 = q0 + P - 1;
            const int64_t n0 = q0 / HW, n1 = q1 / HW, i0 = (q0 % HW) / c.Wg, i1 = (q1 % HW) / c.Wg;
            const int64_t nv = n1 * RP + i1 * p.S + p.k - 1 - (n0 * RP + i0 * p.S) + 1;
            if (nv > worst) worst = (int)nv;
        }
    }
    return worst;
}

int k_dwconv_plan(I2VDwConvParams* p) {
    if (p->k != 3 && p->k != 5) return 1;
    if (p->ncls < 1 || p->ncls > 4 || p->S < 1 || p->S > 2 || p->os < 1 || p->os > 2 || p->C < 1 || p->Hs < 1 || p->Ws < 1) return 1;
    const int pad = p->k / 2;
    int wmax = 1;
    for (int k = 0; k < p->ncls; ++k) {
        I2VDwConvClass& c = p->cls[k];
        if (c.Hg <= 0 || c.Wg <= 0) { c.Hg = c.Wg = 0; continue; }
        // every tap of every position lies inside the padded source plane; every position lands inside the destination plane
        if ((c.Hg - 1) * p->S + p->k - 1 > p->Hs + 2 * pad - 1 || (c.Wg - 1) * p->S + p->k - 1 > p->Ws + 2 * pad - 1) return 1;
        if ((c.Hg - 1) * p->os + c.oh0 >= p->Ho || (c.Wg - 1) * p->os + c.ow0 >= p->Wo) return 1;
        fastdiv_magic((unsigned)c.Wg, &c.dv_w_m, &c.dv_w_s);
        fastdiv_magic((unsigned)(c.Hg * c.Wg), &c.dv_hw_m, &c.dv_hw_s);
        wmax = c.Wg > wmax ? c.Wg : wmax;
    }
    fastdiv_magic((unsigned)(p->Hs + 2 * pad), &p->dv_r_m, &p->dv_r_s);
    const bool v4 = dwconv_v4(*p);
    p->v4 = v4 ? 1 : 0;
    p->pitch = dwconv_pitch(*p, v4);
    fastdiv_magic((unsigned)(v4 ? p->pitch / 4 : p->pitch), &p->dv_u_m, &p->dv_u_s);
    // the block: about eight output rows of the plane, so that the k - 1 halo rows a block stages on top of its own stay a small part of
    // what it reads; 64 .. 1024 positions.  (Results do not depend on it: every output is one lane's chain.)
    int w = 1;
    while (w < 16 && 64 * w < 8 * wmax) w <<= 1;
    for (;; w >>= 1) {
        const int rows = dwconv_rows(*p, 64 * w);
        const size_t lds = (size_t)rows * p->pitch * sizeof(float);
        if (lds <= 32 * 1024 || w == 1) {
            if (lds > 64 * 1024) return 1;
            p->waves = w; p->rows = rows; p->lds_bytes = (int)lds;
            return 0;
        }
    }
}

template <int K>
static int dwconv_launch(const I2VDwConvParams& p, dim3 grid, hipStream_t s) {
    const bool all = dwconv_all(p), v4 = p.v4 != 0;
    const dim3 blk(64 * p.waves);
    const size_t lds = (size_t)p.lds_bytes;
    if (all) { if (v4) hipLaunchKernelGGL((dwconv_kernel<K, true, true>), grid, blk, lds, s, p); else hipLaunchKernelGGL((dwconv_kernel<K, true, false>), grid, blk, lds, s, p); }
    else { if (v4) hipLaunchKernelGGL((dwconv_kernel<K, false, true>), grid, blk, lds, s, p); else hipLaunchKernelGGL((dwconv_kernel<K, false, false>), grid, blk, lds, s, p); }
    LAUNCH_CHECK("dwconv_kernel");
    return 0;
}

int k_dwconv(const I2VDwConvParams& p, i2v_stream_t st) {
    hipStream_t s = (hipStream_t)st;
    if ((p.k != 3 && p.k != 5) || p.waves < 1 || p.waves > 16 || p.rows < p.k || p.lds_bytes <= 0 || p.pitch < p.Ws + 2 * (p.k / 2) ||
        (size_t)p.rows * p.pitch * sizeof(float) != (size_t)p.lds_bytes)
        return hip_fail(hipErrorInvalidValue, "k_dwconv: launch not planned (k_dwconv_plan)");
    if ((p.v4 != 0) != dwconv_v4(p) || (p.v4 && p.pitch != p.Ws + 8))
        return hip_fail(hipErrorInvalidValue, "k_dwconv: launch not planned for this source (k_dwconv_plan)");
    int64_t most = 0;
    for (int k = 0; k < p.ncls; ++k) {
        const int64_t t = (int64_t)p.N * p.cls[k].Hg * p.cls[k].Wg;
        if (t >= (1ll << 31) || (int64_t)(p.N + 1) * (p.Hs + 2 * (p.k / 2)) >= (1ll << 31) || (int64_t)p.N * p.Ho * p.Wo >= (1ll << 31))
            return hip_fail(hipErrorInvalidValue, "k_dwconv: more than 2^31 positions");
        most = t > most ? t : most;
    }
    if (most == 0) return 0;
    if (p.gate_out && (p.ncls != 1 || p.os != 1 || p.cls[0].Hg != p.Ho || p.cls[0].Wg != p.Wo || p.cls[0].oh0 || p.cls[0].ow0))
        return hip_fail(hipErrorInvalidValue, "k_dwconv: gate rows are written by dense forward launches only");
    const int P = 64 * p.waves;
    const dim3 grid((unsigned)((most + P - 1) / P), (unsigned)p.C, (unsigned)p.ncls);
    if (grid.y > 65535u) return hip_fail(hipErrorInvalidValue, "k_dwconv: more than 65535 channels");
    if (grid.z > 65535u) return hip_fail(hipErrorInvalidValue, "k_dwconv: more than 65535 classes");
    __atomic_fetch_add(&g_stat_dwconv, 1, __ATOMIC_RELAXED);
    return p.k == 3 ? dwconv_launch<3>(p, grid, s) : dwconv_launch<5>(p, grid, s);
}
