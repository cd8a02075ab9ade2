// Grouped 3x3 / pad-1 convolution for gfx950 (ResNeXt's conv2), forward and input gradient, ONE launch per node and pass.
//
// With 4..64 channels per group a 32 x 32 fp32 MFMA fragment would be mostly empty (and a block-diagonal dense weight does `groups`
// times the products), so the arithmetic is packed-fp32 FMA on the vector unit, the idiom of i2v_fastblock.hip (DESIGN.md section 10:
// v_pk_fma_f32 has the fp32-input MFMA's peak on this part):
//   * a block is (64 x waves consecutive positions of the N x Hg x Wg grid) x (one group) x (one stride-parity class); positions run
//     LINEARLY over frames, so a wave's 64 lanes are 64 consecutive bits of a gate row, aligned to 64: the ballot of (v > 0) IS the two
//     gate words, owned by this wave alone -- no atomics, no read-modify-write, the same bits every run;
//   * the block stages the source rows its positions touch -- all `gw` channels of the group, one zero column either side, the zero
//     rows above and below every frame ("padded rows": frame n owns rows n (Hs + 2) .. + Hs + 1) -- in LDS once; the nine taps of a
//     lane are then plain LDS reads at lbase + a pitch + b, no bounds checks in the inner loop;
//   * one lane per output position; the weights of a (channel, tap) are `COB` consecutive floats read through the constant address
//     space from a readfirstlane'd base -- scalar loads, SGPR-pair operands of COB / 2 v_pk_fma_f32 against the lane's broadcast
//     source value (checked in the disassembly: no vector load of a weight, no spill, 27-61 VGPRs).
// The input gradient is the same kernel: source = the output's gradient, weights transposed and mirrored, one class per stride parity
// with the taps that parity owns (a uniform branch per tap), written at stride `os`.
#include "i2v_be.h"

long long g_stat_gconv = 0;

typedef float gc_f2 __attribute__((ext_vector_type(2)));

template <int GW, int COB, bool ALL>
__global__ void __launch_bounds__(256) gconv_kernel(const I2VGConvParams p) {
    extern __shared__ __attribute__((aligned(16))) float gc_lds[];
    const int cls = blockIdx.z, g = blockIdx.y;
    const I2VGConvClass c = p.cls[cls];
    const int HW = c.Hg * c.Wg;
    const unsigned total = (unsigned)p.N * (unsigned)HW;
    const int P = blockDim.x, tid = threadIdx.x;
    const unsigned q0 = blockIdx.x * (unsigned)P;
    if (q0 >= total) return;                               // (whole block: classes differ in size, the grid is the largest one's)
    const unsigned qlast = (q0 + P < total ? q0 + P : total) - 1;
    const int RP = p.Hs + 2, pitch = p.Ws + 2, S = p.S;
    const int chs = p.rows * pitch;                        // LDS floats per channel
    // padded source rows this block touches
    const unsigned n0 = fastdiv(q0, c.dv_hw_m, c.dv_hw_s), n1 = fastdiv(qlast, c.dv_hw_m, c.dv_hw_s);
    const unsigned i0 = fastdiv(q0 - n0 * HW, c.dv_w_m, c.dv_w_s), i1 = fastdiv(qlast - n1 * HW, c.dv_w_m, c.dv_w_s);
    const int v_lo = (int)n0 * RP + (int)i0 * S;
    int nv = (int)n1 * RP + (int)i1 * S + 2 - v_lo + 1;
    if (nv > p.rows) nv = p.rows;                          // (k_gconv_plan sized `rows` for the worst block: never taken)
    {   // stage: lanes along a row, rows over the lane groups; every element of the [gw][nv][pitch] image is written (zeros outside)
        int lpr = 64; while (lpr > 8 && (lpr >> 1) >= pitch) lpr >>= 1;
        const int rpp = P / lpr, x0 = tid % lpr;
        const int64_t plane = (int64_t)p.Hs * p.Ws;
        for (int v = tid / lpr; v < nv; v += rpp) {
            const unsigned va = (unsigned)(v_lo + v);
            const unsigned n = fastdiv(va, p.dv_r_m, p.dv_r_s);
            const int y = (int)(va - n * RP) - 1;
            const bool rok = y >= 0 && y < p.Hs && (int)n < p.N;
            const float* srow = p.src + (int64_t)n * p.src_nstride + (int64_t)g * GW * plane + (int64_t)y * p.Ws - 1;
            float* drow = gc_lds + v * pitch;
            for (int x = x0; x < pitch; x += lpr) {
                const bool ok = rok && x >= 1 && x <= p.Ws;
#pragma unroll 4
                for (int ch = 0; ch < GW; ++ch) drow[ch * chs + x] = ok ? srow[ch * plane + x] : 0.f;
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
    const int lbase = ((int)n * RP + (int)i * S - v_lo) * pitch + (int)j * S;
    const int HoWo = p.Ho * p.Wo;
    const int opix = ((int)i * p.os + c.oh0) * p.Wo + (int)j * p.os + c.ow0;
    const unsigned gidx = n * (unsigned)HoWo + (unsigned)opix;
    // the group's weights: the address is made of readfirstlane'd halves, so the compiler KNOWS it is wave-uniform and the reads
    // through the constant address space below are scalar loads (s_load_dwordx4 / x8 / x16), their values SGPR operands of the FMAs
    // (left to its own divergence analysis it issued one per-lane global_load_dwordx4 per two packed FMAs)
    const float* wcls;
    {
        const uint64_t a = (uint64_t)(p.w + ((size_t)cls * p.groups + g) * (size_t)(GW * 9 * GW));
        const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)a), hi = __builtin_amdgcn_readfirstlane((uint32_t)(a >> 32));
        wcls = (const float*)(((uint64_t)hi << 32) | lo);
    }
    const int tapmask = c.tapmask;
#pragma unroll 1
    for (int cb = 0; cb < GW; cb += COB) {
        gc_f2 acc[COB / 2];
#pragma unroll
        for (int k = 0; k < COB / 2; ++k) acc[k] = gc_f2{0.f, 0.f};
#pragma unroll 2
        for (int ci = 0; ci < GW; ++ci) {
            const float* xs = gc_lds + ci * chs + lbase;
            const __attribute__((address_space(4))) gc_f2* wr =
                (const __attribute__((address_space(4))) gc_f2*)(wcls + (size_t)ci * 9 * GW + cb);
#pragma unroll
            for (int t = 0; t < 9; ++t) {
                if (ALL || ((tapmask >> t) & 1)) {
                    const float x = xs[(t / 3) * pitch + (t % 3)];
                    const gc_f2 xx = gc_f2{x, x};
#pragma unroll
                    for (int k = 0; k < COB / 2; ++k) acc[k] = __builtin_elementwise_fma(wr[t * (GW / 2) + k], xx, acc[k]);
                }
            }
        }
#pragma unroll
        for (int k = 0; k < COB; ++k) {
            const int ch = g * GW + cb + k;
            float v = (k & 1) ? acc[k / 2].y : acc[k / 2].x;
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
    }
}

template <int GW, int COB>
static const void* gconv_fn_of(bool all) {
    return all ? reinterpret_cast<const void*>(gconv_kernel<GW, COB, true>) : reinterpret_cast<const void*>(gconv_kernel<GW, COB, false>);
}
static const void* gconv_fn(int gw, bool all) {
    switch (gw) {
        case 4: return gconv_fn_of<4, 4>(all);
        case 8: return gconv_fn_of<8, 8>(all);
        case 16: return gconv_fn_of<16, 16>(all);
        case 32: return gconv_fn_of<32, 16>(all);
        default: return gconv_fn_of<64, 16>(all);
    }
}

// rows of padded source a block of `P` positions touches at most, over every block start of every class
static int gconv_rows(const I2VGConvParams& p, int P) {
    const int RP = p.Hs + 2;
    int worst = 3;
    for (int k = 0; k < p.ncls; ++k) {
        const I2VGConvClass& c = p.cls[k];
        const int64_t HW = (int64_t)c.Hg * c.Wg;
        if (HW <= 0) continue;
        const int64_t blocks = HW;                      // the pattern of block starts repeats after at most HW blocks
        for (int64_t b = 0; b < blocks; ++b) {
            const int64_t q0 = b * P, q1 = q0 + P - 1;
            const int64_t n0 = q0 / HW, n1 = q1 / HW, i0 = (q0 % HW) / c.Wg, i1 = (q1 % HW) / c.Wg;
            const int64_t nv = n1 * RP + i1 * p.S + 2 - (n0 * RP + i0 * p.S) + 1;
            if (nv > worst) worst = (int)nv;
        }
    }
    return worst;
}

int k_gconv_plan(I2VGConvParams* p) {
    if (p->gw != 4 && p->gw != 8 && p->gw != 16 && p->gw != 32 && p->gw != 64) return 1;
    if (p->ncls < 1 || p->ncls > 4 || p->S < 1 || p->os < 1) return 1;
    for (int k = 0; k < p->ncls; ++k) {
        I2VGConvClass& c = p->cls[k];
        if (c.Hg <= 0 || c.Wg <= 0) { c.Hg = c.Wg = 0; continue; }
        // every tap of every position lies inside the padded source plane; every position lands inside the destination plane
        if ((c.Hg - 1) * p->S + 2 > p->Hs + 1 || (c.Wg - 1) * p->S + 2 > p->Ws + 1) return 1;
        if ((c.Hg - 1) * p->os + c.oh0 >= p->Ho || (c.Wg - 1) * p->os + c.ow0 >= p->Wo) return 1;
        fastdiv_magic((unsigned)c.Wg, &c.dv_w_m, &c.dv_w_s);
        fastdiv_magic((unsigned)(c.Hg * c.Wg), &c.dv_hw_m, &c.dv_hw_s);
    }
    fastdiv_magic((unsigned)(p->Hs + 2), &p->dv_r_m, &p->dv_r_s);
    const int pitch = p->Ws + 2;
    int best_w = 0, best_rows = 0; size_t best_lds = 0;
    for (int w = 4; w >= 1; w >>= 1) {
        const int rows = gconv_rows(*p, 64 * w);
        const size_t lds = (size_t)p->gw * rows * pitch * sizeof(float);
        if (!best_w || lds < best_lds) { best_w = w; best_rows = rows; best_lds = lds; }
        if (lds <= 40 * 1024) { best_w = w; best_rows = rows; best_lds = lds; break; }     // the widest block that keeps four blocks per CU
    }
    if (best_lds > 160 * 1024) return 1;
    p->waves = best_w; p->rows = best_rows; p->lds_bytes = (int)best_lds;
    if (best_lds > 64 * 1024)        // above the default dynamic-LDS limit: raised once per instantiation, here, never on the launch path
        for (int all = 0; all < 2; ++all)
            if (hipFuncSetAttribute(gconv_fn(p->gw, all != 0), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) != hipSuccess) return 1;
    return 0;
}

template <int GW, int COB>
static int gconv_launch(const I2VGConvParams& p, dim3 grid, hipStream_t s) {
    bool all = true;
    for (int k = 0; k < p.ncls; ++k) if (p.cls[k].tapmask != 0x1FF) all = false;
    auto fn = all ? gconv_kernel<GW, COB, true> : gconv_kernel<GW, COB, false>;
    hipLaunchKernelGGL(fn, grid, dim3(64 * p.waves), (size_t)p.lds_bytes, s, p);
    LAUNCH_CHECK("gconv_kernel");
    return 0;
}

int k_gconv(const I2VGConvParams& p, i2v_stream_t st) {
    hipStream_t s = (hipStream_t)st;
    if (p.waves < 1 || p.rows < 3 || p.lds_bytes <= 0) return hip_fail(hipErrorInvalidValue, "k_gconv: launch not planned (k_gconv_plan)");
    int64_t most = 0;
    for (int k = 0; k < p.ncls; ++k) {
        const int64_t t = (int64_t)p.N * p.cls[k].Hg * p.cls[k].Wg;
        if (t >= (1ll << 31) || (int64_t)(p.N + 1) * (p.Hs + 2) >= (1ll << 31)) return hip_fail(hipErrorInvalidValue, "k_gconv: more than 2^31 positions");
        most = t > most ? t : most;
    }
    if (most == 0) return 0;
    if (p.gate_out && (p.ncls != 1 || p.os != 1 || p.cls[0].Hg != p.Ho || p.cls[0].Wg != p.Wo))
        return hip_fail(hipErrorInvalidValue, "k_gconv: gate rows are written by dense forward launches only");
    const int P = 64 * p.waves;
    const dim3 grid((unsigned)((most + P - 1) / P), (unsigned)p.groups, (unsigned)p.ncls);
    if (grid.y > 65535u) return hip_fail(hipErrorInvalidValue, "k_gconv: more than 65535 groups");
    __atomic_fetch_add(&g_stat_gconv, 1, __ATOMIC_RELAXED);
    switch (p.gw) {
        case 4: return gconv_launch<4, 4>(p, grid, s);
        case 8: return gconv_launch<8, 8>(p, grid, s);
        case 16: return gconv_launch<16, 16>(p, grid, s);
        case 32: return gconv_launch<32, 16>(p, grid, s);
        case 64: return gconv_launch<64, 16>(p, grid, s);
    }
    return hip_fail(hipErrorInvalidValue, "k_gconv: group width not in {4, 8, 16, 32, 64}");
}
