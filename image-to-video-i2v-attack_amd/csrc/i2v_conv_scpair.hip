// Shortcut pair: a projection shortcut `a` (1x1, `+ shift` and nothing else) and the expand convolution `b` that adds its output, as
// ONE launch -- two K loops into one 64x64 output tile (k_conv_scpair, i2v_kernels.h).  Run as two launches, `a` writes Cd channels per
// pixel that `b` reads back once as add0 and nobody else ever reads: at 56^2 that round trip is 2 x 411 MB per forward pass on launches
// that sit on the HBM roof.  Here a block
//   1. runs a's K loop (conv_tile_loop, MODE 1 pointwise -- or MODE 2 for the tap-uniform 1x1 of a strided shortcut),
//   2. takes the sums through the epilogue's LDS transposition (conv_acc_to_rows) and forms y = acc_a + a.shift[cd] per lane, in the
//      row layout of the dense epilogue: 4 consecutive pixels of 4 channel rows, 16 registers -- exactly the registers the prefetching
//      tile keeps its first addend in (pre0),
//   3. runs b's K loop (MODE 1, with b's gate words prefetched under it),
//   4. runs b's dense epilogue (conv_vec_epilogue, PREF) with y where the prefetched addend would be:
//      v = acc_b + b.shift + y (+ add1), ReLU, gates, 16-byte store.
// Every output element is the same two k-ordered fmaf chains and the same additions in the same order as in the two launches (an fp32
// MFMA IS such a chain; -ffp-contract=off), so the result is bit-identical and the planner may choose per batch bucket by time alone.
// Budget: the registers of the prefetching 64x64 tile (accumulator 16 + y 16 + gate words 4 beside the loop's own) and the 24 KB of
// its three-buffer pointwise loop: 6 resident blocks per CU, which is what the kernel is compiled for.
#include "i2v_conv_tile.h"

#ifndef I2V_SCPAIR_WPE
#define I2V_SCPAIR_WPE I2V_PREF_WPE
#endif

template <int MODE_A>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(I2V_SCPAIR_WPE, I2V_SCPAIR_WPE)))
conv_igemm_scpair(const I2VConvParams a, const I2VConvParams b, const int n_cd_tiles) {
    constexpr int BD = 64, BP = 64, WD = 2, WP = 2, FR = 32;
    constexpr bool PREF_A = MODE_A == 1;         // (the pointwise loop's deeper prefetch comes with the PREF variant; `a` has nothing to prefetch)
    constexpr int LA = conv_lds_floats<BD, BP, WD, false, conv_deep(MODE_A, PREF_A) ? I2V_DEEP_STAGES : 2>();
    constexpr int LB = conv_lds_floats<BD, BP, WD, false, conv_deep(1, true) ? I2V_DEEP_STAGES : 2>();
    __shared__ __attribute__((aligned(16))) float smem[LA > LB ? LA : LB];
    I2V_PROBE_T probe;
    probe.entry();
    const int lid = conv_xcd_lid(blockIdx.x, gridDim.x);
    const int cd0 = (lid % n_cd_tiles) * BD;
    const int64_t px0 = (int64_t)(lid / n_cd_tiles) * BP;

    constexpr int C4 = BP / 4, RSTEP = 1024 / BP, NQ = WD * FR / RSTEP;
    float4 y[NQ];
    {
        f32x16 acc[1][1];
        float4 pre_a[PREF_A ? NQ : 1]; unsigned gw_a[PREF_A ? NQ : 1];
        conv_tile_loop<BD, BP, WD, WP, MODE_A, PREF_A>(a, cd0, px0, gridDim.x, smem, probe, blockIdx.x, I2V_PRIO_LEVELS, acc, pre_a, gw_a);
        float (*Cs)[BP] = reinterpret_cast<float (*)[BP]>(smem);
        conv_acc_to_rows<BP, WP, false>(acc[0], Cs);
        // the rows and pixels conv_vec_rows gives this lane
        const int t = threadIdx.x, c4 = t % C4, rbase = t / C4;
        const bool pok = px0 + (int64_t)c4 * 4 < (int64_t)a.N * a.Hg * a.Wg;
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            const int row = rbase + q * RSTEP, cd = cd0 + row;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (pok && cd < a.Cd) {
                v = *reinterpret_cast<const float4*>(&Cs[row][c4 * 4]);
                if (a.shift) { const float sh = a.shift[cd]; v.x += sh; v.y += sh; v.z += sh; v.w += sh; }
            }
            y[q] = v;
        }
        __syncthreads();      // every lane has read its rows: b's loop may stage into the same LDS
    }
    f32x16 acc[1][1];
    float4 pre0[NQ]; unsigned pregw[NQ];
    conv_tile_loop<BD, BP, WD, WP, 1, true>(b, cd0, px0, gridDim.x, smem, probe, blockIdx.x, I2V_PRIO_LEVELS, acc, pre0, pregw);      // (b.add0 is null here: pre0 comes back as zeros)
#pragma unroll
    for (int q = 0; q < NQ; ++q) pre0[q] = y[q];
    conv_vec_epilogue<BD, BP, WD, WP, true, false, false>(b, acc, cd0, px0, smem, pre0, pregw, nullptr);
    probe.exit(blockIdx.x);
}

long long g_stat_scpair = 0;

int k_conv_scpair_ok(const I2VConvParams& a, const I2VConvParams& b) { return i2v_conv_scpair_ok(a, b) ? 1 : 0; }

int k_conv_scpair(const I2VConvParams& a_in, const I2VConvParams& b_in, i2v_stream_t s) {
    I2VConvParams a = a_in, b = b_in;
    if (!i2v_conv_scpair_ok(a, b)) { snprintf(g_be_err, sizeof g_be_err, "shortcut-pair launch: the two launches do not form a pair"); g_be_has_err = true; return 1; }
    const int64_t P = (int64_t)b.N * b.Hg * b.Wg;
    if (P + 1024 >= (1ll << 31)) { snprintf(g_be_err, sizeof g_be_err, "conv launch of more than 2^31 grid pixels"); g_be_has_err = true; return 1; }
    conv_magics(a); conv_magics(b);
    b.add0 = nullptr; b.add0_nstride = 0;          // the addend never leaves the chip
    const int n_cd = (b.Cd + 63) / 64;
    const int64_t grid = (P + 63) / 64 * n_cd;
    if (grid <= 0) return 0;
    if (grid > 0x7fffffff) { snprintf(g_be_err, sizeof g_be_err, "conv grid too large"); g_be_has_err = true; return 1; }
    __atomic_fetch_add(&g_stat_scpair, 1, __ATOMIC_RELAXED);
    if (a.pointwise) hipLaunchKernelGGL((conv_igemm_scpair<1>), dim3((unsigned)grid), dim3(256), 0, (hipStream_t)s, a, b, n_cd);
    else hipLaunchKernelGGL((conv_igemm_scpair<2>), dim3((unsigned)grid), dim3(256), 0, (hipStream_t)s, a, b, n_cd);
    LAUNCH_CHECK("conv_scpair");
    return 0;
}
