// The 8-bit export and the quality launches for gfx950 (i2v_quality_kernels.h, which states the arithmetic): what an attack's clip is
// worth as a video -- SSE and the largest difference in levels, and Wang et al.'s SSIM, per frame, of two clips that are already on the
// device, as 8-bit frames (frames, h, w, 3) or as normalised fp32 clips (clips, 3, t, h, w).
//
// SSIM LAUNCH.  Per frame and channel an 11 x 11 Gaussian over five moment maps of the two operands, the formula, a mean: about 150
// fma per valid position against 6 bytes (u8) or 24 bytes (f32) of input per pixel.  The window sums and the formula are fp64 vector
// arithmetic on fp32 operands (i2v_quality_kernels.h says why); no MFMA: the window is separable and the sums are short.  A workgroup of
// 256 threads works one 16 x 32 tile of the valid map off, all three channels, and loops over (frame, tile) items, so neither the frame
// count nor the frame size is bounded by the grid:
//   - u8: the tile's 26 rows of 126 interleaved bytes of both operands are staged ONCE, as they lie, with aligned 4-byte loads (a row of
//     3 w bytes starts at any alignment: each row keeps its own skew in LDS; the aligned word around a row's first or last byte is read
//     whole, which stays inside that byte's 4-byte granule); the channel passes read them from LDS.
//     f32: the channel's 26 x 42 floats of both operands are staged per channel, as centred levels -- the planes are separate memory.
//     Either way every byte of an operand comes from memory once per tile, apart from the 10-pixel halo its neighbours stage as well;
//   - horizontal pass: thread = (row, column), lanes along the columns (LDS reads without conflicts), the five row sums into LDS;
//   - vertical pass: thread = (column, 2 consecutive rows): 12 rows of a map in registers serve 2 positions, then the formula;
//   - the thread's SSIM sum, squared differences and largest difference (of the pixels the tile OWNS) go through a fixed fold in LDS, one
//     partial of three doubles per tile to scratch.  A second launch folds a frame's partials in a fixed order.  No atomics anywhere.
// LDS: 8.7 KB staging + 33.3 KB row sums (the fold's 6 KB lie over them) = 42 KB, three workgroups per CU.
// EXPORT: one thread per pixel, three channel planes read along the row, three bytes written.
#include <algorithm>

#include "i2v_be.h"
#include "i2v_quality_kernels.h"
#include "i2v_vit_kernels.h"     // vit_launch_check

long long g_stat_quality = 0;

namespace {

__constant__ float c_tap[QL_TAPS] = {QL_TAP_LITERALS};
__constant__ float c_qmean[3] = {QL_MEAN_LITERALS};
__constant__ float c_qstd[3] = {QL_STD_LITERALS};

constexpr int U8_ROW = 136;                                   // 3 (skew) + 126 bytes, rounded up to 8
constexpr int STAGE_BYTES = 2 * QL_IR * QL_IC * 4;            // f32: both operands of one channel; u8 needs 2 * 26 * 136 bytes, fewer
constexpr int H_DOUBLES = 5 * QL_IR * QL_TC;
static_assert(2 * QL_IR * U8_ROW <= STAGE_BYTES, "the u8 rows fit the staging area");
static_assert(3 * QL_THREADS <= H_DOUBLES, "the fold fits over the row sums");
static_assert(QL_THREADS == QL_TC * (QL_TR / QL_YB), "one thread per column and group of rows");

template <bool U8>
__global__ void __launch_bounds__(QL_THREADS) ql_tile_kernel(QlClips p, int nty, int ntx, int64_t items) {
    __shared__ __attribute__((aligned(16))) unsigned char stage[STAGE_BYTES];
    __shared__ __attribute__((aligned(16))) double Hs[H_DOUBLES];
    float* const sa = reinterpret_cast<float*>(stage);
    float* const sb = sa + QL_IR * QL_IC;
    unsigned char* const ua = stage;
    unsigned char* const ub = stage + QL_IR * U8_ROW;
    const int t = threadIdx.x, h = p.h, w = p.w, oh = h - QL_HALO, ow = w - QL_HALO;
    const int64_t tiles = (int64_t)nty * ntx, hw = (int64_t)h * w;
    double tap[QL_TAPS];
#pragma unroll
    for (int k = 0; k < QL_TAPS; ++k) tap[k] = (double)c_tap[k];

    for (int64_t item = blockIdx.x; item < items; item += gridDim.x) {
        const int64_t n = item / tiles;
        const int ti = (int)(item - n * tiles), ty = ti / ntx, tx = ti - ty * ntx, y0 = ty * QL_TR, x0 = tx * QL_TC;
        const bool lasty = ty == nty - 1, lastx = tx == ntx - 1;
        const int rows = min(QL_IR, h - y0), cols = min(QL_IC, w - x0);          // staged pixels inside the frame
        double sse = 0.0, ss = 0.0;
        double dmx = 0.0;
        int rskew_a = 0, rskew_b = 0;                                            // u8: the skews of row 0; a row adds 3 w
        __syncthreads();                                                        // the previous item's fold has been read

        if (U8) {
            // rows of `cols * 3` bytes at a + ((n h + y0 + r) w + x0) 3, as aligned words; word k of row r lands at r * U8_ROW + 4 k
            const uint8_t* ga = (const uint8_t*)p.a + ((n * h + y0) * (int64_t)w + x0) * 3;
            const uint8_t* gb = (const uint8_t*)p.b + ((n * h + y0) * (int64_t)w + x0) * 3;
            rskew_a = (int)((uintptr_t)ga & 3); rskew_b = (int)((uintptr_t)gb & 3);
            constexpr int WPR = U8_ROW / 4;                                      // 34 word slots a row
            for (int e = t; e < 2 * QL_IR * WPR; e += QL_THREADS) {
                const int op = e / (QL_IR * WPR), r = (e / WPR) % QL_IR, k = e % WPR;
                uint32_t v = 0;
                if (r < rows) {
                    const uint8_t* row = (op ? gb : ga) + (int64_t)r * w * 3;
                    const int skew = (int)((uintptr_t)row & 3);
                    if (4 * k < skew + cols * 3) v = *reinterpret_cast<const uint32_t*>(row - skew + 4 * k);
                }
                *reinterpret_cast<uint32_t*>((op ? ub : ua) + r * U8_ROW + 4 * k) = v;
            }
            __syncthreads();
            // SSE and max of the owned elements, in integers
            uint32_t isse = 0;
            int imx = 0;
            const int orows = lasty ? rows : min(rows, QL_TR), ocols = lastx ? cols : min(cols, QL_TC);
            for (int e = t; e < QL_IR * QL_IC * 3; e += QL_THREADS) {
                const int c = e % 3, q = (e / 3) % QL_IC, r = e / (3 * QL_IC);
                if (r < orows && q < ocols) {
                    const int oa = r * U8_ROW + ((rskew_a + r * w * 3) & 3) + q * 3 + c, ob = r * U8_ROW + ((rskew_b + r * w * 3) & 3) + q * 3 + c;
                    const int d = (int)ua[oa] - (int)ub[ob];
                    isse += (uint32_t)(d * d);
                    imx = max(imx, abs(d));
                }
            }
            sse = (double)isse;
            dmx = (double)imx;
        }

        for (int c = 0; c < 3; ++c) {
            if (!U8) {                                                          // (a barrier lies between this and the last read of sa, sb)
                const int64_t clip = n / p.t, f = n - clip * p.t;
                const int64_t base = ((clip * 3 + c) * p.t + f) * hw + (int64_t)y0 * w + x0;
                const float* ga = (const float*)p.a + base;
                const float* gb = (const float*)p.b + base;
                const float mean = c_qmean[c], sd = c_qstd[c];
                const double kd = 255.0 * (double)sd;
                for (int e = t; e < QL_IR * QL_IC; e += QL_THREADS) {
                    const int r = e / QL_IC, q = e - r * QL_IC;
                    float a = 0.f, b = 0.f;
                    if (r < rows && q < cols) {
                        const float xa = ga[(int64_t)r * w + q], xb = gb[(int64_t)r * w + q];
                        a = 255.f * fmaf(xa, sd, mean) - QL_CENTRE;
                        b = 255.f * fmaf(xb, sd, mean) - QL_CENTRE;
                        if ((r < QL_TR || lasty) && (q < QL_TC || lastx)) {
                            const double d = kd * ((double)xa - (double)xb);
                            sse = sse + d * d;
                            dmx = fmax(dmx, fabs(d));
                        }
                    }
                    sa[e] = a; sb[e] = b;
                }
            }
            __syncthreads();                                                    // staged; the previous channel's vertical pass has read Hs
            // horizontal: (row r, column x), lanes along x
            for (int e = t; e < QL_IR * QL_TC; e += QL_THREADS) {
                const int r = e / QL_TC, x = e - r * QL_TC;
                double ha = 0.0, hb = 0.0, haa = 0.0, hbb = 0.0, hab = 0.0;
                int oa = 0, ob = 0;
                if (U8) {
                    oa = r * U8_ROW + ((rskew_a + r * w * 3) & 3) + x * 3 + c;
                    ob = r * U8_ROW + ((rskew_b + r * w * 3) & 3) + x * 3 + c;
                }
#pragma unroll
                for (int k = 0; k < QL_TAPS; ++k) {
                    double a, b;
                    if (U8) {
                        // a row shorter than the tile (the frame's edge) holds zero words behind its bytes: level 0, and no valid position reads it
                        a = (double)((float)ua[oa + 3 * k] - QL_CENTRE); b = (double)((float)ub[ob + 3 * k] - QL_CENTRE);
                    } else {
                        a = (double)sa[r * QL_IC + x + k]; b = (double)sb[r * QL_IC + x + k];
                    }
                    const double aa = a * a, bb = b * b, ab = a * b;                 // exact: 24-bit factors
                    ha = fma(tap[k], a, ha); hb = fma(tap[k], b, hb); haa = fma(tap[k], aa, haa);
                    hbb = fma(tap[k], bb, hbb); hab = fma(tap[k], ab, hab);
                }
                Hs[(0 * QL_IR + r) * QL_TC + x] = ha; Hs[(1 * QL_IR + r) * QL_TC + x] = hb; Hs[(2 * QL_IR + r) * QL_TC + x] = haa;
                Hs[(3 * QL_IR + r) * QL_TC + x] = hbb; Hs[(4 * QL_IR + r) * QL_TC + x] = hab;
            }
            __syncthreads();
            // vertical: column x, rows yb, yb + 1 from 12 rows of every map
            {
                const int x = t % QL_TC, yb = QL_YB * (t / QL_TC);
                double M[QL_YB][5];
#pragma unroll
                for (int m = 0; m < 5; ++m) {
                    double v[QL_YB + QL_HALO];
#pragma unroll
                    for (int i = 0; i < QL_YB + QL_HALO; ++i) v[i] = Hs[(m * QL_IR + yb + i) * QL_TC + x];
#pragma unroll
                    for (int j = 0; j < QL_YB; ++j) {
                        double acc = 0.0;
#pragma unroll
                        for (int k = 0; k < QL_TAPS; ++k) acc = fma(tap[k], v[j + k], acc);
                        M[j][m] = acc;
                    }
                }
#pragma unroll
                for (int j = 0; j < QL_YB; ++j)
                    if (y0 + yb + j < oh && x0 + x < ow) ss = ss + ssim_value(M[j][0], M[j][1], M[j][2], M[j][3], M[j][4]);
            }
        }

        // the fold, over the row sums
        __syncthreads();
        double* const fs = Hs;
        double* const fm = fs + QL_THREADS;
        double* const fq = fm + QL_THREADS;
        fs[t] = sse; fm[t] = dmx; fq[t] = ss;
        __syncthreads();
        for (int s = QL_THREADS / 2; s > 0; s >>= 1) {
            if (t < s) {
                fs[t] = fs[t] + fs[t + s];
                fm[t] = fm[t + s] > fm[t] ? fm[t + s] : fm[t];
                fq[t] = fq[t] + fq[t + s];
            }
            __syncthreads();
        }
        if (t == 0) {
            double* part = p.scratch + item * 3;
            part[0] = fs[0]; part[1] = fm[0]; part[2] = fq[0];
        }
    }
}

__global__ void __launch_bounds__(QL_FIN_THREADS) ql_frame_kernel(QlClips p, int64_t tiles) {
    __shared__ double fs[QL_FIN_THREADS], fm[QL_FIN_THREADS], fq[QL_FIN_THREADS];
    const int t = threadIdx.x;
    for (int64_t n = blockIdx.x; n < p.frames; n += gridDim.x) {
        double sse = 0.0, mx = 0.0, ss = 0.0;
        for (int64_t i = t; i < tiles; i += QL_FIN_THREADS) {
            const double* q = p.scratch + (n * tiles + i) * 3;
            sse = sse + q[0];
            mx = q[1] > mx ? q[1] : mx;
            ss = ss + q[2];
        }
        __syncthreads();                                                        // the previous frame's fold has been read
        fs[t] = sse; fm[t] = mx; fq[t] = ss;
        __syncthreads();
        for (int s = QL_FIN_THREADS / 2; s > 0; s >>= 1) {
            if (t < s) {
                fs[t] = fs[t] + fs[t + s];
                fm[t] = fm[t + s] > fm[t] ? fm[t + s] : fm[t];
                fq[t] = fq[t] + fq[t + s];
            }
            __syncthreads();
        }
        if (t == 0) {
            p.out[3 * n] = fs[0]; p.out[3 * n + 1] = fm[0];
            p.out[3 * n + 2] = fq[0] / (double)(3ll * (p.h - QL_HALO) * (p.w - QL_HALO));
        }
    }
}

__global__ void __launch_bounds__(256) ql_export_kernel(QlExport p, int64_t hw, int64_t total) {
    for (int64_t o = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; o < total; o += (int64_t)gridDim.x * blockDim.x) {
        const int64_t i = o % hw, r = o / hw, ti = r % p.t, bi = r / p.t;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float x = p.video[((bi * 3 + c) * p.t + ti) * hw + i];
            const float u = fminf(fmaxf(fmaf(x, c_qstd[c], c_qmean[c]), 0.f), 1.f);
            int q = (int)rintf(255.f * u);
            if (p.ref) {
                const int rf = p.ref[o * 3 + c];
                q = min(max(q, max(rf - p.levels, 0)), min(rf + p.levels, 255));
            }
            p.frames[o * 3 + c] = (uint8_t)q;
        }
    }
}

int refuse(const char* who, const char* why) {
    char buf[256];
    snprintf(buf, sizeof buf, "%s: hipErrorInvalidValue: %s", who, why);
    return i2v_api_fail(buf);
}

}  // namespace

int ql_clip_quality(const QlClips& p, hipStream_t s) {
    const int nty = (p.h - QL_HALO + QL_TR - 1) / QL_TR, ntx = (p.w - QL_HALO + QL_TC - 1) / QL_TC;
    const int64_t tiles = (int64_t)nty * ntx, items = p.frames * tiles;
    const dim3 grid((unsigned)std::min<int64_t>(items, QL_MAX_GRID));
    if (p.u8) hipLaunchKernelGGL(ql_tile_kernel<true>, grid, dim3(QL_THREADS), 0, s, p, nty, ntx, items);
    else hipLaunchKernelGGL(ql_tile_kernel<false>, grid, dim3(QL_THREADS), 0, s, p, nty, ntx, items);
    if (int rc = vit_launch_check("clip_quality tiles")) return rc;
    hipLaunchKernelGGL(ql_frame_kernel, dim3((unsigned)std::min<int64_t>(p.frames, QL_MAX_GRID)), dim3(QL_FIN_THREADS), 0, s, p, tiles);
    __atomic_fetch_add(&g_stat_quality, 2, __ATOMIC_RELAXED);
    return vit_launch_check("clip_quality frames");
}

int ql_clip_to_u8(const QlExport& p, hipStream_t s) {
    const int64_t hw = (int64_t)p.h * p.w, total = (int64_t)p.b * p.t * hw;
    hipLaunchKernelGGL(ql_export_kernel, dim3((unsigned)std::min<int64_t>((total + 255) / 256, 1 << 20)), dim3(256), 0, s, p, hw, total);
    __atomic_fetch_add(&g_stat_quality, 1, __ATOMIC_RELAXED);
    return vit_launch_check("clip_to_u8");
}
