// The 8-bit export and the quality launches (i2v_quality_kernels.h) as plain scalar C++ on the backend's memory: what the C entries run
// where the library has no i2v_quality.hip (no -DI2V_HAVE_QUALITY: the host simulation's one-file build, whose backend memory is host
// memory).  The same definitions, the same owner of every pixel, the same order of every sum and the same refusals as the kernels: all
// three fields of every frame are held to the device's bits.
#pragma once
#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "i2v_kernels.h"
#include "i2v_quality_kernels.h"

inline int ql_host_refuse(const char* who, const char* why) {
    char buf[256];
    snprintf(buf, sizeof buf, "%s: hipErrorInvalidValue: %s", who, why);
    return i2v_api_fail(buf);
}

namespace ql_host {

const float kTap[QL_TAPS] = {QL_TAP_LITERALS};
const float kMean[3] = {QL_MEAN_LITERALS}, kStd[3] = {QL_STD_LITERALS};

// p[t] = p[t] + p[t + s] (max: the larger) for s = n / 2 .. 1
inline void fold(double* sse, double* mx, double* ss, int n) {
    for (int s = n / 2; s > 0; s >>= 1)
        for (int t = 0; t < s; ++t) {
            sse[t] = sse[t] + sse[t + s];
            mx[t] = mx[t + s] > mx[t] ? mx[t + s] : mx[t];
            ss[t] = ss[t] + ss[t + s];
        }
}

inline void tile(const QlClips& p, int64_t n, int ty, int tx, int nty, int ntx, double* part) {
    const int h = p.h, w = p.w, oh = h - QL_HALO, ow = w - QL_HALO, y0 = ty * QL_TR, x0 = tx * QL_TC;
    const int64_t hw = (int64_t)h * w;
    const bool lasty = ty == nty - 1, lastx = tx == ntx - 1;
    double sse[QL_THREADS], mx[QL_THREADS], ss[QL_THREADS];
    uint32_t isse[QL_THREADS] = {0};
    int imx[QL_THREADS] = {0};
    for (int t = 0; t < QL_THREADS; ++t) sse[t] = mx[t] = ss[t] = 0.0;
    std::vector<float> va(QL_IR * QL_IC), vb(QL_IR * QL_IC);
    std::vector<double> H(5 * QL_IR * QL_TC);
    for (int c = 0; c < 3; ++c) {
        for (int e = 0; e < QL_IR * QL_IC; ++e) {
            const int r = e / QL_IC, q = e % QL_IC, t = e % QL_THREADS;
            const bool in = y0 + r < h && x0 + q < w, own = in && (r < QL_TR || lasty) && (q < QL_TC || lastx);
            float a = 0.f, b = 0.f;
            if (in && p.u8) {
                const int64_t i = ((n * h + y0 + r) * w + x0 + q) * 3 + c;
                const int ia = ((const uint8_t*)p.a)[i], ib = ((const uint8_t*)p.b)[i];
                a = (float)ia - QL_CENTRE; b = (float)ib - QL_CENTRE;
                if (own) {                                               // (integers: the thread that takes the element does not matter)
                    const int d = ia - ib, ad = d < 0 ? -d : d;
                    isse[t] += (uint32_t)(d * d);
                    if (ad > imx[t]) imx[t] = ad;
                }
            } else if (in) {
                const int64_t clip = n / p.t, f = n % p.t, i = ((clip * 3 + c) * p.t + f) * hw + (int64_t)(y0 + r) * w + x0 + q;
                const float xa = ((const float*)p.a)[i], xb = ((const float*)p.b)[i];
                a = 255.f * fmaf(xa, kStd[c], kMean[c]) - QL_CENTRE;
                b = 255.f * fmaf(xb, kStd[c], kMean[c]) - QL_CENTRE;
                if (own) {
                    const double k = 255.0 * (double)kStd[c], d = k * ((double)xa - (double)xb);
                    sse[t] = sse[t] + d * d;
                    mx[t] = fmax(mx[t], fabs(d));
                }
            }
            va[e] = a; vb[e] = b;
        }
        // (only the row sums a valid position reads: the device forms all 26 x 32 and leaves the others unread)
        for (int r = 0; r < QL_IR && y0 + r < h; ++r)
            for (int x = 0; x < QL_TC && x0 + x < ow; ++x) {
                double acc[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
                for (int k = 0; k < QL_TAPS; ++k) {
                    const double g = (double)kTap[k], a = (double)va[r * QL_IC + x + k], b = (double)vb[r * QL_IC + x + k];
                    const double aa = a * a, bb = b * b, ab = a * b;
                    acc[0] = fma(g, a, acc[0]); acc[1] = fma(g, b, acc[1]); acc[2] = fma(g, aa, acc[2]);
                    acc[3] = fma(g, bb, acc[3]); acc[4] = fma(g, ab, acc[4]);
                }
                for (int m = 0; m < 5; ++m) H[(m * QL_IR + r) * QL_TC + x] = acc[m];
            }
        for (int t = 0; t < QL_THREADS; ++t)
            for (int j = 0; j < QL_YB; ++j) {
                const int x = t % QL_TC, y = QL_YB * (t / QL_TC) + j;
                if (y0 + y >= oh || x0 + x >= ow) continue;
                double M[5];
                for (int m = 0; m < 5; ++m) {
                    double acc = 0.0;
                    for (int k = 0; k < QL_TAPS; ++k) acc = fma((double)kTap[k], H[(m * QL_IR + y + k) * QL_TC + x], acc);
                    M[m] = acc;
                }
                ss[t] = ss[t] + ssim_value(M[0], M[1], M[2], M[3], M[4]);
            }
    }
    for (int t = 0; t < QL_THREADS; ++t) {
        if (p.u8) { sse[t] = (double)isse[t]; mx[t] = (double)imx[t]; }
    }
    fold(sse, mx, ss, QL_THREADS);
    part[0] = sse[0]; part[1] = mx[0]; part[2] = ss[0];
}

}  // namespace ql_host

inline int ql_clip_quality(const QlClips& p, hipStream_t) {
    const int nty = (p.h - QL_HALO + QL_TR - 1) / QL_TR, ntx = (p.w - QL_HALO + QL_TC - 1) / QL_TC;
    const int64_t tiles = (int64_t)nty * ntx;
    for (int64_t n = 0; n < p.frames; ++n) {
        for (int64_t i = 0; i < tiles; ++i) ql_host::tile(p, n, (int)(i / ntx), (int)(i % ntx), nty, ntx, p.scratch + (n * tiles + i) * 3);
        double sse[QL_FIN_THREADS], mx[QL_FIN_THREADS], ss[QL_FIN_THREADS];
        for (int t = 0; t < QL_FIN_THREADS; ++t) {
            sse[t] = mx[t] = ss[t] = 0.0;
            for (int64_t i = t; i < tiles; i += QL_FIN_THREADS) {
                const double* q = p.scratch + (n * tiles + i) * 3;
                sse[t] = sse[t] + q[0];
                mx[t] = q[1] > mx[t] ? q[1] : mx[t];
                ss[t] = ss[t] + q[2];
            }
        }
        ql_host::fold(sse, mx, ss, QL_FIN_THREADS);
        p.out[3 * n] = sse[0]; p.out[3 * n + 1] = mx[0];
        p.out[3 * n + 2] = ss[0] / (double)(3ll * (p.h - QL_HALO) * (p.w - QL_HALO));
    }
    return 0;
}

inline int ql_clip_to_u8(const QlExport& p, hipStream_t) {
    const int64_t hw = (int64_t)p.h * p.w;
    for (int64_t bi = 0; bi < p.b; ++bi)
        for (int ti = 0; ti < p.t; ++ti)
            for (int64_t i = 0; i < hw; ++i)
                for (int c = 0; c < 3; ++c) {
                    const float x = p.video[((bi * 3 + c) * p.t + ti) * hw + i];
                    const float u = fminf(fmaxf(fmaf(x, ql_host::kStd[c], ql_host::kMean[c]), 0.f), 1.f);
                    int q = (int)rintf(255.f * u);
                    const int64_t o = ((bi * p.t + ti) * hw + i) * 3 + c;
                    if (p.ref) {
                        const int r = p.ref[o], lo = r - p.levels < 0 ? 0 : r - p.levels, hi = r + p.levels > 255 ? 255 : r + p.levels;
                        q = q < lo ? lo : (q > hi ? hi : q);
                    }
                    p.frames[o] = (uint8_t)q;
                }
    return 0;
}
