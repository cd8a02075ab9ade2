// The XCiT launches (i2v_xcit_kernels.h) as plain scalar C++ on the backend's memory: what the planner runs where the library has no
// i2v_xcit.hip (no -DI2V_HAVE_XCIT: the host simulation's one-file build, whose backend memory is host memory).  The same definitions and
// the same refusals as the kernels; the ORDER of the sums is the simplest one (one fma chain in increasing index, a plain running sum over
// a row) and is NOT the device's, so these are held to the float64 bound, not to the device's bits.  Only expf / erff are the host's own.
#pragma once
#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "i2v_gelu.h"
#include "i2v_kernels.h"
#include "i2v_xcit_kernels.h"

inline int xcit_host_refuse(const char* who, const char* why) {
    char buf[256];
    snprintf(buf, sizeof buf, "%s: hipErrorInvalidValue: %s", who, why);
    return i2v_api_fail(buf);
}

inline int xcit_attention(const XcitAttn& p, hipStream_t) {
    if (const char* why = xcit_attn_refusal(p, false)) return xcit_host_refuse("xcit_attention", why);
    const int T = p.T, H = p.H, dh = p.dh, C = H * dh;
    std::vector<float> S((size_t)dh);
    for (int f = 0; f < p.F; ++f)
        for (int h = 0; h < H; ++h) {
            const float *q = p.qkv + (int64_t)f * T * 3 * C + h * dh, *k = q + C, *v = q + 2 * C;
            float* gram = p.gram + ((int64_t)f * H + h) * (dh + 2) * dh;
            float* A = p.probs + ((int64_t)f * H + h) * dh * dh;
            float *nq = gram + dh * dh, *nk = nq + dh;
            for (int c = 0; c < dh; ++c) {
                float sq = 0.f, sk = 0.f;
                for (int t = 0; t < T; ++t) {
                    sq = fmaf(q[(int64_t)t * 3 * C + c], q[(int64_t)t * 3 * C + c], sq);
                    sk = fmaf(k[(int64_t)t * 3 * C + c], k[(int64_t)t * 3 * C + c], sk);
                }
                nq[c] = fmaxf(sqrtf(sq), XCIT_NORM_EPS);
                nk[c] = fmaxf(sqrtf(sk), XCIT_NORM_EPS);
            }
            for (int i = 0; i < dh; ++i) {
                float m = -INFINITY, sum = 0.f;
                for (int j = 0; j < dh; ++j) {
                    float acc = 0.f;
                    for (int t = 0; t < T; ++t) acc = fmaf(q[(int64_t)t * 3 * C + i], k[(int64_t)t * 3 * C + j], acc);
                    gram[i * dh + j] = acc / nq[i] / nk[j];
                    S[j] = p.temperature[h] * gram[i * dh + j];
                    m = fmaxf(m, S[j]);
                }
                for (int j = 0; j < dh; ++j) { S[j] = expf(S[j] - m); sum = sum + S[j]; }
                for (int j = 0; j < dh; ++j) A[i * dh + j] = S[j] / sum;
            }
            for (int t = 0; t < T; ++t)
                for (int i = 0; i < dh; ++i) {
                    float acc = 0.f;
                    for (int j = 0; j < dh; ++j) acc = fmaf(A[i * dh + j], v[(int64_t)t * 3 * C + j], acc);
                    p.out[((int64_t)f * T + t) * C + h * dh + i] = acc;
                }
        }
    return 0;
}

inline int xcit_attention_bwd(const XcitAttn& p, hipStream_t) {
    if (const char* why = xcit_attn_refusal(p, true)) return xcit_host_refuse("xcit_attention_bwd", why);
    const int T = p.T, H = p.H, dh = p.dh, C = H * dh;
    std::vector<float> dG((size_t)dh * dh), r((size_t)dh), c((size_t)dh);
    for (int f = 0; f < p.F; ++f)
        for (int h = 0; h < H; ++h) {
            const float *q = p.qkv + (int64_t)f * T * 3 * C + h * dh, *k = q + C, *v = q + 2 * C;
            const float* dout = p.dout + (int64_t)f * T * C + h * dh;
            float* dq = p.dqkv + (int64_t)f * T * 3 * C + h * dh;
            const float* gram = p.gram + ((int64_t)f * H + h) * (dh + 2) * dh;
            const float* A = p.probs + ((int64_t)f * H + h) * dh * dh;
            const float *nq = gram + dh * dh, *nk = nq + dh;
            for (int j = 0; j < dh; ++j) c[j] = 0.f;
            for (int i = 0; i < dh; ++i) {
                float s = 0.f, ri = 0.f;
                for (int j = 0; j < dh; ++j) {
                    float acc = 0.f;
                    for (int t = 0; t < T; ++t) acc = fmaf(dout[(int64_t)t * C + i], v[(int64_t)t * 3 * C + j], acc);
                    dG[i * dh + j] = acc;                                  // dA for now
                    s = s + acc * A[i * dh + j];
                }
                for (int j = 0; j < dh; ++j) {
                    const float g = p.temperature[h] * (A[i * dh + j] * (dG[i * dh + j] - s));
                    dG[i * dh + j] = g;
                    ri = ri + g * gram[i * dh + j];
                    c[j] = c[j] + g * gram[i * dh + j];
                }
                r[i] = ri;
            }
            for (int t = 0; t < T; ++t) {
                const int64_t o = (int64_t)t * 3 * C;
                for (int j = 0; j < dh; ++j) {
                    float av = 0.f, ak = 0.f;
                    for (int i = 0; i < dh; ++i) {
                        av = fmaf(dout[(int64_t)t * C + i], A[i * dh + j], av);
                        ak = fmaf(q[o + i], dG[i * dh + j] / nq[i], ak);
                    }
                    dq[o + 2 * C + j] = av;
                    dq[o + C + j] = (ak - k[o + j] * (c[j] / nk[j])) / nk[j];
                }
                for (int i = 0; i < dh; ++i) {
                    float aq = 0.f;
                    for (int j = 0; j < dh; ++j) aq = fmaf(k[o + j], dG[i * dh + j] / nk[j], aq);
                    dq[o + i] = (aq - q[o + i] * (r[i] / nq[i])) / nq[i];
                }
            }
        }
    return 0;
}

inline int xcit_dw3(const XcitDw3& p, hipStream_t) {
    if (const char* why = xcit_dw3_refusal(p)) return xcit_host_refuse("xcit_dw3", why);
    for (int64_t n = 0; n < p.N; ++n)
        for (int y = 0; y < p.H; ++y)
            for (int x = 0; x < p.W; ++x)
                for (int c = 0; c < p.C; ++c) {
                    float acc = p.b ? p.b[c] : 0.f;
                    for (int ky = 0; ky < 3; ++ky)
                        for (int kx = 0; kx < 3; ++kx) {
                            const int yy = y + ky - 1, xx = x + kx - 1;
                            if (yy < 0 || yy >= p.H || xx < 0 || xx >= p.W) continue;
                            float v = p.x[((n * p.H + yy) * p.W + xx) * p.C + c];
                            if (p.ta) v = fmaf(p.ta[c], gelu_host_f(v), p.ts[c]);
                            acc = fmaf(p.w[(3 * ky + kx) * p.C + c], v, acc);
                        }
                    const int64_t o = ((n * p.H + y) * p.W + x) * p.C + c;
                    if (p.add) acc = acc + p.add[o];
                    if (p.ma) acc = acc * (p.ma[c] * gelu_grad_host_f(p.mu[o]));
                    p.y[o] = acc;
                }
    return 0;
}

inline int xcit_stem_gather(const float* src, float* rows, int F, int H, int W, int C, int nchw, hipStream_t) {
    if (const char* why = xcit_stem_refusal(src, rows, F, H, W, C)) return xcit_host_refuse("xcit_stem_gather", why);
    const int Ho = (H + 1) / 2, Wo = (W + 1) / 2;
    for (int64_t f = 0; f < F; ++f)
        for (int oy = 0; oy < Ho; ++oy)
            for (int ox = 0; ox < Wo; ++ox)
                for (int tap = 0; tap < 9; ++tap)
                    for (int c = 0; c < C; ++c) {
                        const int y = 2 * oy - 1 + tap / 3, x = 2 * ox - 1 + tap % 3;
                        const bool in = y >= 0 && y < H && x >= 0 && x < W;
                        rows[((f * Ho + oy) * Wo + ox) * 9 * C + tap * C + c] =
                            !in ? 0.f : nchw ? src[((f * C + c) * H + y) * W + x] : src[((f * H + y) * W + x) * C + c];
                    }
    return 0;
}

inline int xcit_stem_scatter(const float* drows, const float* pre, float* dst, int F, int H, int W, int C, int nchw, int accumulate, hipStream_t) {
    const char* why = xcit_stem_refusal(drows, dst, F, H, W, C);
    if (!why && ((uintptr_t)pre & 15)) why = "16-byte alignment needed";
    if (!why && nchw && pre) why = "the image layout takes no pre-activation";
    if (!why && !nchw && accumulate) why = "only the image layout accumulates";
    if (why) return xcit_host_refuse("xcit_stem_scatter", why);
    const int Ho = (H + 1) / 2, Wo = (W + 1) / 2;
    for (int64_t f = 0; f < F; ++f)
        for (int y = 0; y < H; ++y)
            for (int x = 0; x < W; ++x)
                for (int c = 0; c < C; ++c) {
                    float acc = 0.f;
                    for (int ky = 0; ky < 3; ++ky)
                        for (int kx = 0; kx < 3; ++kx) {
                            const int ty = y + 1 - ky, tx = x + 1 - kx;
                            if (ty < 0 || (ty & 1) || ty / 2 >= Ho || tx < 0 || (tx & 1) || tx / 2 >= Wo) continue;
                            acc = acc + drows[((f * Ho + ty / 2) * Wo + tx / 2) * 9 * C + (3 * ky + kx) * C + c];
                        }
                    const int64_t tm = ((f * H + y) * W + x) * C + c;
                    if (pre) acc = acc * gelu_grad_host_f(pre[tm]);
                    float* o = dst + (nchw ? ((f * C + c) * H + y) * W + x : tm);
                    *o = accumulate ? *o + acc : acc;
                }
    return 0;
}
