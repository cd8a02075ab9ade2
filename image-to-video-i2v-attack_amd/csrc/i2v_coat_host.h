// The CoaT launches (i2v_coat_kernels.h) as plain scalar C++ on the backend's memory: what the planner runs where the library has no
// i2v_coat.hip (no -DI2V_HAVE_COAT: the host simulation's one-file build, whose backend memory is host memory).  The same definitions
// and the same refusals as the kernels.  The attention restates the definitions -- the column maximum first, then one pass in increasing
// token order -- and NOT the device's tiled order, so it is held to the float64 bound, not to the device's bits.  The convolution and
// the cell launches add in the device's order.  Only expf and logf are the host's own.
#pragma once
#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include <algorithm>
#include <vector>

#include "i2v_kernels.h"
#include "i2v_coat_kernels.h"

inline int coat_host_refuse(const char* who, const char* why) {
    char buf[256];
    snprintf(buf, sizeof buf, "%s: hipErrorInvalidValue: %s", who, why);
    return i2v_api_fail(buf);
}

inline int coat_attention(const CoatAttn& p, hipStream_t) {
    if (const char* why = coat_attn_refusal(p, false)) return coat_host_refuse("coat_attention", why);
    const int T = p.T, H = p.H, dh = p.dh, C = H * dh;
    for (int64_t f = 0; f < p.F; ++f)
        for (int h = 0; h < H; ++h) {
            const float *q = p.qkv + f * T * 3 * C + h * dh, *k = q + C, *v = q + 2 * C;
            float *G = p.gram + (f * H + h) * dh * dh, *st = p.kstat + (f * H + h) * 2 * dh;
            for (int a = 0; a < dh; ++a) {
                float m = -INFINITY, l = 0.f;
                for (int t = 0; t < T; ++t) m = fmaxf(m, k[(int64_t)t * 3 * C + a]);
                for (int b = 0; b < dh; ++b) G[a * dh + b] = 0.f;
                for (int t = 0; t < T; ++t) {
                    const float e = expf(k[(int64_t)t * 3 * C + a] - m);
                    l = l + e;
                    for (int b = 0; b < dh; ++b) G[a * dh + b] = fmaf(e, v[(int64_t)t * 3 * C + b], G[a * dh + b]);
                }
                for (int b = 0; b < dh; ++b) G[a * dh + b] = G[a * dh + b] / l;
                st[a] = m;
                st[dh + a] = logf(l);
            }
            for (int t = 0; t < T; ++t)
                for (int b = 0; b < dh; ++b) {
                    float acc = 0.f;
                    for (int a = 0; a < dh; ++a) acc = fmaf(q[(int64_t)t * 3 * C + a], G[a * dh + b], acc);
                    const int64_t at = (f * T + t) * C + h * dh + b;
                    p.out[at] = acc * p.scale + q[(int64_t)t * 3 * C + b] * p.E[at];
                }
        }
    return 0;
}

inline int coat_attention_bwd(const CoatAttn& p, hipStream_t) {
    if (const char* why = coat_attn_refusal(p, true)) return coat_host_refuse("coat_attention_bwd", why);
    const int T = p.T, H = p.H, dh = p.dh, C = H * dh;
    std::vector<float> c((size_t)dh);
    for (int64_t f = 0; f < p.F; ++f)
        for (int h = 0; h < H; ++h) {
            const float *q = p.qkv + f * T * 3 * C + h * dh, *k = q + C, *v = q + 2 * C;
            const float *G = p.gram + (f * H + h) * dh * dh, *st = p.kstat + (f * H + h) * 2 * dh;
            const float *g = p.dout + f * T * C + h * dh, *E = p.E + f * T * C + h * dh;
            float *dG = p.dgram + (f * H + h) * dh * dh, *dq = p.dqkv + f * T * 3 * C + h * dh, *dk = dq + C, *dv = dq + 2 * C;
            float* dE = p.dE + f * T * C + h * dh;
            for (int a = 0; a < dh; ++a) {
                for (int b = 0; b < dh; ++b) {
                    float acc = 0.f;
                    for (int t = 0; t < T; ++t) acc = fmaf(q[(int64_t)t * 3 * C + a], g[(int64_t)t * C + b], acc);
                    dG[a * dh + b] = acc * p.scale;
                }
                c[a] = 0.f;
                for (int b = 0; b < dh; ++b) c[a] = fmaf(G[a * dh + b], dG[a * dh + b], c[a]);
            }
            for (int t = 0; t < T; ++t) {
                const float *qr = q + (int64_t)t * 3 * C, *kr = k + (int64_t)t * 3 * C, *vr = v + (int64_t)t * 3 * C, *gr = g + (int64_t)t * C;
                for (int a = 0; a < dh; ++a) {
                    float sq = 0.f, sv = 0.f, sk = 0.f;
                    for (int b = 0; b < dh; ++b) {
                        sq = fmaf(gr[b], G[a * dh + b], sq);                                        // dout G^T
                        sk = fmaf(vr[b], dG[a * dh + b], sk);                                       // v dG^T
                        sv = fmaf(expf((kr[b] - st[b]) - st[dh + b]), dG[b * dh + a], sv);          // Ks dG, column a
                    }
                    dq[(int64_t)t * 3 * C + a] = sq * p.scale + gr[a] * E[(int64_t)t * C + a];
                    dE[(int64_t)t * C + a] = gr[a] * qr[a];
                    dv[(int64_t)t * 3 * C + a] = sv;
                    dk[(int64_t)t * 3 * C + a] = expf((kr[a] - st[a]) - st[dh + a]) * (sk - c[a]);
                }
            }
        }
    return 0;
}

// one output element of either direction; mirror: the backward's gather over the mirrored filter
inline float coat_host_dw_at(const CoatDw& p, const float* plane, int64_t rs, int py, int px, int c, bool mirror) {
    const int g = p.g, n7 = p.C - p.n3 - p.n5;
    const int K = c < p.n3 ? 3 : c < p.n3 + p.n5 ? 5 : 7, n = K == 3 ? p.n3 : K == 5 ? p.n5 : n7, cl = K == 3 ? c : K == 5 ? c - p.n3 : c - p.n3 - p.n5;
    const float* w = K == 3 ? p.w3 : K == 5 ? p.w5 : p.w7;
    float acc = !mirror && p.b ? p.b[c] : 0.f;
    for (int ky = 0; ky < K; ++ky)
        for (int kx = 0; kx < K; ++kx) {
            const int iy = mirror ? py + K / 2 - ky : py + ky - K / 2, ix = mirror ? px + K / 2 - kx : px + kx - K / 2;
            if (iy < 0 || iy >= g || ix < 0 || ix >= g) continue;
            acc = fmaf(w[(int64_t)(ky * K + kx) * n + cl], plane[((int64_t)iy * g + ix) * rs + c], acc);
        }
    return acc;
}

inline int coat_host_dw(const CoatDw& p, bool bwd) {
    const int g = p.g, R = p.prefix + g * g;
    for (int64_t f = 0; f < p.F; ++f)
        for (int t = 0; t < R; ++t)
            for (int c = 0; c < p.C; ++c) {
                const float xc = p.x[(f * R + t) * p.xrs + c];
                float* y = p.y + (f * R + t) * p.yrs + c;
                float v;
                if (t < p.prefix) {
                    if (bwd && p.accumulate && !p.residual) continue;
                    v = p.residual ? xc : 0.f;
                } else {
                    v = coat_host_dw_at(p, p.x + (f * R + p.prefix) * p.xrs, p.xrs, (t - p.prefix) / g, (t - p.prefix) % g, c, bwd);
                    if (p.residual) v = xc + v;
                }
                *y = bwd && p.accumulate ? *y + v : v;
            }
    return 0;
}

inline int coat_dwmix(const CoatDw& p, hipStream_t) {
    if (const char* why = coat_dw_refusal(p)) return coat_host_refuse("coat_dwmix", why);
    return coat_host_dw(p, false);
}

inline int coat_dwmix_bwd(const CoatDw& p, hipStream_t) {
    if (const char* why = coat_dw_refusal(p)) return coat_host_refuse("coat_dwmix_bwd", why);
    return coat_host_dw(p, true);
}

inline int coat_host_cells(const CoatCells& p, bool scatter) {
    const int g = p.g, C = p.C, s = p.s, go = g / s, R = p.prefix + g * g;
    for (int64_t f = 0; f < p.F; ++f)
        for (int t = 0; t < R; ++t)
            for (int c = 0; c < C; ++c) {
                const int64_t at = (f * R + t) * C + c;
                if (t < p.prefix) {
                    if (scatter && !p.accumulate) p.dst[at] = 0.f;
                    continue;
                }
                const int py = (t - p.prefix) / g, px = (t - p.prefix) % g;
                const int64_t row = (f * go + py / s) * go + px / s, col = (int64_t)((py % s) * s + px % s) * C + c;
                if (!scatter) p.dst[row * s * s * C + col] = p.src[at];
                else p.dst[at] = p.accumulate ? p.dst[at] + p.src[row * s * s * C + col] : p.src[row * s * s * C + col];
            }
    return 0;
}

inline int coat_cell_gather(const CoatCells& p, hipStream_t) {
    if (const char* why = coat_cells_refusal(p)) return coat_host_refuse("coat_cell_gather", why);
    return coat_host_cells(p, false);
}

inline int coat_cell_scatter(const CoatCells& p, hipStream_t) {
    if (const char* why = coat_cells_refusal(p)) return coat_host_refuse("coat_cell_scatter", why);
    return coat_host_cells(p, true);
}
