// The TNT launches (i2v_tnt_kernels.h) as plain scalar C++ on the backend's memory: what the planner runs where the library has no
// i2v_tnt.hip (no -DI2V_HAVE_TNT: the host simulation's one-file build, whose backend memory is host memory).  The same definitions,
// the same order of every sum and the same refusals as the kernels; only expf is the host's own, so the attention is held to the
// float64 bound and the pixel pair and the row add to the device's bits.
#pragma once
#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include "i2v_kernels.h"
#include "i2v_tnt_kernels.h"

inline int tnt_host_refuse(const char* who, const char* why) {
    char buf[256];
    snprintf(buf, sizeof buf, "%s: hipErrorInvalidValue: %s", who, why);
    return i2v_api_fail(buf);
}

// row i of one (sequence, head): P[j], and with dout_i the row's dS[j]
inline void tnt_host_row(const float* q, const float* k, int64_t rs, int T, int dh, float scale, int i, float* P) {
    float m = -INFINITY, l = 0.f;
    for (int j = 0; j < T; ++j) {
        float acc = 0.f;
        for (int d = 0; d < dh; ++d) acc = fmaf(q[i * rs + d], k[j * rs + d], acc);
        P[j] = acc * scale;
        m = fmaxf(m, P[j]);
    }
    for (int j = 0; j < T; ++j) {
        P[j] = expf(P[j] - m);
        l = l + P[j];
    }
    for (int j = 0; j < T; ++j) P[j] = P[j] / l;
}

inline void tnt_host_row_bwd(const float* v, const float* g, int64_t rs, int64_t gs, int T, int dh, int i, const float* P, float* dS) {
    float delta = 0.f;
    for (int j = 0; j < T; ++j) {
        float acc = 0.f;
        for (int d = 0; d < dh; ++d) acc = fmaf(g[i * gs + d], v[j * rs + d], acc);
        dS[j] = acc;
        delta = fmaf(P[j], acc, delta);
    }
    for (int j = 0; j < T; ++j) dS[j] = P[j] * (dS[j] - delta);
}

inline int tnt_attention(const TntAttn& p, hipStream_t) {
    if (const char* why = tnt_attn_refusal(p, false)) return tnt_host_refuse("tnt_attention", why);
    const int T = p.T, H = p.H, dh = p.dh, C = H * dh;
    float P[TNT_MAX_T];
    for (int64_t s = 0; s < p.S; ++s)
        for (int h = 0; h < H; ++h) {
            const float *q = p.qkv + s * T * 3 * C + h * dh, *k = q + C, *v = q + 2 * C;
            for (int i = 0; i < T; ++i) {
                tnt_host_row(q, k, 3 * C, T, dh, p.scale, i, P);
                for (int d = 0; d < dh; ++d) {
                    float acc = 0.f;
                    for (int j = 0; j < T; ++j) acc = fmaf(P[j], v[(int64_t)j * 3 * C + d], acc);
                    p.out[(s * T + i) * C + h * dh + d] = acc;
                }
            }
        }
    return 0;
}

inline int tnt_attention_bwd(const TntAttn& p, hipStream_t) {
    if (const char* why = tnt_attn_refusal(p, true)) return tnt_host_refuse("tnt_attention_bwd", why);
    const int T = p.T, H = p.H, dh = p.dh, C = H * dh;
    float P[TNT_MAX_T][TNT_MAX_T], dS[TNT_MAX_T][TNT_MAX_T];
    for (int64_t s = 0; s < p.S; ++s)
        for (int h = 0; h < H; ++h) {
            const float *q = p.qkv + s * T * 3 * C + h * dh, *k = q + C, *v = q + 2 * C, *g = p.dout + s * T * C + h * dh;
            float *dq = p.dqkv + s * T * 3 * C + h * dh, *dk = dq + C, *dv = dq + 2 * C;
            for (int i = 0; i < T; ++i) {
                tnt_host_row(q, k, 3 * C, T, dh, p.scale, i, P[i]);
                tnt_host_row_bwd(v, g, 3 * C, C, T, dh, i, P[i], dS[i]);
                for (int d = 0; d < dh; ++d) {
                    float acc = 0.f;
                    for (int j = 0; j < T; ++j) acc = fmaf(dS[i][j], k[(int64_t)j * 3 * C + d], acc);
                    dq[(int64_t)i * 3 * C + d] = acc * p.scale;
                }
            }
            for (int j = 0; j < T; ++j)
                for (int d = 0; d < dh; ++d) {
                    float ak = 0.f, av = 0.f;
                    for (int i = 0; i < T; ++i) {
                        ak = fmaf(dS[i][j], q[(int64_t)i * 3 * C + d], ak);
                        av = fmaf(P[i][j], g[(int64_t)i * C + d], av);
                    }
                    dk[(int64_t)j * 3 * C + d] = ak * p.scale;
                    dv[(int64_t)j * 3 * C + d] = av;
                }
        }
    return 0;
}

inline int tnt_pixel_gather(const TntPixels& p, hipStream_t) {
    if (const char* why = tnt_pixels_refusal(p)) return tnt_host_refuse("tnt_pixel_gather", why);
    const int side = p.side, g = side / 16, K = p.Cin * 49, Kp = tnt_pixel_cols(p.Cin);
    for (int64_t r = 0; r < (int64_t)p.F * g * g * 16; ++r) {
        const int pix = (int)(r % 16), px = (int)((r / 16) % g), py = (int)((r / 16 / g) % g);
        const int64_t f = r / 16 / g / g;
        const int oy = 4 * py + pix / 4, ox = 4 * px + pix % 4;
        for (int col = 0; col < Kp; ++col) {
            const int c = col / 49, ky = (col % 49) / 7, kx = col % 7, y = 4 * oy + ky - 3, x = 4 * ox + kx - 3;
            const bool in = col < K && y >= 0 && y < side && x >= 0 && x < side;
            p.dst[r * Kp + col] = in ? p.src[((f * p.Cin + c) * side + y) * side + x] : 0.f;
        }
    }
    return 0;
}

inline int tnt_pixel_scatter(const TntPixels& p, hipStream_t) {
    if (const char* why = tnt_pixels_refusal(p)) return tnt_host_refuse("tnt_pixel_scatter", why);
    const int side = p.side, g = side / 16, Kp = tnt_pixel_cols(p.Cin), no = side / 4;
    for (int64_t e = 0; e < (int64_t)p.F * p.Cin * side * side; ++e) {
        const int x = (int)(e % side), y = (int)((e / side) % side), c = (int)((e / side / side) % p.Cin);
        const int64_t f = e / side / side / p.Cin;
        float acc = 0.f;
        for (int oy = y / 4; oy <= (y + 3) / 4 && oy < no; ++oy)          // 0 <= ky = y + 3 - 4 oy <= 6
            for (int ox = x / 4; ox <= (x + 3) / 4 && ox < no; ++ox) {
                const int ky = y + 3 - 4 * oy, kx = x + 3 - 4 * ox;
                const int64_t row = ((f * g + oy / 4) * g + ox / 4) * 16 + (oy % 4) * 4 + ox % 4;
                acc = acc + p.src[row * Kp + c * 49 + ky * 7 + kx];
            }
        p.dst[e] = p.accumulate ? p.dst[e] + acc : acc;
    }
    return 0;
}

inline int tnt_row_add(float* x, const float* table, int64_t rows, int C, int64_t period, hipStream_t) {
    if (const char* why = tnt_row_add_refusal(x, table, rows, C, period)) return tnt_host_refuse("tnt_row_add", why);
    for (int64_t r = 0; r < rows; ++r)
        for (int c = 0; c < C; ++c) x[r * C + c] = x[r * C + c] + table[(r % period) * C + c];
    return 0;
}
