// The BEiT launches (i2v_beit_kernels.h) as plain scalar C++ on the backend's memory: what the planner runs where the library has no
// i2v_beit.hip (no -DI2V_HAVE_BEIT: the host simulation's one-file build, whose backend memory is host memory).  The same definitions and the same refusals as the kernels;
// the ORDER of the sums is the simplest one (one fma chain in increasing index, a plain running sum over a row) and is NOT the device's,
// so these are held to the float64 bound, not to the device's bits.  Only expf is the host's own.
#pragma once
#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "i2v_kernels.h"
#include "i2v_beit_kernels.h"

inline int beit_host_refuse(const char* who, const char* why) {
    char buf[256];
    snprintf(buf, sizeof buf, "%s: hipErrorInvalidValue: %s", who, why);
    return i2v_api_fail(buf);
}

// P (T) of query row qr against the T keys at k (row stride sk), with the query's row of the bias (or null)
inline void beit_host_probs(const float* qr, const float* k, int64_t sk, const float* brow, int T, int dh, float scale, float* P) {
    float m = -INFINITY, sum = 0.f;
    for (int j = 0; j < T; ++j) {
        float acc = 0.f;
        for (int d = 0; d < dh; ++d) acc = fmaf(qr[d], k[j * sk + d], acc);
        P[j] = acc * scale;
        if (brow) P[j] = P[j] + brow[j];
        m = fmaxf(m, P[j]);
    }
    for (int j = 0; j < T; ++j) { P[j] = expf(P[j] - m); sum = sum + P[j]; }
    for (int j = 0; j < T; ++j) P[j] = P[j] / sum;
}

inline int beit_attention(const BeitAttn& p, hipStream_t) {
    if (const char* why = beit_attn_refusal(p, false)) return beit_host_refuse("beit_attention", why);
    const int T = p.T, H = p.H, dh = p.dh, C = H * dh;
    std::vector<float> P((size_t)T);
    for (int64_t f = 0; f < p.F; ++f)
        for (int h = 0; h < H; ++h) {
            const float *q = p.qkv + f * T * 3 * C + h * dh, *k = q + C, *v = q + 2 * C;
            for (int i = 0; i < T; ++i) {
                beit_host_probs(q + (int64_t)i * 3 * C, k, 3 * C, p.bias ? p.bias + ((int64_t)h * T + i) * T : nullptr, T, dh, p.scale, P.data());
                for (int d = 0; d < dh; ++d) {
                    float acc = 0.f;
                    for (int j = 0; j < T; ++j) acc = fmaf(P[j], v[(int64_t)j * 3 * C + d], acc);
                    p.out[(f * T + i) * C + h * dh + d] = acc;
                }
            }
        }
    return 0;
}

inline int beit_attention_bwd(const BeitAttn& p, hipStream_t) {
    if (const char* why = beit_attn_refusal(p, true)) return beit_host_refuse("beit_attention_bwd", why);
    const int T = p.T, H = p.H, dh = p.dh, C = H * dh;
    std::vector<float> P((size_t)T), dS((size_t)T);
    for (int64_t f = 0; f < p.F; ++f)
        for (int h = 0; h < H; ++h) {
            const float *q = p.qkv + f * T * 3 * C + h * dh, *k = q + C, *v = q + 2 * C;
            float *dq = p.dqkv + f * T * 3 * C + h * dh, *dk = dq + C, *dv = dq + 2 * C;
            for (int j = 0; j < T; ++j)
                for (int d = 0; d < dh; ++d) dk[(int64_t)j * 3 * C + d] = dv[(int64_t)j * 3 * C + d] = 0.f;
            for (int i = 0; i < T; ++i) {                                   // the queries in increasing order: one owner, one order
                const float *qr = q + (int64_t)i * 3 * C, *gr = p.dout + (f * T + i) * C + h * dh;
                beit_host_probs(qr, k, 3 * C, p.bias ? p.bias + ((int64_t)h * T + i) * T : nullptr, T, dh, p.scale, P.data());
                float delta = 0.f;
                for (int j = 0; j < T; ++j) {
                    float acc = 0.f;
                    for (int d = 0; d < dh; ++d) acc = fmaf(gr[d], v[(int64_t)j * 3 * C + d], acc);
                    dS[j] = acc;                                           // dP for now
                    delta = delta + acc * P[j];
                }
                for (int j = 0; j < T; ++j) dS[j] = p.scale * (P[j] * (dS[j] - delta));
                for (int d = 0; d < dh; ++d) {
                    float acc = 0.f;
                    for (int j = 0; j < T; ++j) acc = fmaf(dS[j], k[(int64_t)j * 3 * C + d], acc);
                    dq[(int64_t)i * 3 * C + d] = acc;
                }
                for (int j = 0; j < T; ++j)
                    for (int d = 0; d < dh; ++d) {
                        dk[(int64_t)j * 3 * C + d] = fmaf(dS[j], qr[d], dk[(int64_t)j * 3 * C + d]);
                        dv[(int64_t)j * 3 * C + d] = fmaf(P[j], gr[d], dv[(int64_t)j * 3 * C + d]);
                    }
            }
        }
    return 0;
}

inline int beit_bias_add(float* S, const float* bias, int F, int64_t per_frame, hipStream_t) {
    if (const char* why = beit_bias_add_refusal(S, bias, F, per_frame)) return beit_host_refuse("beit_bias_add", why);
    for (int64_t f = 0; f < F; ++f)
        for (int64_t e = 0; e < per_frame; ++e) S[f * per_frame + e] = S[f * per_frame + e] + bias[e];
    return 0;
}

