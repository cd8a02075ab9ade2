// The CaiT launches (i2v_cait_kernels.h) as plain scalar C++ on the backend's memory: what the planner runs where the library has no
// i2v_cait.hip (no -DI2V_HAVE_CAIT: the host simulation's one-file build, whose backend memory is host memory).  The same definitions and
// the same refusals as the kernels; the ORDER of the sums is the simplest one (one fma chain in increasing index, a plain running sum over
// a row) and is NOT the device's, so these are held to the float64 bound, not to the device's bits.  Only expf is the host's own.
#pragma once
#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "i2v_cait_kernels.h"
#include "i2v_kernels.h"

inline int cait_host_refuse(const char* who, const char* why) {
    char buf[256];
    snprintf(buf, sizeof buf, "%s: hipErrorInvalidValue: %s", who, why);
    return i2v_api_fail(buf);
}

// out[g] = sum_h w[g][h] x[h] (+ bias[g]); tr: out[h] = sum_g w[g][h] x[g]
inline void cait_host_mix(const float* x, int H, const float* w, const float* bias, bool tr, float* out) {
    for (int g = 0; g < H; ++g) {
        float acc = 0.f;
        for (int h = 0; h < H; ++h) acc = fmaf(tr ? w[h * H + g] : w[g * H + h], x[h], acc);
        out[g] = bias ? acc + bias[g] : acc;
    }
}

inline int cait_attention(const CaitAttn& p, hipStream_t) {
    if (const char* why = cait_attn_refusal(p, false)) return cait_host_refuse("cait_attention", why);
    const int T = p.T, H = p.H, dh = p.dh, C = H * dh, ld = cait_probs_ld(T);
    std::vector<float> S((size_t)H * T), x(H), y(H);
    for (int f = 0; f < p.F; ++f) {
        const float* qkv = p.qkv + (int64_t)f * T * 3 * C;
        for (int row = 0; row < T; ++row) {
            for (int h = 0; h < H; ++h)
                for (int key = 0; key < T; ++key) {
                    float acc = 0.f;
                    for (int k = 0; k < dh; ++k)
                        acc = fmaf(p.scale * qkv[(int64_t)row * 3 * C + h * dh + k], qkv[(int64_t)key * 3 * C + C + h * dh + k], acc);
                    S[(size_t)h * T + key] = acc;
                }
            for (int key = 0; key < T; ++key) {
                for (int h = 0; h < H; ++h) x[h] = S[(size_t)h * T + key];
                cait_host_mix(x.data(), H, p.wl, p.bl, false, y.data());
                for (int h = 0; h < H; ++h) S[(size_t)h * T + key] = y[h];
            }
            for (int h = 0; h < H; ++h) {
                float* s = &S[(size_t)h * T];
                float m = -INFINITY, sum = 0.f;
                for (int key = 0; key < T; ++key) m = fmaxf(m, s[key]);
                for (int key = 0; key < T; ++key) { s[key] = expf(s[key] - m); sum = sum + s[key]; }
                const float inv = 1.f / sum;
                float* pr = p.P + (((int64_t)f * H + h) * T + row) * ld;
                for (int key = 0; key < T; ++key) pr[key] = s[key] = s[key] * inv;
            }
            for (int key = 0; key < T; ++key) {
                for (int h = 0; h < H; ++h) x[h] = S[(size_t)h * T + key];
                cait_host_mix(x.data(), H, p.ww, p.bw, false, y.data());
                for (int h = 0; h < H; ++h) S[(size_t)h * T + key] = y[h];
            }
            for (int h = 0; h < H; ++h)
                for (int d = 0; d < dh; ++d) {
                    float acc = 0.f;
                    for (int key = 0; key < T; ++key) acc = fmaf(S[(size_t)h * T + key], qkv[(int64_t)key * 3 * C + 2 * C + h * dh + d], acc);
                    p.out[((int64_t)f * T + row) * C + h * dh + d] = acc;
                }
        }
    }
    return 0;
}

inline int cait_attention_bwd(const CaitAttn& p, hipStream_t) {
    if (const char* why = cait_attn_refusal(p, true)) return cait_host_refuse("cait_attention_bwd", why);
    const int T = p.T, H = p.H, dh = p.dh, C = H * dh, ld = cait_probs_ld(T);
    const int64_t hs = (int64_t)T * ld;
    std::vector<float> S((size_t)H * T), x(H), y(H);
    for (int f = 0; f < p.F; ++f) {
        const float* qkv = p.qkv + (int64_t)f * T * 3 * C;
        const float* dout = p.dout + (int64_t)f * T * C;
        float* dqkv = p.dqkv + (int64_t)f * T * 3 * C;
        const int64_t fo = (int64_t)f * H * hs;
        for (int row = 0; row < T; ++row) {                         // the row-tile launch: dS, Pm, dq
            for (int g = 0; g < H; ++g)
                for (int key = 0; key < T; ++key) {
                    float acc = 0.f;
                    for (int k = 0; k < dh; ++k) acc = fmaf(dout[(int64_t)row * C + g * dh + k], qkv[(int64_t)key * 3 * C + 2 * C + g * dh + k], acc);
                    S[(size_t)g * T + key] = acc;
                }
            for (int key = 0; key < T; ++key) {
                const int64_t o = fo + (int64_t)row * ld + key;
                for (int h = 0; h < H; ++h) x[h] = p.P[o + h * hs];
                cait_host_mix(x.data(), H, p.ww, p.bw, false, y.data());
                for (int h = 0; h < H; ++h) p.Pm[o + h * hs] = y[h];
                for (int h = 0; h < H; ++h) x[h] = S[(size_t)h * T + key];
                cait_host_mix(x.data(), H, p.ww, nullptr, true, y.data());
                for (int h = 0; h < H; ++h) S[(size_t)h * T + key] = y[h];
            }
            for (int h = 0; h < H; ++h) {
                float* s = &S[(size_t)h * T];
                const float* pr = p.P + fo + h * hs + (int64_t)row * ld;
                float sum = 0.f;
                for (int key = 0; key < T; ++key) sum = sum + s[key] * pr[key];
                for (int key = 0; key < T; ++key) s[key] = pr[key] * (s[key] - sum);
            }
            for (int key = 0; key < T; ++key) {
                const int64_t o = fo + (int64_t)row * ld + key;
                for (int h = 0; h < H; ++h) x[h] = S[(size_t)h * T + key];
                cait_host_mix(x.data(), H, p.wl, nullptr, true, y.data());
                for (int h = 0; h < H; ++h) p.dS[o + h * hs] = S[(size_t)h * T + key] = y[h];
            }
            for (int h = 0; h < H; ++h)
                for (int d = 0; d < dh; ++d) {
                    float acc = 0.f;
                    for (int key = 0; key < T; ++key) acc = fmaf(S[(size_t)h * T + key], qkv[(int64_t)key * 3 * C + C + h * dh + d], acc);
                    dqkv[(int64_t)row * 3 * C + h * dh + d] = p.scale * acc;
                }
        }
        for (int key = 0; key < T; ++key)                           // the key-tile launch: dk, dv
            for (int h = 0; h < H; ++h)
                for (int d = 0; d < dh; ++d) {
                    float ak = 0.f, av = 0.f;
                    for (int row = 0; row < T; ++row) {
                        const int64_t o = fo + h * hs + (int64_t)row * ld + key;
                        ak = fmaf(p.dS[o], qkv[(int64_t)row * 3 * C + h * dh + d], ak);
                        av = fmaf(p.Pm[o], dout[(int64_t)row * C + h * dh + d], av);
                    }
                    dqkv[(int64_t)key * 3 * C + C + h * dh + d] = p.scale * ak;
                    dqkv[(int64_t)key * 3 * C + 2 * C + h * dh + d] = av;
                }
    }
    return 0;
}

inline int cait_add_pos(float* x, const float* pos, int F, int T, int C, hipStream_t) {
    if (!x || !pos || F <= 0 || T <= 0 || C <= 0 || C % 4 != 0 || (((uintptr_t)x | (uintptr_t)pos) & 15))
        return cait_host_refuse("cait_add_pos", "C % 4 == 0 and 16-byte alignment needed");
    for (int f = 0; f < F; ++f)
        for (int64_t i = 0; i < (int64_t)T * C; ++i) x[(int64_t)f * T * C + i] = x[(int64_t)f * T * C + i] + pos[i];
    return 0;
}
