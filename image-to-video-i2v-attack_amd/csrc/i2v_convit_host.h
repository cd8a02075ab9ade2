// The ConViT launches (i2v_convit_kernels.h) as plain scalar C++ on the backend's memory: what the planner runs where the library has no
// i2v_convit.hip (no -DI2V_HAVE_CONVIT: the host simulation's one-file build, whose backend memory is host memory).  The same definitions
// and the same refusals as the kernels; the ORDER of the sums is the simplest one (one fma chain in increasing index, a plain running sum
// over a row) and is NOT the device's, so these are held to the float64 bound, not to the device's bits.  Only expf is the host's own.
#pragma once
#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "i2v_convit_kernels.h"
#include "i2v_kernels.h"

inline int convit_host_refuse(const char* who, const char* why) {
    char buf[256];
    snprintf(buf, sizeof buf, "%s: hipErrorInvalidValue: %s", who, why);
    return i2v_api_fail(buf);
}

inline int convit_attention(const ConvitAttn& p, hipStream_t) {
    if (const char* why = convit_attn_refusal(p, false)) return convit_host_refuse("convit_attention", why);
    const int T = p.T, H = p.H, dh = p.dh, C = H * dh, ld = convit_probs_ld(T);
    std::vector<float> S((size_t)T);
    for (int f = 0; f < p.F; ++f) {
        const float* qkv = p.qkv + (int64_t)f * T * 3 * C;
        for (int h = 0; h < H; ++h)
            for (int row = 0; row < T; ++row) {
                float m = -INFINITY, sum = 0.f;
                for (int key = 0; key < T; ++key) {
                    float acc = 0.f;
                    for (int k = 0; k < dh; ++k)
                        acc = fmaf(p.scale * qkv[(int64_t)row * 3 * C + h * dh + k], qkv[(int64_t)key * 3 * C + C + h * dh + k], acc);
                    S[key] = acc;
                    m = fmaxf(m, acc);
                }
                for (int key = 0; key < T; ++key) { S[key] = expf(S[key] - m); sum = sum + S[key]; }
                const float inv = 1.f / sum;
                float* pr = p.P + (((int64_t)f * H + h) * T + row) * ld;
                const float* tb = p.table ? p.table + ((int64_t)h * T + row) * ld : nullptr;
                for (int key = 0; key < T; ++key) {
                    const float v = S[key] * inv;
                    pr[key] = v;
                    S[key] = tb ? fmaf(p.c[h], v, tb[key]) : v;
                }
                for (int d = 0; d < dh; ++d) {
                    float acc = 0.f;
                    for (int key = 0; key < T; ++key) acc = fmaf(S[key], qkv[(int64_t)key * 3 * C + 2 * C + h * dh + d], acc);
                    p.out[((int64_t)f * T + row) * C + h * dh + d] = acc;
                }
            }
    }
    return 0;
}

inline int convit_attention_bwd(const ConvitAttn& p, hipStream_t) {
    if (const char* why = convit_attn_refusal(p, true)) return convit_host_refuse("convit_attention_bwd", why);
    const int T = p.T, H = p.H, dh = p.dh, C = H * dh, ld = convit_probs_ld(T);
    std::vector<float> S((size_t)T);
    for (int f = 0; f < p.F; ++f) {
        const float* qkv = p.qkv + (int64_t)f * T * 3 * C;
        const float* dout = p.dout + (int64_t)f * T * C;
        float* dqkv = p.dqkv + (int64_t)f * T * 3 * C;
        for (int h = 0; h < H; ++h) {
            const int64_t ho = ((int64_t)f * H + h) * T * ld;
            const float cv = p.c ? p.c[h] : 1.f;
            for (int row = 0; row < T; ++row) {                         // the row-tile launch: dS, dq
                const float* pr = p.P + ho + (int64_t)row * ld;
                float sum = 0.f;
                for (int key = 0; key < T; ++key) {
                    float acc = 0.f;
                    for (int k = 0; k < dh; ++k) acc = fmaf(dout[(int64_t)row * C + h * dh + k], qkv[(int64_t)key * 3 * C + 2 * C + h * dh + k], acc);
                    S[key] = cv * acc;
                    sum = sum + S[key] * pr[key];
                }
                for (int key = 0; key < T; ++key) p.dS[ho + (int64_t)row * ld + key] = S[key] = pr[key] * (S[key] - sum);
                for (int d = 0; d < dh; ++d) {
                    float acc = 0.f;
                    for (int key = 0; key < T; ++key) acc = fmaf(S[key], qkv[(int64_t)key * 3 * C + C + h * dh + d], acc);
                    dqkv[(int64_t)row * 3 * C + h * dh + d] = p.scale * acc;
                }
            }
            for (int key = 0; key < T; ++key)                           // the key-tile launch: dk, dv
                for (int d = 0; d < dh; ++d) {
                    float ak = 0.f, av = 0.f;
                    for (int row = 0; row < T; ++row) {
                        const int64_t o = ho + (int64_t)row * ld + key;
                        const float pv = p.table ? fmaf(cv, p.P[o], p.table[((int64_t)h * T + row) * ld + key]) : p.P[o];
                        ak = fmaf(p.dS[o], qkv[(int64_t)row * 3 * C + h * dh + d], ak);
                        av = fmaf(pv, dout[(int64_t)row * C + h * dh + d], av);
                    }
                    dqkv[(int64_t)key * 3 * C + C + h * dh + d] = p.scale * ak;
                    dqkv[(int64_t)key * 3 * C + 2 * C + h * dh + d] = av;
                }
        }
    }
    return 0;
}

// what the device's join launches refuse (i2v_convit.hip, join_ok): `b` may be null
inline int convit_host_join_ok(const void* a, const void* b, const void* c, int F, int T, int C) {
    return a && c && F > 0 && T > 0 && C > 0 && C % 4 == 0 && (int64_t)F * (T + 1) * C < (1ll << 31) &&
           !(((uintptr_t)a | (uintptr_t)b | (uintptr_t)c) & 15);
}

inline int convit_join_cls(const float* x, const float* cls, float* out, int F, int T, int C, hipStream_t) {
    if (!cls || !convit_host_join_ok(x, cls, out, F, T, C))
        return convit_host_refuse("convit_join_cls", "C % 4 == 0, fewer than 2^31 elements and 16-byte alignment needed");
    for (int f = 0; f < F; ++f) {
        float* o = out + (int64_t)f * (T + 1) * C;
        for (int c = 0; c < C; ++c) o[c] = cls[c];
        for (int64_t i = 0; i < (int64_t)T * C; ++i) o[C + i] = x[(int64_t)f * T * C + i];
    }
    return 0;
}

inline int convit_join_cls_bwd(const float* dout, const float* add, float* dx, int F, int T, int C, hipStream_t) {
    if (!convit_host_join_ok(dout, add, dx, F, T, C))
        return convit_host_refuse("convit_join_cls_bwd", "C % 4 == 0, fewer than 2^31 elements and 16-byte alignment needed");
    for (int f = 0; f < F; ++f)
        for (int64_t i = 0; i < (int64_t)T * C; ++i) {
            const float v = dout[(int64_t)f * (T + 1) * C + C + i];
            dx[(int64_t)f * T * C + i] = add ? v + add[(int64_t)f * T * C + i] : v;
        }
    return 0;
}
