// The Twins launches (i2v_twins_kernels.h) as plain scalar C++ on the backend's memory: what the planner runs where the library has no
// i2v_twins.hip (no -DI2V_HAVE_TWINS: the host simulation's one-file build, whose backend memory is host memory), and window attention
// at shift 0 without a table, which the host simulation has in no other form.  The same definitions and the same refusals as the
// kernels; the ORDER of the sums is the simplest one (one fma chain in increasing index, a plain running sum over a row) and is NOT
// the device's, so these are held to the float64 bound, not to the device's bits.  Only expf is the host's own.
#pragma once
#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "i2v_kernels.h"
#include "i2v_twins_kernels.h"

inline int twins_host_refuse(const char* who, const char* why) {
    char buf[256];
    snprintf(buf, sizeof buf, "%s: hipErrorInvalidValue: %s", who, why);
    return i2v_api_fail(buf);
}

// P (Tk) of query row qr against the Tk keys at k (row stride sk)
inline void twins_host_probs(const float* qr, const float* k, int64_t sk, int Tk, int dh, float scale, float* P) {
    float m = -INFINITY, sum = 0.f;
    for (int j = 0; j < Tk; ++j) {
        float acc = 0.f;
        for (int d = 0; d < dh; ++d) acc = fmaf(qr[d], k[j * sk + d], acc);
        P[j] = acc * scale;
        m = fmaxf(m, P[j]);
    }
    for (int j = 0; j < Tk; ++j) { P[j] = expf(P[j] - m); sum = sum + P[j]; }
    for (int j = 0; j < Tk; ++j) P[j] = P[j] / sum;
}

inline int twins_attention(const TwinsAttn& p, hipStream_t) {
    if (const char* why = twins_attn_refusal(p, false)) return twins_host_refuse("twins_attention", why);
    const int Tq = p.Tq, Tk = p.Tk, H = p.H, dh = p.dh, C = H * dh;
    std::vector<float> P((size_t)Tk);
    for (int64_t f = 0; f < p.F; ++f)
        for (int h = 0; h < H; ++h) {
            const float *k = p.kv + f * Tk * 2 * C + h * dh, *v = k + C;
            for (int i = 0; i < Tq; ++i) {
                const int64_t o = (f * Tq + i) * C + h * dh;
                twins_host_probs(p.q + o, k, 2 * C, Tk, dh, p.scale, P.data());
                for (int d = 0; d < dh; ++d) {
                    float acc = 0.f;
                    for (int j = 0; j < Tk; ++j) acc = fmaf(P[j], v[(int64_t)j * 2 * C + d], acc);
                    p.out[o + d] = acc;
                }
            }
        }
    return 0;
}

inline int twins_attention_bwd(const TwinsAttn& p, hipStream_t) {
    if (const char* why = twins_attn_refusal(p, true)) return twins_host_refuse("twins_attention_bwd", why);
    const int Tq = p.Tq, Tk = p.Tk, H = p.H, dh = p.dh, C = H * dh;
    std::vector<float> P((size_t)Tk), dS((size_t)Tk);
    for (int64_t f = 0; f < p.F; ++f)
        for (int h = 0; h < H; ++h) {
            const float *k = p.kv + f * Tk * 2 * C + h * dh, *v = k + C;
            float *dk = p.dkv + f * Tk * 2 * C + h * dh, *dv = dk + C;
            for (int j = 0; j < Tk; ++j)
                for (int d = 0; d < dh; ++d) dk[(int64_t)j * 2 * C + d] = dv[(int64_t)j * 2 * C + d] = 0.f;
            for (int i = 0; i < Tq; ++i) {                                  // the queries in increasing order: one owner, one order
                const int64_t o = (f * Tq + i) * C + h * dh;
                const float *qr = p.q + o, *gr = p.dout + o;
                twins_host_probs(qr, k, 2 * C, Tk, dh, p.scale, P.data());
                float delta = 0.f;
                for (int j = 0; j < Tk; ++j) {
                    float acc = 0.f;
                    for (int d = 0; d < dh; ++d) acc = fmaf(gr[d], v[(int64_t)j * 2 * C + d], acc);
                    dS[j] = acc;                                           // dP for now
                    delta = delta + acc * P[j];
                }
                for (int j = 0; j < Tk; ++j) dS[j] = p.scale * (P[j] * (dS[j] - delta));
                for (int d = 0; d < dh; ++d) {
                    float acc = 0.f;
                    for (int j = 0; j < Tk; ++j) acc = fmaf(dS[j], k[(int64_t)j * 2 * C + d], acc);
                    p.dq[o + d] = acc;
                }
                for (int j = 0; j < Tk; ++j)
                    for (int d = 0; d < dh; ++d) {
                        dk[(int64_t)j * 2 * C + d] = fmaf(dS[j], qr[d], dk[(int64_t)j * 2 * C + d]);
                        dv[(int64_t)j * 2 * C + d] = fmaf(P[j], gr[d], dv[(int64_t)j * 2 * C + d]);
                    }
            }
        }
    return 0;
}

inline int twins_host_block(const float* in, float* out, int F, int H, int W, int C, int sr, int scatter, int accumulate) {
    const int Wo = W / sr, Ho = H / sr;
    for (int64_t f = 0; f < F; ++f)
        for (int y = 0; y < H; ++y)
            for (int x = 0; x < W; ++x)
                for (int c = 0; c < C; ++c) {
                    const int64_t full = ((f * H + y) * W + x) * C + c;
                    const int64_t row = (f * Ho + y / sr) * Wo + x / sr;
                    const int64_t cell = (row * sr * sr + (y % sr) * sr + x % sr) * C + c;
                    if (!scatter) out[cell] = in[full];
                    else out[full] = accumulate ? out[full] + in[cell] : in[cell];
                }
    return 0;
}

inline int twins_block_gather(const float* x, float* rows, int F, int H, int W, int C, int sr, hipStream_t) {
    if (const char* why = twins_block_refusal(x, rows, F, H, W, C, sr)) return twins_host_refuse("twins_block_gather", why);
    return twins_host_block(x, rows, F, H, W, C, sr, 0, 0);
}

inline int twins_block_scatter(const float* drows, float* dx, int F, int H, int W, int C, int sr, int accumulate, hipStream_t) {
    if (const char* why = twins_block_refusal(drows, dx, F, H, W, C, sr)) return twins_host_refuse("twins_block_scatter", why);
    return twins_host_block(drows, dx, F, H, W, C, sr, 1, accumulate);
}

// the (frame, window, head) problems of window attention at shift 0: the window's tokens in row-major order are its queries and keys
template <class Fn>
inline void twins_host_windows(int F, int H, int W, int ws, int heads, Fn fn) {
    std::vector<int64_t> tok((size_t)ws * ws);
    for (int64_t f = 0; f < F; ++f)
        for (int wy = 0; wy < H / ws; ++wy)
            for (int wx = 0; wx < W / ws; ++wx) {
                for (int i = 0; i < ws * ws; ++i) tok[i] = (f * H + wy * ws + i / ws) * W + wx * ws + i % ws;
                for (int h = 0; h < heads; ++h) fn(tok, h);
            }
}

inline int twins_window_attention(const float* qkv, int F, int H, int W, int ws, int heads, int dh, const float*, float* out, hipStream_t) {
    if (const char* why = twins_window_refusal(qkv, out, out, F, H, W, ws, heads, dh)) return twins_host_refuse("twins_window_attention", why);
    const int N = ws * ws, C = heads * dh;
    const float scale = 1.f / sqrtf((float)dh);
    std::vector<float> P((size_t)N), K((size_t)N * dh);
    twins_host_windows(F, H, W, ws, heads, [&](const std::vector<int64_t>& tok, int h) {
        for (int j = 0; j < N; ++j)
            for (int d = 0; d < dh; ++d) K[j * dh + d] = qkv[tok[j] * 3 * C + C + h * dh + d];
        for (int i = 0; i < N; ++i) {
            twins_host_probs(qkv + tok[i] * 3 * C + h * dh, K.data(), dh, N, dh, scale, P.data());
            for (int d = 0; d < dh; ++d) {
                float acc = 0.f;
                for (int j = 0; j < N; ++j) acc = fmaf(P[j], qkv[tok[j] * 3 * C + 2 * C + h * dh + d], acc);
                out[tok[i] * C + h * dh + d] = acc;
            }
        }
    });
    return 0;
}

inline int twins_window_attention_bwd(const float* qkv, const float* dout, int F, int H, int W, int ws, int heads, int dh, const float*,
                                      float* dqkv, hipStream_t) {
    if (const char* why = twins_window_refusal(qkv, dout, dqkv, F, H, W, ws, heads, dh))
        return twins_host_refuse("twins_window_attention_bwd", why);
    const int N = ws * ws, C = heads * dh;
    const float scale = 1.f / sqrtf((float)dh);
    std::vector<float> P((size_t)N), dS((size_t)N), K((size_t)N * dh);
    twins_host_windows(F, H, W, ws, heads, [&](const std::vector<int64_t>& tok, int h) {
        for (int j = 0; j < N; ++j)
            for (int d = 0; d < dh; ++d) {
                K[j * dh + d] = qkv[tok[j] * 3 * C + C + h * dh + d];
                dqkv[tok[j] * 3 * C + C + h * dh + d] = dqkv[tok[j] * 3 * C + 2 * C + h * dh + d] = 0.f;
            }
        for (int i = 0; i < N; ++i) {
            const float *qr = qkv + tok[i] * 3 * C + h * dh, *gr = dout + tok[i] * C + h * dh;
            twins_host_probs(qr, K.data(), dh, N, dh, scale, P.data());
            float delta = 0.f;
            for (int j = 0; j < N; ++j) {
                float acc = 0.f;
                for (int d = 0; d < dh; ++d) acc = fmaf(gr[d], qkv[tok[j] * 3 * C + 2 * C + h * dh + d], acc);
                dS[j] = acc;
                delta = delta + acc * P[j];
            }
            for (int j = 0; j < N; ++j) dS[j] = scale * (P[j] * (dS[j] - delta));
            for (int d = 0; d < dh; ++d) {
                float acc = 0.f;
                for (int j = 0; j < N; ++j) acc = fmaf(dS[j], K[j * dh + d], acc);
                dqkv[tok[i] * 3 * C + h * dh + d] = acc;
            }
            for (int j = 0; j < N; ++j)
                for (int d = 0; d < dh; ++d) {
                    float* dk = dqkv + tok[j] * 3 * C + C + h * dh + d;
                    *dk = fmaf(dS[j], qr[d], *dk);
                    dk[C] = fmaf(P[j], gr[d], dk[C]);
                }
        }
    });
    return 0;
}

