// The PiT launches (i2v_pit_kernels.h) as plain scalar C++ on the backend's memory: what the planner runs where the library has no
// i2v_pit.hip (no -DI2V_HAVE_PIT: the host simulation's one-file build, whose backend memory is host memory).  The same definitions and
// the same refusals as the kernels; the attention is NOT streamed here (one pass over a whole row) and the ORDER of its sums is the
// simplest one, not the device's, so it is held to the float64 bound, not to the device's bits.  The pool and patch launches add their
// taps in the device's order.  Only expf and logf are the host's own.
#pragma once
#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include <algorithm>
#include <vector>

#include "i2v_kernels.h"
#include "i2v_pit_kernels.h"

inline int pit_host_refuse(const char* who, const char* why) {
    char buf[256];
    snprintf(buf, sizeof buf, "%s: hipErrorInvalidValue: %s", who, why);
    return i2v_api_fail(buf);
}

// S (T) = scale q k^T of query row qr against the T keys at k (row stride sk)
inline void pit_host_scores(const float* qr, const float* k, int64_t sk, int T, int dh, float scale, float* S) {
    for (int j = 0; j < T; ++j) {
        float acc = 0.f;
        for (int d = 0; d < dh; ++d) acc = fmaf(qr[d], k[j * sk + d], acc);
        S[j] = acc * scale;
    }
}

inline int pit_attention(const PitAttn& p, hipStream_t) {
    if (const char* why = pit_attn_refusal(p, false)) return pit_host_refuse("pit_attention", why);
    const int T = p.T, H = p.H, dh = p.dh, C = H * dh;
    std::vector<float> P((size_t)T);
    for (int64_t f = 0; f < p.F; ++f)
        for (int h = 0; h < H; ++h) {
            const float *q = p.qkv + f * T * 3 * C + h * dh, *k = q + C, *v = q + 2 * C;
            for (int i = 0; i < T; ++i) {
                pit_host_scores(q + (int64_t)i * 3 * C, k, 3 * C, T, dh, p.scale, P.data());
                float m = -INFINITY, sum = 0.f;
                for (int j = 0; j < T; ++j) m = fmaxf(m, P[j]);
                for (int j = 0; j < T; ++j) { P[j] = expf(P[j] - m); sum = sum + P[j]; }
                for (int d = 0; d < dh; ++d) {
                    float acc = 0.f;
                    for (int j = 0; j < T; ++j) acc = fmaf(P[j], v[(int64_t)j * 3 * C + d], acc);
                    p.out[(f * T + i) * C + h * dh + d] = acc / sum;
                }
                p.lse[(f * H + h) * T + i] = m + logf(sum);
            }
        }
    return 0;
}

inline int pit_attention_bwd(const PitAttn& p, hipStream_t) {
    if (const char* why = pit_attn_refusal(p, true)) return pit_host_refuse("pit_attention_bwd", why);
    const int T = p.T, H = p.H, dh = p.dh, C = H * dh;
    std::vector<float> P((size_t)T), dS((size_t)T);
    for (int64_t f = 0; f < p.F; ++f)
        for (int h = 0; h < H; ++h) {
            const float *q = p.qkv + f * T * 3 * C + h * dh, *k = q + C, *v = q + 2 * C;
            float *dq = p.dqkv + f * T * 3 * C + h * dh, *dk = dq + C, *dv = dq + 2 * C;
            for (int j = 0; j < T; ++j)
                for (int d = 0; d < dh; ++d) dk[(int64_t)j * 3 * C + d] = dv[(int64_t)j * 3 * C + d] = 0.f;
            for (int i = 0; i < T; ++i) {                                   // the queries in increasing order: one owner, one order
                const float *qr = q + (int64_t)i * 3 * C, *gr = p.dout + (f * T + i) * C + h * dh, *orow = p.out + (f * T + i) * C + h * dh;
                const int64_t st = (f * H + h) * T + i;
                float delta = 0.f;
                for (int d = 0; d < dh; ++d) delta = fmaf(gr[d], orow[d], delta);
                p.delta[st] = delta;
                pit_host_scores(qr, k, 3 * C, T, dh, p.scale, P.data());
                for (int j = 0; j < T; ++j) {
                    P[j] = expf(P[j] - p.lse[st]);                          // no row reduction: the statistics are the forward's
                    float acc = 0.f;
                    for (int d = 0; d < dh; ++d) acc = fmaf(gr[d], v[(int64_t)j * 3 * C + d], acc);
                    dS[j] = p.scale * (P[j] * (acc - delta));
                }
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

inline int pit_pool(const PitPool& p, hipStream_t) {
    if (const char* why = pit_pool_refusal(p)) return pit_host_refuse("pit_pool", why);
    const int g = p.g, C = p.C, go = (g - 1) / 2 + 1;
    for (int64_t f = 0; f < p.F; ++f)
        for (int oy = 0; oy < go; ++oy)
            for (int ox = 0; ox < go; ++ox)
                for (int o = 0; o < 2 * C; ++o) {
                    float acc = p.b ? p.b[o] : 0.f;
                    for (int ky = 0; ky < 3; ++ky)
                        for (int kx = 0; kx < 3; ++kx) {
                            const int iy = 2 * oy - 1 + ky, ix = 2 * ox - 1 + kx;
                            if (iy < 0 || iy >= g || ix < 0 || ix >= g) continue;
                            acc = fmaf(p.w[(int64_t)o * 9 + 3 * ky + kx], p.x[f * p.xs + ((int64_t)iy * g + ix) * C + o / 2], acc);
                        }
                    p.y[f * p.ys + ((int64_t)oy * go + ox) * 2 * C + o] = acc;
                }
    return 0;
}

inline int pit_pool_bwd(const PitPool& p, hipStream_t) {
    if (const char* why = pit_pool_refusal(p)) return pit_host_refuse("pit_pool_bwd", why);
    const int g = p.g, C = p.C, go = (g - 1) / 2 + 1;
    for (int64_t f = 0; f < p.F; ++f)
        for (int iy = 0; iy < g; ++iy)
            for (int ix = 0; ix < g; ++ix)
                for (int c = 0; c < C; ++c) {
                    float acc = 0.f;
                    for (int ky = 0; ky < 3; ++ky)
                        for (int kx = 0; kx < 3; ++kx) {
                            const int ty = iy + 1 - ky, tx = ix + 1 - kx;
                            if (ty < 0 || tx < 0 || (ty & 1) || (tx & 1) || ty / 2 >= go || tx / 2 >= go) continue;
                            const float* d = p.x + f * p.ys + ((int64_t)(ty / 2) * go + tx / 2) * 2 * C + 2 * c;
                            acc = fmaf(p.w[(int64_t)(2 * c) * 9 + 3 * ky + kx], d[0], acc);
                            acc = fmaf(p.w[(int64_t)(2 * c + 1) * 9 + 3 * ky + kx], d[1], acc);
                        }
                    float* dx = p.y + f * p.xs + ((int64_t)iy * g + ix) * C + c;
                    *dx = p.accumulate ? *dx + acc : acc;
                }
    return 0;
}

inline int pit_patch_gather(const PitPatch& p, hipStream_t) {
    if (const char* why = pit_patch_refusal(p)) return pit_host_refuse("pit_patch_gather", why);
    const int P = p.p, S = p.s, side = p.side, g = (side - P) / S + 1;
    const int64_t KP = (int64_t)p.Cin * P * P;
    for (int64_t f = 0; f < p.F; ++f)
        for (int py = 0; py < g; ++py)
            for (int px = 0; px < g; ++px)
                for (int c = 0; c < p.Cin; ++c)
                    for (int dy = 0; dy < P; ++dy)
                        for (int dx = 0; dx < P; ++dx)
                            p.dst[((f * g + py) * g + px) * KP + ((int64_t)c * P + dy) * P + dx] =
                                p.src[((f * p.Cin + c) * side + py * S + dy) * side + px * S + dx];
    return 0;
}

inline int pit_patch_scatter(const PitPatch& p, hipStream_t) {
    if (const char* why = pit_patch_refusal(p)) return pit_host_refuse("pit_patch_scatter", why);
    const int P = p.p, S = p.s, side = p.side, g = (side - P) / S + 1;
    const int64_t KP = (int64_t)p.Cin * P * P;
    for (int64_t f = 0; f < p.F; ++f)
        for (int c = 0; c < p.Cin; ++c)
            for (int y = 0; y < side; ++y)
                for (int x = 0; x < side; ++x) {
                    const int py0 = std::max(0, (y - P + S) / S), py1 = std::min(g - 1, y / S);
                    const int px0 = std::max(0, (x - P + S) / S), px1 = std::min(g - 1, x / S);
                    float acc = 0.f;
                    for (int py = py0; py <= py1; ++py)
                        for (int px = px0; px <= px1; ++px)
                            acc = acc + p.src[((f * g + py) * g + px) * KP + ((int64_t)c * P + (y - py * S)) * P + (x - px * S)];
                    float* d = p.dst + ((f * p.Cin + c) * side + y) * side + x;
                    *d = p.accumulate ? *d + acc : acc;
                }
    return 0;
}
