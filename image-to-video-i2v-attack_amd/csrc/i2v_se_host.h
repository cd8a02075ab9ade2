// The squeeze-and-excitation node as plain scalar C++ on the backend's memory: what the engine units run where the library has no
// i2v_se.hip (no -DI2V_HAVE_SE: the host simulation's one-file build, whose backend memory is host memory).  The same operations in
// the same order as the kernels (I2VSeParams, i2v_params.h): lane partial sums, the 64-lane fold, the fma chains.
#pragma once
#include <math.h>
#include <stdint.h>

#include <vector>

#include "i2v_params.h"

namespace eng {
namespace se_host {

inline float tree64(float* v) {                 // lane 0 of: for o in 32, 16, .. 1: v[l] += v[l + o]
    for (int o = 32; o > 0; o >>= 1) for (int l = 0; l < o; ++l) v[l] = v[l] + v[l + o];
    return v[0];
}

inline int plan(I2VSeParams* p) {
    if (p->C < 1 || p->rd < 1 || p->HW < 1) return 1;
    p->inv_hw = 1.f / (float)p->HW;
    return 0;
}

inline int squeeze(const I2VSeParams& p) {
    for (int n = 0; n < p.N; ++n)
        for (int c = 0; c < p.C; ++c) {
            const float* x = p.x + (int64_t)n * p.x_nstride + (int64_t)c * p.HW;
            const float* g = p.backward ? p.g + (int64_t)n * p.g_nstride + (int64_t)c * p.HW : nullptr;
            float part[64];
            for (int l = 0; l < 64; ++l) {
                float acc = 0.f;
                for (int e = 4 * l; e < p.HW; e += 256)
                    for (int j = 0; j < 4 && e + j < p.HW; ++j) acc = acc + (g ? g[e + j] * x[e + j] : x[e + j]);
                part[l] = acc;
            }
            const float sum = tree64(part);
            if (p.backward) p.t[(int64_t)n * p.C + c] = sum;
            else p.m[(int64_t)n * p.C + c] = sum * p.inv_hw;
        }
    return 0;
}

inline int excite(const I2VSeParams& p) {
    const int C = p.C, rd = p.rd;
    std::vector<float> mid(rd);
    for (int n = 0; n < p.N; ++n) {
        const float* s = p.s + (int64_t)n * C;
        const float* v = p.backward ? p.t + (int64_t)n * C : p.m + (int64_t)n * C;
        const float* W = p.backward ? p.w2t : p.w1;
        for (int j = 0; j < rd; ++j) {
            float part[64];
            for (int l = 0; l < 64; ++l) {
                float acc = 0.f;
                for (int c = l; c < C; c += 64) {
                    float f = v[c];
                    if (p.backward) { const float sc = s[c]; f = (f * sc) * (1.f - sc); }
                    acc = fmaf(W[(int64_t)j * C + c], f, acc);
                }
                part[l] = acc;
            }
            const float sum = tree64(part);
            if (p.backward) mid[j] = p.h[(int64_t)n * rd + j] > 0.f ? sum : 0.f;
            else { const float hv = sum + p.b1[j]; mid[j] = hv > 0.f ? hv : 0.f; p.h[(int64_t)n * rd + j] = mid[j]; }
        }
        const float* V = p.backward ? p.w1 : p.w2t;
        for (int c = 0; c < C; ++c) {
            float acc = 0.f;
            for (int j = 0; j < rd; ++j) acc = fmaf(V[(int64_t)j * C + c], mid[j], acc);
            if (p.backward) p.dmh[(int64_t)n * C + c] = acc * p.inv_hw;
            else p.s[(int64_t)n * C + c] = 1.f / (1.f + expf(-(acc + p.b2[c])));
        }
    }
    return 0;
}

inline int scale(const I2VSeParams& p) {
    for (int n = 0; n < p.N; ++n)
        for (int c = 0; c < p.C; ++c) {
            const int64_t nc = (int64_t)n * p.C + c, off = (int64_t)c * p.HW;
            const float* a = (p.backward ? p.g + (int64_t)n * p.g_nstride : p.x + (int64_t)n * p.x_nstride) + off;
            const float* r = (!p.backward && p.r) ? p.r + (int64_t)n * p.r_nstride + off : nullptr;
            float* d = p.dst + (int64_t)n * p.dst_nstride + off;
            const float sc = p.s[nc];
            for (int i = 0; i < p.HW; ++i) {
                float u = a[i] * sc;
                if (r) u = u + r[i]; else if (p.backward) u = u + p.dmh[nc];
                if (p.relu) u = u > 0.f ? u : 0.f;
                d[i] = u;
                if (p.gate_out) {
                    const size_t b = (size_t)n * p.HW + i;
                    uint32_t& w = p.gate_out[(size_t)c * p.gate_out_stride + (b >> 5)];
                    w = u > 0.f ? (w | (1u << (b & 31))) : (w & ~(1u << (b & 31)));
                }
            }
        }
    return 0;
}

}  // namespace se_host
}  // namespace eng
