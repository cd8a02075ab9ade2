// What the transformer planners need where there is no HIP (the host simulation's one-file build, g++): a stand-in for the few runtime
// calls of i2v_xf.h on host memory, and the shared launches the planners use -- vit_gemm, the LayerNorm pair, the row softmax pair,
// vit_patchify, vit_assemble and the 2 x 2 gather / scatter -- as plain scalar C++, in the style of i2v_se_host.h and i2v_convnext_host.h.  The same definitions as the
// kernels (i2v_vit_kernels.h, i2v_swin_kernels.h); the ORDER of their sums is a simple one (one fma chain in increasing k; a row's
// channels as 64 interleaved partial sums and a pairwise tree over them, xf_host_rowsum) and is NOT the device's, so these are held to
// the float64 bound, not to the device's bits.  The softmax pair is one running sum over a row; only expf is the host's own.
// Window attention has no host form, and the ViT and Swin planners are not part of the one-file build: they stay device-only.
#pragma once
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "i2v_hip_stub.h"
#include "i2v_kernels.h"         // i2v_api_fail
#include "i2v_vit_kernels.h"
#include "i2v_swin_kernels.h"

inline float xf_host_gelu(float x) { return 0.5f * x * (1.f + erff(x * 0.70710678118654752f)); }
inline float xf_host_gelu_grad(float x) {
    return 0.5f * (1.f + erff(x * 0.70710678118654752f)) + x * 0.39894228040143268f * expf(-0.5f * x * x);
}

inline int vit_launch_check(const char*) { return 0; }

inline int vit_gemm(VitGemm p, hipStream_t) {
    if (p.M <= 0 || p.N <= 0 || p.batch <= 0) return 0;
    if (p.nb_in <= 0) p.nb_in = 1;
    // the device launch's refusals, in its order and its words (i2v_vit.hip)
    if (p.a_sk != 1 && p.a_sm != 1) return i2v_api_fail("vit_gemm: A must be contiguous along M or K");
    if (p.b_sk != 1 && p.b_sn != 1) return i2v_api_fail("vit_gemm: B must be contiguous along K or N");
    if (p.mode == VIT_EPI_GELU && !p.C2) return i2v_api_fail("vit_gemm: the GELU epilogue needs its second output");
    if (p.mode == VIT_EPI_GELU_BWD && !p.H) return i2v_api_fail("vit_gemm: the GELU backward epilogue needs the pre-activation");
    if (p.K <= 0) return i2v_api_fail("vit_gemm: K must be positive");
    if (p.batch > 65535) return i2v_api_fail("vit_gemm: grid too large");
    for (int b = 0; b < p.batch; ++b) {
        const int64_t bo = b / p.nb_in, bi = b % p.nb_in;
        const float* A = p.A + bo * p.a_bo + bi * p.a_bi;
        const float* B = p.B + bo * p.b_bo + bi * p.b_bi;
        const int64_t co = bo * p.c_bo + bi * p.c_bi;
        for (int m = 0; m < p.M; ++m)
            for (int n = 0; n < p.N; ++n) {
                float acc = 0.f;
                for (int k = 0; k < p.K; ++k) acc = fmaf(A[m * p.a_sm + k * p.a_sk], B[k * p.b_sk + n * p.b_sn], acc);
                const int64_t o = co + m * p.c_sm + n;
                float v = p.alpha * acc;
                if (p.bias) v = v + p.bias[n];
                if (p.R) v = v + p.R[o];
                if (p.mode == VIT_EPI_GELU_BWD) v = v * xf_host_gelu_grad(p.H[o]);
                p.C[o] = v;
                if (p.mode == VIT_EPI_GELU) p.C2[o] = xf_host_gelu(v);
            }
    }
    return 0;
}

// The sum of term(c) over a row's C channels: 64 partial sums over the channels c % 64, then a pairwise tree.  One running sum over a
// wide row loses what LayerNorm needs from it: over 770 channels of mean 100 and spread 0.01 its mean is off by 2e-5, a fifth of a
// percent of the spread, which the variance then takes for signal (rstd off by 2.2e-6, dx by 8e-5 of its largest element, where plain
// float32 torch is within 2.1e-7 and 1.5e-5: tests/xf_cases.py, ln-r4-C770-mean100).
template <class Term>
inline float xf_host_rowsum(int C, Term term) {
    float part[64];
    for (int l = 0; l < 64; ++l) part[l] = 0.f;
    for (int c = 0; c < C; ++c) part[c & 63] = part[c & 63] + term(c);
    for (int o = 32; o > 0; o >>= 1)
        for (int l = 0; l < o; ++l) part[l] = part[l] + part[l + o];
    return part[0];
}

inline int vit_layernorm(const float* x, int64_t rows, int C, const float* gamma, const float* beta, float eps, float* out, float* mean,
                         float* rstd, hipStream_t) {
    for (int64_t r = 0; r < rows; ++r) {
        const float* xr = x + r * C;
        const float mu = xf_host_rowsum(C, [&](int c) { return xr[c]; }) / (float)C;
        const float q = xf_host_rowsum(C, [&](int c) { return (xr[c] - mu) * (xr[c] - mu); });
        const float rs = 1.f / sqrtf(q / (float)C + eps);
        for (int c = 0; c < C; ++c) out[r * C + c] = (xr[c] - mu) * rs * gamma[c] + beta[c];
        mean[r] = mu;
        rstd[r] = rs;
    }
    return 0;
}

inline int vit_layernorm_bwd(const float* dy, const float* x, const float* mean, const float* rstd, const float* gamma, int64_t rows, int C,
                             const float* add0, const float* add1, float* dx, hipStream_t) {
    for (int64_t r = 0; r < rows; ++r) {
        const float mu = mean[r], rs = rstd[r];
        const float s1 = xf_host_rowsum(C, [&](int c) { return dy[r * C + c] * gamma[c]; });
        const float s2 = xf_host_rowsum(C, [&](int c) { return (dy[r * C + c] * gamma[c]) * ((x[r * C + c] - mu) * rs); });
        const float m1 = s1 / (float)C, m2 = s2 / (float)C;
        for (int c = 0; c < C; ++c) {
            const int64_t o = r * C + c;
            float v = rs * (dy[o] * gamma[c] - m1 - (x[o] - mu) * rs * m2);
            if (add0) v = v + add0[o];
            if (add1) v = v + add1[o];
            dx[o] = v;
        }
    }
    return 0;
}

inline int vit_patchify(const float* img, float* patches, int F, int Cin, int gh, int gw, int P, float* gimg, int accumulate, hipStream_t) {
    const int64_t H = (int64_t)gh * P, W = (int64_t)gw * P;
    for (int f = 0; f < F; ++f)
        for (int py = 0; py < gh; ++py)
            for (int px = 0; px < gw; ++px)
                for (int c = 0; c < Cin; ++c)
                    for (int dy = 0; dy < P; ++dy)
                        for (int dx = 0; dx < P; ++dx) {
                            const int64_t row = ((int64_t)f * gh + py) * gw + px, col = ((int64_t)c * P + dy) * P + dx;
                            const int64_t pi = row * ((int64_t)Cin * P * P) + col, ii = (((int64_t)f * Cin + c) * H + py * P + dy) * W + px * P + dx;
                            if (!gimg) patches[pi] = img[ii];
                            else gimg[ii] = accumulate ? gimg[ii] + patches[pi] : patches[pi];
                        }
    return 0;
}

// X (rows, ld) = softmax over the first N of each row, in place
inline int vit_softmax(float* X, int64_t rows, int N, int ld, hipStream_t) {
    if (ld % 4 != 0 || ld < N || ((uintptr_t)X & 15)) return i2v_api_fail("vit_softmax: rows must be 16-byte aligned (ld % 4 == 0, ld >= N)");
    for (int64_t r = 0; r < rows; ++r) {
        float* x = X + r * ld;
        float m = -INFINITY, sum = 0.f;
        for (int j = 0; j < N; ++j) m = fmaxf(m, x[j]);
        for (int j = 0; j < N; ++j) { x[j] = expf(x[j] - m); sum = sum + x[j]; }
        for (int j = 0; j < N; ++j) x[j] = x[j] / sum;
    }
    return 0;
}

// dX = scale P (dX - rowsum(dX P)) in place
inline int vit_softmax_bwd(float* dX, const float* P, int64_t rows, int N, int ld, float scale, hipStream_t) {
    if (ld % 4 != 0 || ld < N || (((uintptr_t)dX | (uintptr_t)P) & 15))
        return i2v_api_fail("vit_softmax_bwd: rows must be 16-byte aligned (ld % 4 == 0, ld >= N)");
    for (int64_t r = 0; r < rows; ++r) {
        float* d = dX + r * ld;
        const float* p = P + r * ld;
        float sum = 0.f;
        for (int j = 0; j < N; ++j) sum = sum + d[j] * p[j];
        for (int j = 0; j < N; ++j) d[j] = scale * (p[j] * (d[j] - sum));
    }
    return 0;
}

// x (F, T, C) = [prefix (n_prefix, C); E (F, T - n_prefix, C)] + pos (T, C)
inline int vit_assemble(const float* E, const float* prefix, int n_prefix, const float* pos, float* x, int F, int T, int C, hipStream_t) {
    if (!E || !prefix || !pos || !x) return i2v_api_fail("vit_assemble: null argument");
    if (n_prefix < 1 || n_prefix >= T) return i2v_api_fail("vit_assemble: the prefix tokens must leave at least one patch row");
    const int np = T - n_prefix;
    for (int64_t f = 0; f < F; ++f)
        for (int t = 0; t < T; ++t)
            for (int c = 0; c < C; ++c) {
                const float v = t < n_prefix ? prefix[(int64_t)t * C + c] : E[(f * np + t - n_prefix) * C + c];
                x[(f * T + t) * C + c] = v + pos[(int64_t)t * C + c];
            }
    return 0;
}

// quarter q of a gathered row: the position at (row, column) offset (q & 1, q >> 1) of its 2 x 2 cell
inline int xf_host_merge(const float* in, float* out, int F, int H, int W, int C, const float* add, int scatter) {
    if (H % 2 || W % 2) return 1;
    for (int f = 0; f < F; ++f)
        for (int y = 0; y < H; ++y)
            for (int x = 0; x < W; ++x)
                for (int c = 0; c < C; ++c) {
                    const int q = (y & 1) + 2 * (x & 1);
                    const int64_t full = (((int64_t)f * H + y) * W + x) * C + c;
                    const int64_t cell = ((((int64_t)f * (H / 2) + y / 2) * (W / 2) + x / 2) * 4 + q) * C + c;
                    if (!scatter) out[cell] = in[full];
                    else out[full] = add ? in[cell] + add[full] : in[cell];
                }
    return 0;
}
inline int swin_merge_gather(const float* x, int F, int H, int W, int C, float* out, hipStream_t) { return xf_host_merge(x, out, F, H, W, C, nullptr, 0); }
inline int swin_merge_scatter(const float* dout, int F, int H, int W, int C, const float* add, float* dx, hipStream_t) {
    return xf_host_merge(dout, dx, F, H, W, C, add, 1);
}
