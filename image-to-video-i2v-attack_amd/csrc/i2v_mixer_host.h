// The token-mixing launch of the MLP-Mixer / ResMLP blocks as plain scalar C++ on the backend's memory: what the callers run where the
// library has no i2v_mixer.hip (no -DI2V_HAVE_MIXER: the host simulation's one-file build, whose backend memory is host memory).  The
// same operations in the same order as the kernel (I2VMixTokParams, i2v_params.h): one fma chain per product element from 0.f over the
// contracted index in increasing order, an odd length closed by one fma(0.f, 0.f, acc); then the bias of the row, GELU, the scales and
// the residual.  Only erff / expf are the host's own.
#pragma once
#include <math.h>
#include <stdint.h>

#include <vector>

#include "i2v_gelu.h"
#include "i2v_params.h"

namespace eng {
namespace mixer_host {

inline int plan(I2VMixTokParams* p) {
    if (!p->out || !p->r || p->F < 0 || p->S < 1 || p->Sh < 0 || p->C < 4 || p->C % 4 != 0) return 1;
    if ((p->in_scale == nullptr) != (p->in_shift == nullptr)) return 1;
    if (p->Sh > 0 ? (!p->z || !p->wa || !p->ba || !p->wb || (p->bwd ? !p->wc : !p->bb)) : (p->bwd ? !p->wb : (!p->z || !p->wa || !p->ba))) return 1;
    const int want = p->ct;
    if (want != 0 && want != 32 && want != 64) return 1;
    const int ct = want ? want : 32;
    if ((int64_t)(p->S + p->Sh) * ct * 4 > I2V_MIXTOK_LDS_MAX) return 1;
    p->ct = ct;
    p->lds_bytes = (p->S + p->Sh) * ct * 4;
    return 0;
}

// out[m][c] for m < M: the chain over k < K of w[m][k] * v[k][c], v (K, C)
inline float chain(const float* wrow, int K, const float* v, int C, int c) {
    float acc = 0.f;
    for (int k = 0; k < K; ++k) acc = fmaf(wrow[k], v[(int64_t)k * C + c], acc);
    if (K & 1) acc = fmaf(0.f, 0.f, acc);
    return acc;
}

inline int tokens(const I2VMixTokParams& p) {
    const int S = p.S, Sh = p.Sh, C = p.C;
    if (p.ct != 32 && p.ct != 64) return 1;       // not planned
    std::vector<float> X((size_t)S * C), H((size_t)(Sh > 0 ? Sh : 1) * C);
    for (int f = 0; f < p.F; ++f) {
        const int64_t fo = (int64_t)f * S * C;
        const bool need_t = !(p.bwd && Sh == 0);
        if (need_t)
            for (int s = 0; s < S; ++s)
                for (int c = 0; c < C; ++c) {
                    const float zv = p.z[fo + (int64_t)s * C + c];
                    X[(size_t)s * C + c] = p.in_scale ? fmaf(p.in_scale[c], zv, p.in_shift[c]) : zv;
                }
        if (Sh > 0)
            for (int m = 0; m < Sh; ++m)
                for (int c = 0; c < C; ++c) {
                    const float pre = chain(p.wa + (int64_t)m * S, S, X.data(), C, c) + p.ba[m];
                    H[(size_t)m * C + c] = p.bwd ? pre : gelu_host_f(pre);
                }
        if (p.bwd) {
            for (int s = 0; s < S; ++s)
                for (int c = 0; c < C; ++c) {
                    const float g = p.r[fo + (int64_t)s * C + c];
                    X[(size_t)s * C + c] = p.out_scale ? p.out_scale[c] * g : g;
                }
            if (Sh > 0)
                for (int m = 0; m < Sh; ++m)
                    for (int c = 0; c < C; ++c) {
                        const float dh = chain(p.wb + (int64_t)m * S, S, X.data(), C, c);
                        H[(size_t)m * C + c] = dh * gelu_grad_host_f(H[(size_t)m * C + c]);
                    }
        }
        // the last product: rows of the token axis again
        const float* W = p.bwd ? (Sh > 0 ? p.wc : p.wb) : (Sh > 0 ? p.wb : p.wa);
        const float* bias = p.bwd ? nullptr : (Sh > 0 ? p.bb : p.ba);
        const float* V = Sh > 0 ? H.data() : X.data();
        const int K = Sh > 0 ? Sh : S;
        std::vector<float> O((size_t)S * C);
        for (int m = 0; m < S; ++m)
            for (int c = 0; c < C; ++c) {
                float v = chain(W + (int64_t)m * K, K, V, C, c);
                const int64_t o = fo + (int64_t)m * C + c;
                if (!p.bwd) {
                    v = v + bias[m];
                    if (p.out_scale) v = p.out_scale[c] * v;
                    v = p.r[o] + v;
                } else {
                    if (p.in_scale) v = p.in_scale[c] * v;
                    if (p.add0) v = p.add0[o] + v;
                    if (p.add1) v = v + p.add1[o];
                }
                O[(size_t)m * C + c] = v;
            }
        for (size_t i = 0; i < O.size(); ++i) p.out[fo + (int64_t)i] = O[i];      // (out may be z, r or add0: written last)
    }
    return 0;
}

}  // namespace mixer_host
}  // namespace eng
