// The token-major depthwise 7 x 7 launch as plain scalar C++ on the backend's memory: what the callers run where the library has no
// i2v_convnext.hip (no -DI2V_HAVE_CONVNEXT: the host simulation's one-file build, whose backend memory is host memory).  The same
// operations in the same order as the kernel (I2VCnDwParams, i2v_params.h): one fma chain over the 49 taps in row-major order from
// 0.f with zero operands outside the plane, then + b[c], then + add.
#pragma once
#include <math.h>
#include <stdint.h>

#include "i2v_params.h"

namespace eng {
namespace convnext_host {

inline int plan(I2VCnDwParams* p) {
    if (!p->x || !p->w || !p->y || p->H < 1 || p->W < 1 || p->C < 1) return 1;
    p->runs = (p->W + I2V_CNDW_RUN - 1) / I2V_CNDW_RUN;
    p->vec = 1;
    p->lanes = p->C;
    return 0;
}

inline int dw(const I2VCnDwParams& p) {
    const int H = p.H, W = p.W, C = p.C;
    if (p.runs != (W + I2V_CNDW_RUN - 1) / I2V_CNDW_RUN || p.lanes != C || p.N < 0) return 1;     // not planned
    if ((int64_t)p.N * H * W * C >= (1ll << 31)) return 1;
    for (int n = 0; n < p.N; ++n)
        for (int h = 0; h < H; ++h)
            for (int w = 0; w < W; ++w)
                for (int c = 0; c < C; ++c) {
                    float acc = 0.f;
                    for (int a = 0; a < 7; ++a)
                        for (int b = 0; b < 7; ++b) {
                            const int hs = h + a - 3, ws = w + b - 3;
                            const bool ok = hs >= 0 && hs < H && ws >= 0 && ws < W;
                            const float xv = ok ? p.x[(((int64_t)n * H + hs) * W + ws) * C + c] : 0.f;
                            acc = fmaf(p.w[(a * 7 + b) * C + c], xv, acc);
                        }
                    const int64_t o = (((int64_t)n * H + h) * W + w) * C + c;
                    float v = acc;
                    if (p.b) v = v + p.b[c];
                    if (p.add) v = v + p.add[o];
                    p.y[o] = v;
                }
    return 0;
}

}  // namespace convnext_host
}  // namespace eng
