// What k_gconv and k_dwconv are given, as plain host functions: the packed operands (I2VGConvParams::w, I2VDwConvParams::w), the tap masks
// and the per-class geometry of a launch.  No Net and no Node: the planner (pack_gconv / pack_dwconv in i2v_pack.cpp, gconv_launch /
// dwconv_launch in i2v_plan.cpp) and the launches' own C entries (i2v_conv_aux_api.cpp) call the same code, so there is one packing.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "i2v_params.h"

namespace eng {
namespace conv_aux {

inline int fdiv(int a, int b) { return (a >= 0) ? a / b : -((-a + b - 1) / b); }
inline int pmod(int a, int b) { int m = a % b; return m < 0 ? m + b : m; }

// floats of the operands
inline size_t gconv_fwd_floats(int G, int gw) { return (size_t)G * gw * 9 * gw; }
inline size_t gconv_bwd_floats(int G, int gw, int st) { return (size_t)st * st * gconv_fwd_floats(G, gw); }
inline size_t dwconv_bwd_floats(int C, int k, int st) { return (size_t)st * st * C * k * k; }

// k_gconv's forward operand [group][ci][tap 3 r + s][co] from the compact kernel wg [G gw co][gw ci][3][3]
inline void gconv_pack_fwd(const float* wg, int G, int gw, float* wf) {
    for (int g = 0; g < G; ++g)
        for (int co = 0; co < gw; ++co)
            for (int ci = 0; ci < gw; ++ci)
                for (int t = 0; t < 9; ++t)
                    wf[(((size_t)g * gw + ci) * 9 + t) * gw + co] = wg[(((size_t)(g * gw + co)) * gw + ci) * 9 + t];
}

// k_gconv's input-gradient operand: per stride-parity class (ph, pw), class ph st + pw, [group][co][slot 3 a + b][ci] with
// a - 1 = (ph + 1 - r) / stride for the row taps r the class owns (b alike), zeros in the slots it does not; tapmask[cls] has a bit per
// owned slot.  `wb` holds gconv_bwd_floats floats and is written whole.
inline void gconv_pack_bwd(const float* wg, int G, int gw, int st, float* wb, int* tapmask) {
    for (size_t i = 0, n = gconv_bwd_floats(G, gw, st); i < n; ++i) wb[i] = 0.f;
    for (int ph = 0; ph < st; ++ph)
        for (int pw = 0; pw < st; ++pw) {
            const int cls = ph * st + pw;
            int mask = 0;
            for (int r = 0; r < 3; ++r) {
                if (pmod(ph + 1 - r, st)) continue;
                const int a = fdiv(ph + 1 - r, st) + 1;
                for (int s = 0; s < 3; ++s) {
                    if (pmod(pw + 1 - s, st)) continue;
                    const int b = fdiv(pw + 1 - s, st) + 1;
                    mask |= 1 << (3 * a + b);
                    for (int g = 0; g < G; ++g)
                        for (int co = 0; co < gw; ++co)
                            for (int ci = 0; ci < gw; ++ci)
                                wb[((((size_t)cls * G + g) * gw + co) * 9 + 3 * a + b) * gw + ci] = wg[(((size_t)(g * gw + co)) * gw + ci) * 9 + 3 * r + s];
                }
            }
            tapmask[cls] = mask;
        }
}

// k_dwconv's input-gradient operand (the forward operand is the filter wg [C][k r + s] as it is): per stride-parity class, [C][slot
// k a + b] with a - pad = (ph + pad - r) / stride for the row taps r the class owns (b alike): the mirrored filter, zeros in the slots
// the class does not own; tapmask[cls] has a bit per owned slot.  `wb` holds dwconv_bwd_floats floats and is written whole.
inline void dwconv_pack_bwd(const float* wg, int C, int k, int st, float* wb, int* tapmask) {
    const int pad = k / 2, nt = k * k;
    for (size_t i = 0, n = dwconv_bwd_floats(C, k, st); i < n; ++i) wb[i] = 0.f;
    for (int ph = 0; ph < st; ++ph)
        for (int pw = 0; pw < st; ++pw) {
            const int cls = ph * st + pw;
            int mask = 0;
            for (int r = 0; r < k; ++r) {
                if (pmod(ph + pad - r, st)) continue;
                const int a = fdiv(ph + pad - r, st) + pad;
                for (int s = 0; s < k; ++s) {
                    if (pmod(pw + pad - s, st)) continue;
                    const int b = fdiv(pw + pad - s, st) + pad;
                    mask |= 1 << (k * a + b);
                    for (int ch = 0; ch < C; ++ch) wb[((size_t)cls * C + ch) * nt + k * a + b] = wg[(size_t)ch * nt + k * r + s];
                }
            }
            tapmask[cls] = mask;
        }
}

// The classes of one launch over a destination plane q.Ho x q.Wo (set by the caller), for I2VGConvParams and I2VDwConvParams alike.
// Forward: one class over the whole plane with all `ntaps` slots, S = stride, os = 1.  Input gradient: S = 1, os = stride, one class per
// stride parity (oh0, ow0) = (ph, pw) over the positions of that parity, with the slots `tapmask` (of the pack functions above) gives it.
template <class Params>
inline void conv_classes(Params& q, bool backward, int st, int ntaps, const int* tapmask) {
    if (!backward) {
        q.S = st; q.os = 1; q.ncls = 1;
        q.cls[0].Hg = q.Ho; q.cls[0].Wg = q.Wo; q.cls[0].oh0 = 0; q.cls[0].ow0 = 0; q.cls[0].tapmask = (1 << ntaps) - 1;
        return;
    }
    q.S = 1; q.os = st; q.ncls = st * st;
    for (int ph = 0; ph < st; ++ph)
        for (int pw = 0; pw < st; ++pw) {
            auto& k = q.cls[ph * st + pw];
            k.Hg = (q.Ho - ph + st - 1) / st; k.Wg = (q.Wo - pw + st - 1) / st; k.oh0 = ph; k.ow0 = pw; k.tapmask = tapmask[ph * st + pw];
        }
}

}  // namespace conv_aux
}  // namespace eng
