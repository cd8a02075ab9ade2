// The shortcut pair (k_conv_scpair, i2v_kernels.h) where the library has no i2v_conv_scpair.hip (no -DI2V_HAVE_SCPAIR: the host
// simulation's one-file build): the two launches one after the other through the backend's k_conv -- the same values either way --
// and then the intermediate POISONED, as the device kernel never stores it: a reader the planner overlooked shows up as NaN in the
// CPU tests instead of passing on values the GPU would not have.
#pragma once
#include <algorithm>
#include <limits>

#include "i2v_kernels.h"

namespace eng {
namespace scpair_host {

inline int ok(const I2VConvParams& a, const I2VConvParams& b) { return i2v_conv_scpair_ok(a, b) ? 1 : 0; }

inline int run(const I2VConvParams& a, const I2VConvParams& b, i2v_stream_t s) {
    if (!i2v_conv_scpair_ok(a, b)) return 1;
    if (k_conv(a, s) || k_conv(b, s)) return 1;
    if (b.dst == a.dst) return 0;        // (an in-place addend: that memory now holds b's result, as after the device kernel)
    for (int64_t f = 0; f < (int64_t)a.N; ++f)
        std::fill(a.dst + f * a.dst_nstride, a.dst + f * a.dst_nstride + (int64_t)a.Cd * a.Ho * a.Wo, std::numeric_limits<float>::quiet_NaN());
    return 0;
}

}  // namespace scpair_host
}  // namespace eng
