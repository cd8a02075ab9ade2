// The exact (erf) GELU and its derivative, shared by the kernels that apply them (i2v_vit.hip's GEMM epilogues, i2v_mixer.hip's token
// tile) and, in the same operation order on the host's libm, by the scalar restatement i2v_mixer_host.h.  Every product and sum is
// written out (-ffp-contract=off keeps them apart); device and host differ only in erff / expf themselves.
#pragma once
#include <math.h>

#ifdef __HIP__
__device__ __forceinline__ float gelu_f(float h) {            // 0.5 h (1 + erf(h / sqrt 2)), torch's exact form
    return __fmul_rn(__fmul_rn(0.5f, h), __fadd_rn(1.f, erff(__fmul_rn(h, 0.70710678118654752f))));
}
__device__ __forceinline__ float gelu_grad_f(float h) {       // 0.5 (1 + erf(h / sqrt 2)) + h exp(-h^2 / 2) / sqrt(2 pi)
    const float cdf = __fmul_rn(0.5f, __fadd_rn(1.f, erff(__fmul_rn(h, 0.70710678118654752f))));
    const float pdf = __fmul_rn(expf(__fmul_rn(-0.5f, __fmul_rn(h, h))), 0.39894228040143268f);
    return __fadd_rn(cdf, __fmul_rn(h, pdf));
}
#endif

inline float gelu_host_f(float h) { return (0.5f * h) * (1.f + erff(h * 0.70710678118654752f)); }
inline float gelu_grad_host_f(float h) {
    const float cdf = 0.5f * (1.f + erff(h * 0.70710678118654752f));
    const float pdf = expf(-0.5f * (h * h)) * 0.39894228040143268f;
    return cdf + h * pdf;
}
