// Internal interface of the ViT kernels (i2v_vit.hip) to their planner (i2v_vit.cpp).  Both are HIP translation units of the product
// library only: the CNN planner (i2v_engine.cpp) and its host simulation know nothing of them.
#pragma once
#ifdef __HIP__
#include <hip/hip_runtime.h>
#else
#include "i2v_hip_stub.h"     // (no HIP: the host simulation's build)
#endif
#include <stdint.h>

enum { VIT_EPI_PLAIN = 0, VIT_EPI_GELU = 1, VIT_EPI_GELU_BWD = 2 };

// C[b](m, n) = alpha * sum_k A[b](m, k) B[b](k, n) (+ bias[n]) (+ R[b](m, n)), then the epilogue `mode`:
//   VIT_EPI_GELU      C = that value (the pre-activation), C2 = gelu(C)
//   VIT_EPI_GELU_BWD  C = that value * gelu'(H[b](m, n))
// Batch b = outer * nb_in + inner; operand X's element is X + outer * x_bo + inner * x_bi + row * stride + col * stride.  A must be
// contiguous along M or K, B along K or N; C, R, C2 and H share C's strides and are contiguous along N.  R may alias C, element for element: the thread that stores C[m][n] is the only one that reads R[m][n], it reads it
// after the K loop and before the store, and K is never split across blocks -- i2v_convnext.cpp relies on it (x = x + fc2(...) in place).
struct VitGemm {
    const float* A; int64_t a_bo, a_bi, a_sm, a_sk;
    const float* B; int64_t b_bo, b_bi, b_sk, b_sn;
    float* C; int64_t c_bo, c_bi, c_sm;
    const float* bias;
    const float* R;
    float* C2;
    const float* H;
    int32_t M, N, K, batch, nb_in;
    float alpha;
    int32_t mode;
    int32_t a_vec, b_vec, c_vec, bias_vec;      // set by vit_gemm
};

int vit_gemm(VitGemm p, hipStream_t s);
int vit_layernorm(const float* x, int64_t rows, int C, const float* gamma, const float* beta, float eps, float* out, float* mean, float* rstd,
                  hipStream_t s);
int vit_layernorm_bwd(const float* dy, const float* x, const float* mean, const float* rstd, const float* gamma, int64_t rows, int C,
                      const float* add0, const float* add1, float* dx, hipStream_t s);
int vit_softmax(float* X, int64_t rows, int N, int ld, hipStream_t s);
int vit_softmax_bwd(float* dX, const float* P, int64_t rows, int N, int ld, float scale, hipStream_t s);
// gimg == nullptr: image -> patch rows; else the patch rows' gradient `patches` -> gimg (written, or added with `accumulate`)
int vit_patchify(const float* img, float* patches, int F, int Cin, int gh, int gw, int P, float* gimg, int accumulate, hipStream_t s);
// x (F, T, C) = [prefix (n_prefix, C); E (F, T - n_prefix, C)] + pos (T, C)
int vit_assemble(const float* E, const float* prefix, int n_prefix, const float* pos, float* x, int F, int T, int C, hipStream_t s);
int vit_launch_check(const char* what);
