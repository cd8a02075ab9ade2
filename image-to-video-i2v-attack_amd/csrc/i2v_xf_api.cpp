// The shared transformer launches on their own (include/i2v_xf_launch.h): thin C entries over vit_gemm, the LayerNorm pair, vit_patchify
// and the softmax pair, for tests and tools.  i2v_xf.h picks the kernels (i2v_vit.hip) or, where there is no HIP, their scalar
// restatements (i2v_xf_host.h), so this unit is part of the library and of the host simulation's one-file build alike; the softmax
// pair's entries are the device library's only.
#include "../../include/i2v_xf_launch.h"
#include "i2v_xf.h"

static_assert((int)I2V_XF_EPI_PLAIN == (int)VIT_EPI_PLAIN && (int)I2V_XF_EPI_GELU == (int)VIT_EPI_GELU &&
              (int)I2V_XF_EPI_GELU_BWD == (int)VIT_EPI_GELU_BWD, "the public epilogue modes are the launch's");

extern "C" int i2v_xf_gemm_f32(const i2v_xf_gemm_desc* d, void* stream) {
    if (!d) return fail("i2v_xf_gemm_f32: null descriptor");
    VitGemm g{};                                 // (the four *_vec fields stay vit_gemm's to set)
    g.A = d->A; g.a_bo = d->a_bo; g.a_bi = d->a_bi; g.a_sm = d->a_sm; g.a_sk = d->a_sk;
    g.B = d->B; g.b_bo = d->b_bo; g.b_bi = d->b_bi; g.b_sk = d->b_sk; g.b_sn = d->b_sn;
    g.C = d->C; g.c_bo = d->c_bo; g.c_bi = d->c_bi; g.c_sm = d->c_sm;
    g.bias = d->bias; g.R = d->R; g.C2 = d->C2; g.H = d->H;
    g.M = d->M; g.N = d->N; g.K = d->K; g.batch = d->batch; g.nb_in = d->nb_in;
    g.alpha = d->alpha;
    g.mode = d->mode;
    return vit_gemm(g, (hipStream_t)stream);
}

extern "C" int i2v_xf_layernorm_f32(const float* x, int64_t rows, int C, const float* gamma, const float* beta, float eps, float* out,
                                    float* mean, float* rstd, void* stream) {
    return vit_layernorm(x, rows, C, gamma, beta, eps, out, mean, rstd, (hipStream_t)stream);
}

extern "C" int i2v_xf_layernorm_bwd_f32(const float* dy, const float* x, const float* mean, const float* rstd, const float* gamma,
                                        int64_t rows, int C, const float* add0, const float* add1, float* dx, void* stream) {
    return vit_layernorm_bwd(dy, x, mean, rstd, gamma, rows, C, add0, add1, dx, (hipStream_t)stream);
}

extern "C" int i2v_xf_patchify_f32(const float* img, float* patches, int F, int in_chans, int gh, int gw, int patch, float* gimg,
                                   int accumulate, void* stream) {
    return vit_patchify(img, patches, F, in_chans, gh, gw, patch, gimg, accumulate, (hipStream_t)stream);
}

#ifdef __HIP__
extern "C" int i2v_xf_softmax_f32(float* X, int64_t rows, int N, int ld, void* stream) {
    return vit_softmax(X, rows, N, ld, (hipStream_t)stream);
}

extern "C" int i2v_xf_softmax_bwd_f32(float* dX, const float* P, int64_t rows, int N, int ld, float scale, void* stream) {
    return vit_softmax_bwd(dX, P, rows, N, ld, scale, (hipStream_t)stream);
}
#endif
