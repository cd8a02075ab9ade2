/* libi2v_hip.so -- the launches that every transformer-stack surrogate shares (csrc/i2v_vit.hip: ViT / DeiT, Swin, ConvNeXt, MLP-Mixer /
 * ResMLP, CaiT, ConViT and XCiT compose their blocks from them), reachable on their own with arbitrary descriptors: tests and tools.
 * No planner calls these entries and they change no launch.
 *
 * Same conventions as i2v_hip.h: every function returns 0 on success and non-zero on error with the text in `i2v_last_error()`; tensors
 * are caller-owned fp32 pointers of the library's memory space (device pointers in libi2v_hip.so, host pointers in the host
 * simulation); work is enqueued on `stream` (a hipStream_t as void*, 0 = default) and nothing synchronises the host.
 */
#ifndef I2V_XF_LAUNCH_H
#define I2V_XF_LAUNCH_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum { I2V_XF_EPI_PLAIN = 0, I2V_XF_EPI_GELU = 1, I2V_XF_EPI_GELU_BWD = 2 };

/* C[b](m, n) = alpha * sum_k A[b](m, k) B[b](k, n) (+ bias[n]) (+ R[b](m, n)), then the epilogue `mode`:
 *   I2V_XF_EPI_GELU      C = that value (the pre-activation), C2 = gelu(C)
 *   I2V_XF_EPI_GELU_BWD  C = that value * gelu'(H[b](m, n))
 * Batch b = outer * nb_in + inner (nb_in <= 0 counts as 1); operand X's element is X + outer * x_bo + inner * x_bi + row * stride +
 * col * stride, strides in floats.  A must be contiguous along M (a_sm == 1) or K (a_sk == 1), B along K (b_sk == 1) or N (b_sn == 1);
 * C, R, C2 and H share C's strides and are contiguous along N; bias, R, C2 and H may be null where the mode does not need them.  R may
 * alias C, element for element.  Each operand is read and written 16 bytes at a time where its base is 16-byte aligned and its leading
 * dimension and batch strides are multiples of 4 floats, element by element otherwise -- the launch decides, the caller need not.
 * M <= 0, N <= 0 or batch <= 0: nothing to do, 0.  Refused: A or B contiguous along neither axis, the GELU epilogue without C2, the GELU
 * backward epilogue without H, K <= 0, batch > 65535. */
typedef struct {
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
} i2v_xf_gemm_desc;

/* Exported by every build of the C ABI: the host simulation runs the same definition as scalar host code. */
int i2v_xf_gemm_f32(const i2v_xf_gemm_desc* desc, void* stream);

/* LayerNorm over the last axis and its backward, and the image <-> patch-row copy (gimg null: img (F, in_chans, gh*patch, gw*patch) ->
 * patches (F*gh*gw, in_chans*patch*patch); else the patch rows' gradient -> gimg, written or added with `accumulate`), as the planners
 * launch them.  `i2v_vit_layernorm_f32`, `i2v_vit_layernorm_bwd_f32` (i2v_vit.h) are the first two under the names the ViT tests use;
 * these exist so that the host simulation, which has no ViT, exports them too. */
int i2v_xf_layernorm_f32(const float* x, int64_t rows, int C, const float* gamma, const float* beta, float eps, float* out, float* mean,
                         float* rstd, void* stream);
int i2v_xf_layernorm_bwd_f32(const float* dy, const float* x, const float* mean, const float* rstd, const float* gamma, int64_t rows, int C,
                             const float* add0, const float* add1, float* dx, void* stream);
int i2v_xf_patchify_f32(const float* img, float* patches, int F, int in_chans, int gh, int gw, int patch, float* gimg, int accumulate,
                        void* stream);

/* Row softmax in place over the first N of `ld` floats of each of `rows` rows of X, and its backward in place on dX:
 * dX = scale * P * (dX - sum_j dX P).  Columns [N, ld) are neither read nor written.  Refused: ld % 4 != 0, ld < N, X / dX / P not
 * 16-byte aligned.  libi2v_hip.so only: the softmax has no host form. */
int i2v_xf_softmax_f32(float* X, int64_t rows, int N, int ld, void* stream);
int i2v_xf_softmax_bwd_f32(float* dX, const float* P, int64_t rows, int N, int ld, float scale, void* stream);

#ifdef __cplusplus
}
#endif
#endif
