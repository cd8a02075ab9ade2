/* libi2v_hip.so -- C ABI of the all-MLP surrogates (timm 0.5.0's `MlpMixer` at 224 x 224: MLP-Mixer mixer_{s,b,l}{16,32}_224 and ResMLP
 * resmlp_{12,24,36}_224), forward to the hooked blocks and backward to the input, run on the transformer stack.  DESIGN.md section 19
 * states the model.
 *
 * Same conventions as i2v_hip.h, i2v_vit.h, i2v_swin.h and i2v_convnext.h: every function returns 0 on success and non-zero on error
 * with the text in `i2v_last_error()`; tensors are caller-owned contiguous fp32 DEVICE pointers; work is enqueued on `stream` (a
 * hipStream_t as void*, 0 = default) and nothing synchronises the host inside a forward or a backward.
 *
 * Model: the stem is a patch x patch convolution with stride patch and bias (in_chans -> dim): ViT's patch embedding with no prefix
 * token, no pos_embed and no norm.  S = (img / patch)^2 tokens, D = dim channels; activations are TOKEN-MAJOR, a frame is (S, D)
 * row-major.  Then `blocks` blocks:
 *   kind 0 (MLP-Mixer)   y = x + (W2 . gelu(W1 . LN1(x) + b1) + b2)   down the TOKEN axis, per channel; W1 (Sh, S), W2 (S, Sh)
 *                        x' = y + fc2(gelu(fc1(LN2(y))))               per token over channels; fc1 (mlp, D), fc2 (D, mlp)
 *   kind 1 (ResMLP)      y = x + ls1 * (W . (a1 * x + b1a) + b)        down the token axis; W (S, S); a1, b1a, ls1 per channel
 *                        x' = y + fc2'(gelu(fc1'(y)))                  with norm2 folded into fc1' and ls2 into fc2' by the caller
 * LayerNorm over channels, eps `ln_eps`; exact erf GELU.  A hook is the residual stream after a block, all tokens: S * D floats per
 * frame.
 *
 * ARITHMETIC of the token-mixing launch (csrc/i2v_mixer.hip; csrc/i2v_mixer_host.h is its scalar restatement):
 *   - every product element is ONE fp32 fma chain from 0 over the contracted index in increasing order (the fp32 MFMA, which is
 *     bitwise an fmaf chain); the index is stepped in pairs, so an odd length ends with one fma(0, 0, acc); operands beyond a tail
 *     are zero;
 *   - then + bias[row]; then GELU (backward: * gelu'(pre)); then * out_scale[c]; then residual + value (backward: * in_scale[c], then
 *     addend + value);
 *   - the affine in front is fma(in_scale[c], z, in_shift[c]);
 *   - the contracted index is never split across lanes or workgroups, and there are no atomics: the bits depend on neither the frame
 *     count, nor the frames a net was planned for, nor the channel tile. */
#ifndef I2V_MIXER_H
#define I2V_MIXER_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct i2v_mixer* i2v_mixer_handle;

typedef struct {
    int32_t img, patch, in_chans, dim, blocks;      /* input side, patch side, input channels, width D, blocks */
    int32_t tokens_hidden;                          /* Sh of the token MLP (dim / 2 for MLP-Mixer); 0 for kind 1 */
    int32_t mlp;                                    /* width of the channel MLP (4 dim) */
    int32_t kind;                                   /* 0 MLP-Mixer, 1 ResMLP */
    float ln_eps;
} i2v_mixer_config;

/* Weights: host fp32 arrays in this order, for the blocks 0 .. B-1 that run, B = deepest hooked block + 1:
 *   stem.proj.weight (dim, in_chans, patch, patch), stem.proj.bias (dim);
 *   kind 0, per block 12 arrays: norm1.weight, norm1.bias (D), mlp_tokens.fc1.weight (Sh, S), .fc1.bias (Sh), mlp_tokens.fc2.weight
 *     (S, Sh), .fc2.bias (S), norm2.weight, norm2.bias (D), mlp_channels.fc1.weight (mlp, D), .fc1.bias, mlp_channels.fc2.weight
 *     (D, mlp), .fc2.bias (D);
 *   kind 1, per block 9 arrays: norm1.alpha (D), norm1.beta (D), ls1 (D), linear_tokens.weight (S, S), .bias (S), then
 *     mlp_channels.fc1 with norm2 folded in -- weight[o][c] * alpha2[c], bias[o] + sum_c weight[o][c] * beta2[c] --, and
 *     mlp_channels.fc2 with ls2 folded in -- row o of the weight and element o of the bias times ls2[o].
 * The token weights are also uploaded transposed, so that both passes read them with the contracted index contiguous.
 * hook_blocks: zero-based block indices, distinct, in the order the hooks fire.  Uploads the weights and allocates the activation arena
 * for up to `max_frames` frames on `device` (synchronous: a planning step); sized in 64 bits before anything is allocated.  Refused
 * when (S + Sh) * 32 * 4 bytes do not fit the 160 KiB of LDS a workgroup may hold. */
int i2v_mixer_create(int device, const i2v_mixer_config* cfg, const float* const* weights, int n_weights, const int32_t* hook_blocks,
                     int n_hooks, int max_frames, i2v_mixer_handle* out);
int i2v_mixer_destroy(i2v_mixer_handle net);
/* Bytes of device memory the net holds (weights and arena). */
int64_t i2v_mixer_workspace_bytes(i2v_mixer_handle net);
/* x: (frames, in_chans, img, img), frames <= max_frames.  Runs up to the deepest hooked block, keeping what the backward needs. */
int i2v_mixer_forward(i2v_mixer_handle net, const float* x, int frames, void* stream);
/* d(cost)/d(x) of the last forward from the hooks' gradient views (all of them are read): written into gx (accumulate = 0) or added to
 * it (accumulate = 1).  gx: (frames, in_chans, img, img). */
int i2v_mixer_backward(i2v_mixer_handle net, float* gx, int accumulate, void* stream);
int i2v_mixer_hook_info(i2v_mixer_handle net, int hook, float** act, int64_t* act_stride, float** grad, int64_t* grad_stride, int64_t* D);
/* Copy hook `hook`'s activation (which = 0) or gradient (which = 1) for `frames` frames into out (frames, D), on `stream`. */
int i2v_mixer_read_hook(i2v_mixer_handle net, int hook, int which, float* out, int frames, void* stream);

/* ---- the kernel on its own (tests, tools) --------------------------------------------------------------------------------------
 * z, residual, out, g, add, dz: (frames, S, C), channels contiguous, C a multiple of 4.  With t = in_scale * z + in_shift per channel
 * (t = z when both are null; give both or neither) and out_scale per channel (1 when null):
 *   forward   out = residual + out_scale * (w2 . gelu(w1 . t + b1[row]) + b2[row])        w1 (Sh, S), w2 (S, Sh)
 *             Sh = 0: out = residual + out_scale * (w1 . t + b1[row])                     w1 (S, S); w2, b2 ignored
 *   backward  dz = in_scale * (w1t . (gelu'(w1 . t + b1[row]) * (w2t . (out_scale * g)))) + add     w2t = w2^T (Sh, S), w1t = w1^T (S, Sh)
 *             Sh = 0: dz = in_scale * (w2t . (out_scale * g)) + add                       w2t = w1^T (S, S); z, w1, b1, w1t ignored
 * `add` may be null.  out may be z or residual, dz may be g or add.  channel_tile: 0 (the planned tile: 32 channels, the faster one
 * where it was measured), or 32 / 64 to insist; the result does not depend on it.  Exported by every build of the C ABI: where the library has no
 * device kernel (the host simulation) the same operations run as scalar host code in the same order. */
int i2v_mixer_tokens_f32(const float* z, const float* residual, float* out, int frames, int S, int Sh, int C, const float* w1,
                         const float* b1, const float* w2, const float* b2, const float* in_scale, const float* in_shift,
                         const float* out_scale, int channel_tile, void* stream);
int i2v_mixer_tokens_bwd_f32(const float* z, const float* g, const float* add, float* dz, int frames, int S, int Sh, int C,
                             const float* w1, const float* b1, const float* w2t, const float* w1t, const float* in_scale,
                             const float* in_shift, const float* out_scale, int channel_tile, void* stream);

#ifdef __cplusplus
}
#endif
#endif
