/* libi2v_hip.so -- C ABI of the Swin Transformer surrogates (timm's `SwinTransformer` at 224 x 224: swin_{tiny,small,base,large}_patch4_
 * window7_224), forward to the hooked stages and backward to the input.  DESIGN.md section 14 states the model.
 *
 * Same conventions as i2v_hip.h and i2v_vit.h: every function returns 0 on success and non-zero on error with the text in
 * `i2v_last_error()`; tensors are caller-owned contiguous fp32 DEVICE pointers; work is enqueued on `stream` (a hipStream_t as void*,
 * 0 = default) and nothing synchronises the host inside a forward or a backward.
 *
 * Model: patch embedding (a patch x patch convolution with stride patch and bias, in_chans -> dim), flattened row-major to a g x g grid of
 * tokens (g = img / patch), LayerNorm; no class token, no position embedding.  Stage i (0-based) is `depths[i]` blocks at width
 * dim * 2^i with `heads[i]` heads on a grid of g / 2^i; patch merging follows every stage but the last (2 x 2 cells concatenated in the
 * order (0,0), (1,0), (0,1), (1,1) as (row, column) offsets, LayerNorm over 4 width, Linear 4 width -> 2 width without bias).  A block is
 *   x = x + proj(WMSA(LN1(x)));  x = x + fc2(GELU(fc1(LN2(x))))         (MLP width 4 x the stage's width, exact erf GELU)
 * with window attention over window x window windows of the grid rolled by (-shift, -shift): shift 0 in even blocks of a stage,
 * window / 2 in odd ones, and window = grid, shift = 0 where the grid is not larger than the window.  Scores are
 * (q dh^-0.5) k^T + B + M: B[h, i, j] = relative_position_bias_table[(r_i - r_j + window - 1)(2 window - 1) + c_i - c_j + window - 1, h],
 * M = -100 where the two tokens lie in different ones of the 9 regions cut by [0, -window), [-window, -shift), [-shift, end) on each
 * axis of the rolled grid (shifted blocks only), 0 elsewhere.  Activations are TOKEN-MAJOR: a frame is (grid^2, width) row-major.
 *
 * A hook is the output of the last block of a stage, BEFORE that stage's patch merging: D = grid_i^2 * width_i floats per frame. */
#ifndef I2V_SWIN_H
#define I2V_SWIN_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct i2v_swin* i2v_swin_handle;

#define I2V_SWIN_MAX_STAGES 4

typedef struct {
    int32_t img, patch, in_chans, dim, window, stages;     /* input side, patch side, input channels, stage-0 width, window side, stages */
    int32_t depths[I2V_SWIN_MAX_STAGES];                    /* blocks per stage */
    int32_t heads[I2V_SWIN_MAX_STAGES];                     /* heads per stage: width_i / heads[i] is 32 with window 7, 16 with window 4 */
    float ln_eps;
} i2v_swin_config;

/* Weights: host fp32 arrays in this order (timm `state_dict` shapes), for the stages 0 .. S-1 that run, S = deepest hooked stage + 1:
 *   patch_embed.proj.weight (dim, in_chans, patch, patch), patch_embed.proj.bias (dim), patch_embed.norm.weight, patch_embed.norm.bias;
 *   then per stage i, per block j, 13 arrays: norm1.weight, norm1.bias, attn.qkv.weight (3 w, w), attn.qkv.bias (3 w),
 *   attn.relative_position_bias_table ((2 window - 1)^2, heads[i]), attn.proj.weight (w, w), attn.proj.bias, norm2.weight, norm2.bias,
 *   mlp.fc1.weight (4 w, w), mlp.fc1.bias (4 w), mlp.fc2.weight (w, 4 w), mlp.fc2.bias (w);
 *   and, after the blocks of every stage i < S-1, 3 arrays: downsample.norm.weight (4 w), downsample.norm.bias (4 w),
 *   downsample.reduction.weight (2 w, 4 w).
 * hook_stages: zero-based stage indices, distinct, in the order the hooks fire.  Uploads the weights and allocates the activation arena
 * for up to `max_frames` frames on `device` (synchronous: a planning step).  The arena's size is summed in 64 bits before anything is
 * allocated; when the device cannot hold it the call fails and `i2v_last_error()` names the bytes needed. */
int i2v_swin_create(int device, const i2v_swin_config* cfg, const float* const* weights, int n_weights, const int32_t* hook_stages,
                    int n_hooks, int max_frames, i2v_swin_handle* out);
int i2v_swin_destroy(i2v_swin_handle net);
/* Bytes of device memory the net holds (weights and arena). */
int64_t i2v_swin_workspace_bytes(i2v_swin_handle net);
/* x: (frames, in_chans, img, img), frames <= max_frames.  Runs up to the deepest hooked stage, keeping what the backward needs. */
int i2v_swin_forward(i2v_swin_handle net, const float* x, int frames, void* stream);
/* d(cost)/d(x) of the last forward from the hooks' gradient views (all of them are read): written into gx (accumulate = 0) or added to
 * it (accumulate = 1).  gx: (frames, in_chans, img, img). */
int i2v_swin_backward(i2v_swin_handle net, float* gx, int accumulate, void* stream);
/* Hook `hook`'s activation and gradient views: frame stride (elements) and D contiguous elements per frame -- what
 * `i2v_cossim_fwd_bwd_f32` / `i2v_std_*` of i2v_hip.h read and fill. */
int i2v_swin_hook_info(i2v_swin_handle net, int hook, float** act, int64_t* act_stride, float** grad, int64_t* grad_stride, int64_t* D);
/* Copy hook `hook`'s activation (which = 0) or gradient (which = 1) for `frames` frames into out (frames, D), on `stream`. */
int i2v_swin_read_hook(i2v_swin_handle net, int hook, int which, float* out, int frames, void* stream);

/* ---- the kernels on their own (tests) ----------------------------------------------------------------------------------------
 * Window attention core of one block: qkv (frames, H*W, 3 heads dh) token-major over an H x W grid -> out (frames, H*W, heads dh) in
 * the same layout; the roll by (-shift, -shift), the window partition, the bias, the shift mask (shift != 0), the softmax and the roll
 * back are all inside the one launch.  table: ((2 window - 1)^2, heads).  Served (window, dh): (7, 32) and (4, 16).  The backward takes
 * dout (frames, H*W, heads dh), recomputes the probabilities from qkv and writes dqkv (frames, H*W, 3 heads dh). */
int i2v_swin_window_attention_f32(const float* qkv, int frames, int H, int W, int window, int shift, int heads, int dh, const float* table,
                                  float* out, void* stream);
int i2v_swin_window_attention_bwd_f32(const float* qkv, const float* dout, int frames, int H, int W, int window, int shift, int heads,
                                      int dh, const float* table, float* dqkv, void* stream);
/* Patch merging's gather: x (frames, H, W, C) -> out (frames, H/2, W/2, 4C), and its adjoint: dx (frames, H, W, C) from dout
 * (frames, H/2, W/2, 4C), written (accumulate = 0) or added to what dx holds (accumulate = 1).  A permutation: exact. */
int i2v_swin_merge_f32(const float* x, int frames, int H, int W, int C, float* out, void* stream);
int i2v_swin_merge_bwd_f32(const float* dout, int frames, int H, int W, int C, float* dx, int accumulate, void* stream);
/* Embedding without prefix or position rows: img (frames, in_chans, g*patch, g*patch) -> tokens (frames, g*g, dim) =
 * LayerNorm(patches W^T + b); patches: scratch (frames * g*g, in_chans*patch*patch); emb (frames * g*g, dim), mean and rstd (frames * g*g)
 * are what the backward reads.  Backward: gimg (=, or += with accumulate) from dtokens; patches and demb (frames * g*g, dim) are scratch. */
int i2v_swin_embed_f32(const float* img, int frames, int in_chans, int g, int patch, const float* W, const float* b, const float* norm_w,
                       const float* norm_b, float eps, int dim, float* patches, float* emb, float* mean, float* rstd, float* tokens,
                       void* stream);
int i2v_swin_embed_bwd_f32(const float* dtokens, int frames, int in_chans, int g, int patch, const float* W, const float* norm_w, int dim,
                           const float* emb, const float* mean, const float* rstd, float* demb, float* patches, float* gimg, int accumulate,
                           void* stream);

#ifdef __cplusplus
}
#endif
#endif
