/* libi2v_hip.so -- C ABI of the ConvNeXt surrogates (timm's `ConvNeXt` at 224 x 224: convnext_{tiny,small,base,large}), forward to the
 * hooked stages and backward to the input, run on the transformer stack.  DESIGN.md section 18 states the model.
 *
 * Same conventions as i2v_hip.h, i2v_vit.h and i2v_swin.h: every function returns 0 on success and non-zero on error with the text in
 * `i2v_last_error()`; tensors are caller-owned contiguous fp32 DEVICE pointers; work is enqueued on `stream` (a hipStream_t as void*,
 * 0 = default) and nothing synchronises the host inside a forward or a backward.
 *
 * Model: the stem is a patch x patch convolution with stride patch and bias (in_chans -> dim) and a LayerNorm over channels -- the Swin
 * patch embedding.  Stage i (0-based) is `depths[i]` blocks at width dim * 2^i on a plane of (img / patch) / 2^i squared; in front of
 * every stage but the first sits a downsample: LayerNorm over channels per position, then a 2 x 2 convolution with stride 2 and bias,
 * run as the 2 x 2 neighbour gather of i2v_swin.h (quarters in the order (0,0), (1,0), (0,1), (1,1) as (row, column) offsets) and a
 * Linear 4 w -> 2 w.  A block is
 *   x = x + gamma * fc2(GELU(fc1(LN(dwconv7x7(x)))))         (depthwise, pad 3, bias; MLP width 4 x the stage's width, exact erf GELU)
 * with LN, fc1, GELU and fc2 acting per position over channels.  Activations are TOKEN-MAJOR: a frame is (plane^2, width) row-major,
 * i.e. (row, column, channel) with channels contiguous.
 *
 * A hook is the output of the last block of a stage, BEFORE the next stage's downsample: D = plane_i^2 * width_i floats per frame. */
#ifndef I2V_CONVNEXT_H
#define I2V_CONVNEXT_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct i2v_convnext* i2v_convnext_handle;

#define I2V_CONVNEXT_MAX_STAGES 4

typedef struct {
    int32_t img, patch, in_chans, dim, stages;                  /* input side, stem patch side, input channels, stage-0 width, stages */
    int32_t depths[I2V_CONVNEXT_MAX_STAGES];                    /* blocks per stage */
    float ln_eps;
} i2v_convnext_config;

/* Weights: host fp32 arrays in this order, for the stages 0 .. S-1 that run, S = deepest hooked stage + 1:
 *   stem.0.weight (dim, in_chans, patch, patch), stem.0.bias (dim), stem.1.weight (dim), stem.1.bias (dim);
 *   then per stage i: for i >= 1 the 4 arrays of its downsample -- downsample.0.weight (w/2), downsample.0.bias (w/2), the Linear's
 *   weight (w, 2 w): L[o][q * (w/2) + c] = downsample.1.weight[o][c][q & 1][q >> 1] (q = 2 * column offset + row offset: the gather's
 *   quarter order), downsample.1.bias (w) -- and per block j 8 arrays: conv_dw.weight TRANSPOSED to (49, w) -- tap a * 7 + b of channel
 *   c at [a * 7 + b][c] --, conv_dw.bias (w), norm.weight (w), norm.bias (w), mlp.fc1.weight (4 w, w), mlp.fc1.bias (4 w), and
 *   mlp.fc2.weight (w, 4 w) and mlp.fc2.bias (w) each with `gamma` already multiplied in (row o of the weight and element o of the bias
 *   times gamma[o]): the layer scale costs nothing at run time.
 * hook_stages: zero-based stage indices, distinct, in the order the hooks fire.  Uploads the weights and allocates the activation arena
 * for up to `max_frames` frames on `device` (synchronous: a planning step); sized in 64 bits before anything is allocated. */
int i2v_convnext_create(int device, const i2v_convnext_config* cfg, const float* const* weights, int n_weights, const int32_t* hook_stages,
                        int n_hooks, int max_frames, i2v_convnext_handle* out);
int i2v_convnext_destroy(i2v_convnext_handle net);
/* Bytes of device memory the net holds (weights and arena). */
int64_t i2v_convnext_workspace_bytes(i2v_convnext_handle net);
/* x: (frames, in_chans, img, img), frames <= max_frames.  Runs up to the deepest hooked stage, keeping what the backward needs. */
int i2v_convnext_forward(i2v_convnext_handle net, const float* x, int frames, void* stream);
/* d(cost)/d(x) of the last forward from the hooks' gradient views (all of them are read): written into gx (accumulate = 0) or added to
 * it (accumulate = 1).  gx: (frames, in_chans, img, img). */
int i2v_convnext_backward(i2v_convnext_handle net, float* gx, int accumulate, void* stream);
int i2v_convnext_hook_info(i2v_convnext_handle net, int hook, float** act, int64_t* act_stride, float** grad, int64_t* grad_stride, int64_t* D);
/* Copy hook `hook`'s activation (which = 0) or gradient (which = 1) for `frames` frames into out (frames, D), on `stream`. */
int i2v_convnext_read_hook(i2v_convnext_handle net, int hook, int which, float* out, int frames, void* stream);

/* ---- the kernel on its own (tests, tools) --------------------------------------------------------------------------------------
 * Token-major depthwise 7 x 7 convolution, pad 3: x, y and the optional `add` are (frames, H, W, C), filter (49, C), optional bias (C):
 *   y[n][h][w][c] = (sum_{a,b} filter[a * 7 + b][c] * x[n][h + a - 3][w + b - 3][c]) + bias[c] + add[n][h][w][c]
 * Each output is one fp32 fma chain from 0 over the taps in row-major order, then + bias, then + add.  The input gradient of the layer is
 * this call on the output's gradient with the mirrored filter (row t -> row 48 - t) and no bias.  Exported by every build of the C ABI:
 * where the library has no device kernel (the host simulation) the same operations run as scalar host code in the same order. */
int i2v_convnext_dw_f32(const float* x, const float* filter, const float* bias, const float* add, float* y, int frames, int H, int W,
                        int C, void* stream);

#ifdef __cplusplus
}
#endif
#endif
