/* libi2v_hip.so -- C ABI of the Twins surrogates (timm 0.5.0's `Twins` at 224 x 224: twins_pcpvt_small / base / large and twins_svt_small /
 * base / large), forward to the hooked stages and backward to the input, run on the transformer stack.  DESIGN.md section 25 states the
 * model.
 *
 * Same conventions as i2v_hip.h, i2v_vit.h, i2v_swin.h, i2v_convnext.h, i2v_mixer.h, i2v_cait.h, i2v_convit.h and i2v_xcit.h: every
 * function returns 0 on success and non-zero on error with the text in `i2v_last_error()`; tensors are caller-owned contiguous fp32
 * DEVICE pointers; work is enqueued on `stream` (a hipStream_t as void*, 0 = default) and nothing synchronises the host inside a
 * forward or a backward.
 *
 * Model: `stages` stages (1 .. 4).  Stage k opens with a patch embedding -- a convolution with kernel = stride = `patch` (stage 0) or 2
 * (later stages), as a gather and a Linear, then LayerNorm eps `pe_eps` -- onto a grid of (img / patch) >> k positions a side, width
 * dims[k], token = y * grid + x.  Then depths[k] pre-norm blocks, LayerNorm eps `ln_eps`, exact GELU, MLP width mlp[k]:
 *   x = x + proj(attn(LN1 x))        x = x + fc2(gelu(fc1(LN2 x)))
 * and, after block 0 of the stage, the conditional position encoding  x = x + dw3x3(x) + bias  (depthwise, pad 1, on the grid).
 * attn of block j is global sub-sampled attention (GSA) where `window` is 0 or j is odd, else locally-grouped attention (LSA):
 *   GSA  q = q(t);  u = t where sr[k] is 1, else LN(sr(t)) with sr a convolution of kernel = stride = sr[k] (a block gather and a
 *        Linear) and LayerNorm eps `pe_eps`;  (k, v) = kv(u);  per head of width dims[k] / heads[k]:
 *        softmax(q k^T / sqrt(dh)) v -- grid^2 queries against (grid / sr[k])^2 keys
 *   LSA  attention inside window x window windows of the grid, no shift, no bias: qkv(t), softmax(q k^T / sqrt(dh)) v per window
 * A hook is the stream after the last block of a stage, before the next patch embedding: grid^2 * dims[k] floats per frame.
 *
 * Developer switch I2V_TWINS_ATTN=0 (read when the net is planned): the core of every GSA block runs on the shared launches instead of
 * the attention launch -- a batched GEMM, the row softmax and a second GEMM forward, with the probabilities kept per block
 * (frames * heads * queries * (keys rounded up to 4) floats, and one such array of scratch); the softmax backward and four GEMMs
 * backward.  The same definitions in another order of sums: results agree to rounding, not to the bit.
 *
 * ARITHMETIC of the new launches (csrc/i2v_twins.hip; csrc/i2v_twins_host.h restates the definitions, not the order):
 *   - an element of S = q k^T or dP = dout v^T is ONE fp32 fma chain from 0 over the head index in chunks of 16, inside a chunk in the
 *     order 0 4 8 12 1 5 9 13 2 6 10 14 3 7 11 15 (the fp32 MFMA, bitwise an fmaf chain), a chunk past dh filled with zero operands;
 *     then one product with the scale;
 *   - a row maximum, softmax denominator and rowsum(dP P): lane r of 16 adds its keys r, r + 16, r + 32, r + 48 in increasing order,
 *     then a butterfly over lane distances 8 .. 1;  P = exp(S - max) / sum;  dS = scale (P (dP - rowsum));
 *   - an element of out = P v or dq = dS k is one chain from 0 over the keys in increasing order (keys past Tk are zero operands);
 *   - an element of dk = dS^T q or dv = P^T dout is one chain from 0 over ALL the queries of its frame and head in increasing order, in
 *     one workgroup: no sum is split across workgroups and there are no atomics, so reruns repeat the bits, and they depend on neither
 *     the frame count nor the frames a net was planned for;
 *   - the block gather and its scatter are copies; a scatter with `accumulate` adds each element once. */
#ifndef I2V_TWINS_H
#define I2V_TWINS_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define I2V_TWINS_MAX_STAGES 4

typedef struct i2v_twins* i2v_twins_handle;

typedef struct {
    int32_t img, in_chans, patch, stages;      /* input side, input channels, stage 0's patch (a multiple of 4), stages */
    int32_t window;                            /* 0: every block GSA; 7 (head width 32) or 4 (head width 16): even blocks LSA */
    int32_t dims[I2V_TWINS_MAX_STAGES], heads[I2V_TWINS_MAX_STAGES], mlp[I2V_TWINS_MAX_STAGES], depths[I2V_TWINS_MAX_STAGES],
            sr[I2V_TWINS_MAX_STAGES];          /* sr: 1, 2, 4 or 8 */
    float ln_eps, pe_eps;                      /* the blocks' LayerNorms; the patch embeddings' and the sub-sampling's */
} i2v_twins_config;

/* Weights: host fp32 arrays in this order, for the stages 0 .. S-1 that run, S = deepest hooked stage + 1.  Per stage:
 *   the patch embedding as a Linear (dims[k], K) and its bias, norm weight and bias: stage 0 K = in_chans patch^2 with column
 *   (c patch + dy) patch + dx; later stages K = 4 dims[k-1] with column (dy + 2 dx) dims[k-1] + c (the 2 x 2 merge gather's order);
 *   per block: norm1.weight, norm1.bias; then for LSA attn.qkv.weight (3 D, D) and bias, for GSA attn.q.weight (D, D) and bias,
 *   attn.kv.weight (2 D, D) and bias and, where sr > 1, attn.sr as a Linear (D, sr^2 D) with column (dy sr + dx) D + c, its bias,
 *   attn.norm.weight and bias; then attn.proj.weight, bias, norm2.weight, bias, mlp.fc1.weight (mlp, D), bias, mlp.fc2.weight (D, mlp),
 *   bias; behind block 0's arrays the position encoding's filter as (9, D) with tap = 3 ky + kx, and its bias.
 * hook_stages: zero-based stage indices, distinct, in the order the hooks fire.  Uploads the weights and allocates the activation
 * arena for up to `max_frames` frames on `device` (synchronous: a planning step); sized in 64 bits before anything is allocated, and a
 * plan the device cannot hold is refused with the bytes it needs.  Refused as well: a grid that is not whole under the patch, the 2 x 2
 * embeddings, sr or the window; more than 64 keys; a head width that is no multiple of 4 or over 64, or is not the window's; a hook
 * hooked twice or outside the stages. */
int i2v_twins_create(int device, const i2v_twins_config* cfg, const float* const* weights, int n_weights, const int32_t* hook_stages,
                     int n_hooks, int max_frames, i2v_twins_handle* out);
int i2v_twins_destroy(i2v_twins_handle net);
/* Bytes of device memory the net holds (weights and arena). */
int64_t i2v_twins_workspace_bytes(i2v_twins_handle net);
/* x: (frames, in_chans, img, img), frames <= max_frames.  Runs up to the deepest hooked stage, keeping what the backward needs. */
int i2v_twins_forward(i2v_twins_handle net, const float* x, int frames, void* stream);
/* d(cost)/d(x) of the last forward from the hooks' gradient views (all of them are read): written into gx (accumulate = 0) or added to
 * it (accumulate = 1).  gx: (frames, in_chans, img, img). */
int i2v_twins_backward(i2v_twins_handle net, float* gx, int accumulate, void* stream);
/* D: grid^2 * dims of the hooked stage. */
int i2v_twins_hook_info(i2v_twins_handle net, int hook, float** act, int64_t* act_stride, float** grad, int64_t* grad_stride, int64_t* D);
/* Copy hook `hook`'s activation (which = 0) or gradient (which = 1) for `frames` frames into out (frames, D), on `stream`. */
int i2v_twins_read_hook(i2v_twins_handle net, int hook, int which, float* out, int frames, void* stream);

/* ---- the kernels on their own (tests, tools) -----------------------------------------------------------------------------------
 * Sub-sampled attention.  q: (frames, Tq, heads dh); kv: (frames, Tk, 2 heads dh), k of head h at column h dh and v at heads dh + h dh;
 * out, dout, dq as q; dkv as kv.  The forward is one launch (a workgroup owns one (frame, head, tile of 256 queries) and stages the
 * head's whole K and V in LDS once); the backward is two -- dq by query tile, then dk and dv by one workgroup per (frame, head) that
 * walks the queries in increasing order -- and recomputes the probabilities.  Tq is not bounded.  Refused with hipErrorInvalidValue and
 * the reason: Tk over 64; dh no multiple of 4 or over 64; more than 2^31 elements; more than 65 535 frames or heads; null or misaligned
 * (16 bytes) arrays.  Exported by every build of the C ABI: where the library has no device kernel (the host simulation) the same
 * definitions run as scalar host code. */
int i2v_twins_attention_f32(const float* q, const float* kv, int frames, int Tq, int Tk, int heads, int dh, float scale, float* out,
                            void* stream);
int i2v_twins_attention_bwd_f32(const float* q, const float* kv, const float* dout, int frames, int Tq, int Tk, int heads, int dh, float scale,
                                float* dq, float* dkv, void* stream);
/* The s x s block gather, s = 2, 4 or 8: x (frames, H, W, C) -> rows (frames H/s W/s, s s C) with column (dy s + dx) C + c; and its
 * inverse, which writes dx or, with `accumulate`, adds to it.  Refused: another s, a plane that is no whole number of blocks, C no
 * multiple of 4, more than 2^31 elements, null, misaligned or identical arrays. */
int i2v_twins_block_gather_f32(const float* x, float* rows, int frames, int H, int W, int C, int s, void* stream);
int i2v_twins_block_scatter_f32(const float* drows, float* dx, int frames, int H, int W, int C, int s, int accumulate, void* stream);
/* Window attention at shift 0 without a bias table on qkv (frames, H W, 3 heads dh), as `i2v_swin_window_attention_f32` lays it out;
 * window 7 with dh 32 or window 4 with dh 16.  The device build runs the Swin launch, which requires a table: `zero_table` is
 * (2 window - 1)^2 * heads zeros.  The host simulation runs scalar code and does not read it. */
int i2v_twins_window_attention_f32(const float* qkv, int frames, int H, int W, int window, int heads, int dh, const float* zero_table,
                                   float* out, void* stream);
int i2v_twins_window_attention_bwd_f32(const float* qkv, const float* dout, int frames, int H, int W, int window, int heads, int dh,
                                       const float* zero_table, float* dqkv, void* stream);

#ifdef __cplusplus
}
#endif
#endif
