/* libi2v_hip.so -- C ABI of the PiT surrogates (timm 0.5.0's `PoolingVisionTransformer` at 224 x 224: pit_ti / pit_xs / pit_s / pit_b
 * and their _distilled twins), forward to the hooked blocks and backward to the input, run on the transformer stack.  DESIGN.md section
 * 29 states the model.
 *
 * Same conventions as i2v_hip.h, i2v_vit.h and the other family headers: every function returns 0 on success and non-zero on error with
 * the text in `i2v_last_error()`; tensors are caller-owned contiguous fp32 DEVICE pointers; work is enqueued on `stream` (a hipStream_t
 * as void*, 0 = default) and nothing synchronises the host inside a forward or a backward.
 *
 * Model: the patch embedding is a convolution with kernel `patch` and stride `stride` < patch (overlapping patches, as patch rows and a
 * Linear) onto a grid of g0 = (img - patch) / stride + 1 positions a side; a spatial position table is added to the grid tokens only and
 * `prefix` tokens (1, or 2 for a distilled net) come in front: T0 = prefix + g0^2 tokens, dims[0] wide.  Then three stages of pre-norm
 * blocks, LayerNorm eps `ln_eps`, exact GELU, MLP width 4 x the stage's width:
 *   x = x + proj(attn(LN1 x))        x = x + fc2(gelu(fc1(LN2 x)))         attn: softmax(q k^T / sqrt(dh)) v per head
 * Between the stages the grid tokens pass a depthwise convolution (kernel 3, stride 2, padding 1, two output channels per input channel)
 * onto a grid of (g - 1) / 2 + 1, and the prefix tokens a Linear to twice the width.  A hook is the residual stream after a block, all
 * tokens, the prefix tokens included, BEFORE any pooling: tokens * width floats per frame.  Blocks are numbered flat across the stages.
 *
 * Developer switch I2V_PIT_ATTN=0 (read when the net is planned): the attention core of every block runs on the shared launches -- a
 * batched GEMM, the row softmax and a second GEMM forward, with the probabilities kept per block (frames * heads * T * (T rounded up to
 * 4) floats and one such array of scratch); the softmax backward and four GEMMs backward.  The same definitions in another order of
 * sums: results agree to rounding, not to the bit.  Without it a block keeps the attention output and the row log-sum-exp instead,
 * frames * T * (width + heads) floats.
 *
 * ARITHMETIC of the new launches (csrc/i2v_pit.hip; csrc/i2v_pit_host.h restates the definitions, not the attention's order):
 *   - an element of q k^T or dP = dout v^T is ONE fp32 fma chain from 0 over the head index in chunks of 16, inside a chunk in the order
 *     0 4 8 12 1 5 9 13 2 6 10 14 3 7 11 15 (the fp32 MFMA, bitwise an fmaf chain), a chunk past dh filled with zero operands; then one
 *     product with the scale; delta = rowsum(dout o out) is one chain in that same order;
 *   - the keys pass in tiles of 64 in increasing order.  Per tile: the tile maximum and the sum of p = exp(s - m') -- lane group g of 4
 *     takes its keys 16 n + 4 g + i (n = 0 .. 3; i = 0 .. 3 inside n) in increasing order, then a butterfly over lane distances 16 and 32
 *     -- then m' = max(m, tile maximum), alpha = exp(m - m'), l = l alpha + sum, out = out alpha + p v.  out is rescaled in every tile
 *     (alpha is exactly 1 where the maximum has not moved); there is no threshold.  At the end out = out / l, lse = m + log(l);
 *   - backward: P = exp(s - lse) from the forward's lse, dS = scale (P (dP - delta)): no row reduction;
 *   - inside a tile an element of p v, dS k, P^T dout or dS^T q adds the tile's 64 rows to its running fp32 accumulator in the order
 *     16 n + {0 4 8 12 1 5 9 13 2 6 10 14 3 7 11 15}, n increasing (rows past T are zero operands); an element of out or dq walks the key
 *     tiles, an element of dk or dv ALL the query tiles of its frame and head, in increasing order, in one workgroup: no sum is split
 *     across workgroups and there are no atomics, so reruns repeat the bits, and they depend on neither the frame count nor the frames a
 *     net was planned for;
 *   - the pool adds its taps (ky, kx) in increasing order onto the bias, a tap on the padding taking no part; its input gradient sums,
 *     from 0, over (ky, kx) in increasing order and inside a tap over the two output channels 2 c, 2 c + 1;
 *   - the patch gather copies; the scatter sums a pixel's patches from 0 in increasing (row, column) order of the patch grid. */
#ifndef I2V_PIT_H
#define I2V_PIT_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct i2v_pit* i2v_pit_handle;

#define I2V_PIT_STAGES 3

typedef struct {
    int32_t img, patch, stride, in_chans, prefix;      /* input side, patch side, patch stride, input channels, prefix tokens (1 or 2) */
    int32_t dims[I2V_PIT_STAGES], heads[I2V_PIT_STAGES], depths[I2V_PIT_STAGES];
    float ln_eps;
} i2v_pit_config;

/* Weights: host fp32 arrays in this order, for the blocks 0 .. B-1 that run (flat across the stages), B = deepest hooked block + 1:
 *   patch_embed.conv.weight as (dims[0], in_chans patch^2) with column (c patch + dy) patch + dx, its bias, the position table TOKEN-MAJOR
 *   as (prefix + g0^2, dims[0]) with `prefix` rows of zeros in front, cls_token (prefix, dims[0]);
 *   then stage by stage: per block 12 arrays -- norm1.weight, norm1.bias, attn.qkv.weight (3 D, D), bias, attn.proj.weight, bias,
 *   norm2.weight, norm2.bias, mlp.fc1.weight (4 D, D), bias, mlp.fc2.weight (D, 4 D), bias -- and, behind a stage whose successor runs at
 *   least one block, 4 arrays: pool.conv.weight (2 D, 9), pool.conv.bias (2 D), pool.fc.weight (2 D, D), pool.fc.bias (2 D).
 * hook_blocks: zero-based flat block indices, distinct, in the order the hooks fire.  Uploads the weights and allocates the activation
 * arena for up to `max_frames` frames on `device` (synchronous: a planning step); sized in 64 bits before anything is allocated, and a
 * plan the device cannot hold is refused with the bytes it needs.  Refused as well: patches that do not tile the frame at the stride; a
 * width that is not twice its predecessor's; a head width that is no multiple of 4 or over 64; a hook hooked twice or outside the
 * blocks. */
int i2v_pit_create(int device, const i2v_pit_config* cfg, const float* const* weights, int n_weights, const int32_t* hook_blocks, int n_hooks,
                   int max_frames, i2v_pit_handle* out);
int i2v_pit_destroy(i2v_pit_handle net);
/* Bytes of device memory the net holds (weights and arena). */
int64_t i2v_pit_workspace_bytes(i2v_pit_handle net);
/* x: (frames, in_chans, img, img), frames <= max_frames.  Runs up to the deepest hooked block, keeping what the backward needs. */
int i2v_pit_forward(i2v_pit_handle net, const float* x, int frames, void* stream);
/* d(cost)/d(x) of the last forward from the hooks' gradient views (all of them are read): written into gx (accumulate = 0) or added to
 * it (accumulate = 1).  gx: (frames, in_chans, img, img). */
int i2v_pit_backward(i2v_pit_handle net, float* gx, int accumulate, void* stream);
/* D: tokens * width of the hooked block's stage. */
int i2v_pit_hook_info(i2v_pit_handle net, int hook, float** act, int64_t* act_stride, float** grad, int64_t* grad_stride, int64_t* D);
/* Copy hook `hook`'s activation (which = 0) or gradient (which = 1) for `frames` frames into out (frames, D), on `stream`. */
int i2v_pit_read_hook(i2v_pit_handle net, int hook, int which, float* out, int frames, void* stream);

/* ---- the kernels on their own (tests, tools) --------------------------------------------------------------------------------------
 * Exported by every build of the C ABI: where the library has no device kernel (the host simulation) the same definitions run as scalar
 * host code.  Each refuses with hipErrorInvalidValue and the reason, nothing launched.
 *
 * Streaming attention.  qkv: (frames, T, 3 heads dh), q of head h at column h dh, k at heads dh + h dh, v at 2 heads dh + h dh; out,
 * dout: (frames, T, heads dh); lse, delta: (frames, heads, T); dqkv as qkv.  T is unbounded.  The forward is one launch (a workgroup of
 * 4 waves owns one (frame, head, tile of 64 queries) and streams K and V through LDS in tiles of 64 keys under an online softmax) and
 * writes out and lse.  The backward reads out and lse, fills the scratch delta, and is three launches: delta; dq per query tile streaming
 * the keys; dk and dv per KEY tile streaming the queries in increasing order.  Refused: dh no multiple of 4 or over 64; more than 65 535
 * frames, heads or token tiles; more than 2^31 elements; null or misaligned (16 bytes) arrays. */
int i2v_pit_attention_f32(const float* qkv, int frames, int T, int heads, int dh, float scale, float* out, float* lse, void* stream);
int i2v_pit_attention_bwd_f32(const float* qkv, const float* out, const float* lse, const float* dout, int frames, int T, int heads, int dh,
                              float scale, float* delta, float* dqkv, void* stream);
/* The pooling convolution on token-major streams.  x: frames of T_in = prefix + g^2 rows of C floats; y: frames of prefix + go^2 rows of
 * 2 C floats, go = (g - 1) / 2 + 1; the `prefix` rows in front of every frame are skipped in both and left untouched.  w: (2 C, 9), b:
 * (2 C) or null.  The backward takes dy laid out as y and writes dx laid out as x (accumulate = 0) or adds to it (accumulate = 1). */
int i2v_pit_pool_f32(const float* x, const float* w, const float* b, int frames, int g, int C, int prefix, float* y, void* stream);
int i2v_pit_pool_bwd_f32(const float* dy, const float* w, int frames, int g, int C, int prefix, int accumulate, float* dx, void* stream);
/* Overlapping patches.  img: (frames, in_chans, side, side); rows: (frames g^2, in_chans p^2), g = (side - p) / s + 1, in vit_patchify's
 * column order.  The scatter is the gather's transpose (a pixel sums its at most (p / s)^2 patches), written or added to gimg. */
int i2v_pit_patch_gather_f32(const float* img, int frames, int in_chans, int side, int p, int s, float* rows, void* stream);
int i2v_pit_patch_scatter_f32(const float* rows, int frames, int in_chans, int side, int p, int s, int accumulate, float* gimg, void* stream);

#ifdef __cplusplus
}
#endif
#endif
