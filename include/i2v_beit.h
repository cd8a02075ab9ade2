/* libi2v_hip.so -- C ABI of the BEiT surrogates (timm 0.5.0's `Beit` at 224 x 224: beit_base_patch16_224 and beit_large_patch16_224),
 * forward to the hooked blocks and backward to the input, run on the transformer stack.  DESIGN.md section 26 states the model.
 *
 * Same conventions as i2v_hip.h, i2v_vit.h, i2v_swin.h, i2v_convnext.h, i2v_mixer.h, i2v_cait.h, i2v_convit.h, i2v_xcit.h and
 * i2v_twins.h: every function returns 0 on success and non-zero on error with the text in `i2v_last_error()`; tensors are caller-owned
 * contiguous fp32 DEVICE pointers; work is enqueued on `stream` (a hipStream_t as void*, 0 = default) and nothing synchronises the host
 * inside a forward or a backward.
 *
 * Model: the patch embedding (a convolution with kernel = stride = `patch`, as patch rows and a Linear) onto a grid of img / patch
 * positions a side, one class token in front: T = 1 + grid^2 tokens, `dim` wide.  NO position embedding.  Then `blocks` pre-norm blocks,
 * LayerNorm eps `ln_eps`, exact GELU, MLP width `mlp`:
 *   x = x + proj(attn(LN1 x))        x = x + fc2(gelu(fc1(LN2 x)))
 * with timm's LayerScale vectors gamma_1 / gamma_2 ALREADY FOLDED into proj and fc2 by the caller, and
 *   attn: qkv = qkv(t) with a bias whose k part is zero; per head of width dim / heads: softmax(q k^T / sqrt(dh) + B_h) v
 * where B_h is the block's relative position bias, given DENSE as (heads, T, T).  A hook is the residual stream after a block, all
 * tokens, the class token included: T * dim floats per frame.
 *
 * Developer switch I2V_BEIT_ATTN=0 (read when the net is planned): the attention core of every block runs on the shared launches instead
 * of the attention launch -- a batched GEMM, the bias-add launch, the row softmax and a second GEMM forward, with the probabilities kept
 * per block (frames * heads * T * (T rounded up to 4) floats, one such array of scratch, and per block the bias padded to that row
 * stride); the softmax backward and four GEMMs backward.  The same definitions in another order of sums: results agree to rounding,
 * not to the bit.
 *
 * ARITHMETIC of the new launches (csrc/i2v_beit.hip; csrc/i2v_beit_host.h restates the definitions, not the order):
 *   - an element of q k^T or dP = dout v^T is ONE fp32 fma chain from 0 over the head index in chunks of 16, inside a chunk in the order
 *     0 4 8 12 1 5 9 13 2 6 10 14 3 7 11 15 (the fp32 MFMA, bitwise an fmaf chain), a chunk past dh filled with zero operands; then
 *     one product with the scale, then one sum with the bias element: S = (q k^T) scale + B;
 *   - a row maximum, softmax denominator and rowsum(dP P): lane group g of 4 takes its keys 16 n + 4 g + i (n = 0, 1, ...; i = 0 .. 3
 *     inside n) in increasing order, then a butterfly over lane distances 16 and 32;  P = exp(S - max) / sum;
 *     dS = scale (P (dP - rowsum));
 *   - an element of out = P v or dq = dS k is one chain from 0 over the key tiles of 16 in increasing order, inside a tile in the order
 *     0 4 8 12 1 5 9 13 2 6 10 14 3 7 11 15 (keys past T are zero operands);
 *   - an element of dk = dS^T q or dv = P^T dout is one chain from 0 over ALL the query tiles of 16 of its frame and head in increasing
 *     order, inside a tile in that same order, in one workgroup: no sum is split across workgroups and there are no atomics, so reruns
 *     repeat the bits, and they depend on neither the frame count nor the frames a net was planned for;
 *   - the bias-add launch adds each element once. */
#ifndef I2V_BEIT_H
#define I2V_BEIT_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct i2v_beit* i2v_beit_handle;

typedef struct {
    int32_t img, patch, in_chans;      /* input side, patch side (a multiple of 4), input channels */
    int32_t dim, heads, mlp, blocks;
    float ln_eps;
} i2v_beit_config;

/* Weights: host fp32 arrays in this order, for the blocks 0 .. B-1 that run, B = deepest hooked block + 1:
 *   patch_embed.proj.weight as (dim, in_chans patch^2) with column (c patch + dy) patch + dx, its bias, cls_token (dim);
 *   per block 13 arrays: norm1.weight, norm1.bias, attn.qkv.weight (3 dim, dim), the qkv bias (3 dim) = [q_bias | 0 | v_bias], the
 *   relative position bias DENSE as (heads, T, T), attn.proj.weight and bias with gamma_1 folded in, norm2.weight, norm2.bias,
 *   mlp.fc1.weight (mlp, dim), bias, mlp.fc2.weight (dim, mlp) and bias with gamma_2 folded in.
 * hook_blocks: zero-based block indices, distinct, in the order the hooks fire.  Uploads the weights and allocates the activation arena
 * for up to `max_frames` frames on `device` (synchronous: a planning step); sized in 64 bits before anything is allocated, and a plan
 * the device cannot hold is refused with the bytes it needs.  Refused as well: a frame that is no whole number of patches; more than
 * 208 tokens; a head width that is no multiple of 4 or over 64; a hook hooked twice or outside the blocks. */
int i2v_beit_create(int device, const i2v_beit_config* cfg, const float* const* weights, int n_weights, const int32_t* hook_blocks,
                    int n_hooks, int max_frames, i2v_beit_handle* out);
int i2v_beit_destroy(i2v_beit_handle net);
/* Bytes of device memory the net holds (weights and arena). */
int64_t i2v_beit_workspace_bytes(i2v_beit_handle net);
/* x: (frames, in_chans, img, img), frames <= max_frames.  Runs up to the deepest hooked block, keeping what the backward needs. */
int i2v_beit_forward(i2v_beit_handle net, const float* x, int frames, void* stream);
/* d(cost)/d(x) of the last forward from the hooks' gradient views (all of them are read): written into gx (accumulate = 0) or added to
 * it (accumulate = 1).  gx: (frames, in_chans, img, img). */
int i2v_beit_backward(i2v_beit_handle net, float* gx, int accumulate, void* stream);
/* D: T * dim. */
int i2v_beit_hook_info(i2v_beit_handle net, int hook, float** act, int64_t* act_stride, float** grad, int64_t* grad_stride, int64_t* D);
/* Copy hook `hook`'s activation (which = 0) or gradient (which = 1) for `frames` frames into out (frames, D), on `stream`. */
int i2v_beit_read_hook(i2v_beit_handle net, int hook, int which, float* out, int frames, void* stream);

/* ---- the kernel on its own (tests, tools) ---------------------------------------------------------------------------------------
 * Biased global attention.  qkv: (frames, T, 3 heads dh), q of head h at column h dh, k at heads dh + h dh, v at 2 heads dh + h dh;
 * bias: (heads, T, T) with row stride T, or null for plain attention; out, dout: (frames, T, heads dh); dqkv as qkv.  The forward is
 * one launch (a workgroup of 4 waves owns one (frame, head) and stages the head's whole K and V in LDS once; scores, bias, softmax and
 * P v stay in registers); the backward is two -- dq with the same ownership, then dk and dv by one workgroup per (frame, head) that
 * walks the queries in increasing order -- and recomputes the probabilities; no gradient is formed for the bias.  Refused with
 * hipErrorInvalidValue and the reason, nothing launched: T over 208; dh no multiple of 4 or over 64; more than 65 535 frames or heads;
 * more than 2^31 elements; null or misaligned (16 bytes) arrays, a null `bias` alone allowed.  Exported by every build of the C ABI:
 * where the library has no device kernel (the host simulation) the same definitions run as scalar host code. */
int i2v_beit_attention_f32(const float* qkv, const float* bias, int frames, int T, int heads, int dh, float scale, float* out, void* stream);
int i2v_beit_attention_bwd_f32(const float* qkv, const float* bias, const float* dout, int frames, int T, int heads, int dh, float scale,
                               float* dqkv, void* stream);
/* The bias-add launch of the shared-launch route on its own: S (frames, per_frame) += bias (per_frame), every element once; per_frame
 * is heads * T * ld with ld a multiple of 4.  Refused: null or misaligned (16 bytes) arrays, per_frame no positive multiple of 4. */
int i2v_beit_bias_add_f32(float* S, const float* bias, int frames, int64_t per_frame, void* stream);

#ifdef __cplusplus
}
#endif
#endif
