/* libi2v_hip.so -- C ABI of the ConViT surrogates (timm 0.5.0's `ConViT` at 224 x 224: convit_tiny, convit_small, convit_base), forward to
 * the hooked blocks and backward to the input, run on the transformer stack.  DESIGN.md section 22 states the model.
 *
 * Same conventions as i2v_hip.h, i2v_vit.h, i2v_swin.h, i2v_convnext.h, i2v_mixer.h and i2v_cait.h: every function returns 0 on success and
 * non-zero on error with the text in `i2v_last_error()`; tensors are caller-owned contiguous fp32 DEVICE pointers; work is enqueued on
 * `stream` (a hipStream_t as void*, 0 = default) and nothing synchronises the host inside a forward or a backward.
 *
 * Model: the stem is a patch x patch convolution with stride patch and bias (in_chans -> dim), then + pos_embed (T, dim): T = (img /
 * patch)^2 tokens and no prefix token yet.  Then `blocks` pre-norm blocks, LayerNorm eps `ln_eps`, exact erf GELU:
 *   x = x + proj(attn(LN1 x))        x = x + fc2(gelu(fc1(LN2 x)))
 * Blocks 0 .. local_blocks - 1 use gated positional self-attention (GPSA) over H heads of width dh = dim / H, scale = dh^-0.5:
 *   S_h = (scale q_h) k_h^T | Ppatch_h = softmax over keys of S_h | Ppos_h[i][j] = softmax over j of (w_h . r_ij + b_h),
 *   r_ij = (jx - ix, jy - iy, (jx - ix)^2 + (jy - iy)^2), token = y * grid + x |
 *   P_h = (1 - sigma(g_h)) Ppatch_h + sigma(g_h) Ppos_h | P_h /= sum_j P_h | O_h = P_h v_h
 * Before block `local_blocks` the stream becomes [cls_token; x], T + 1 tokens, and the remaining blocks use plain softmax attention.
 * A hook is the residual stream after a block, all tokens: T * dim floats per frame before the join, (T + 1) * dim after it.
 *
 * WHAT THE CALLER FOLDS (ConvitSpec.native_arrays, in float64 at load time).  Ppos depends on the weights only, and pos_proj.bias
 * cancels inside its softmax.  A row of the blend sums to (1 - sigma) + sigma = 1 whatever S is, so timm's final division is a division by
 * 1 +- rounding and its derivative with respect to S is identically zero.  The library therefore takes, per GPSA block, the table
 * A_h = sigma(g_h) Ppos_h as (H, T, ld) with rows padded to ld = i2v_vit_probs_ld(T), and c_h = 1 - sigma(g_h) as (H); the launch computes
 * P = fma(c_h, Ppatch_h, A_h) and neither divides nor differentiates a division.  attn.qk.weight and attn.v.weight arrive stacked as one
 * (3 dim, dim) array, whose columns then lie as `i2v_vit_attention_f32` expects them, with a zero qkv bias.
 *
 * ARITHMETIC of the attention launches (csrc/i2v_convit.hip; csrc/i2v_convit_host.h restates the definitions, not the order):
 *   - every product element is ONE fp32 fma chain from 0 (the fp32 MFMA, bitwise an fmaf chain).  Over the head width (q k^T, dout v^T)
 *     and over the keys (P v, dS k) the contracted index goes in chunks of 16, inside a chunk in the order 0 4 8 12 1 5 9 13 2 6 10 14 3 7
 *     11 15, a chunk past the end filled with zero operands; over the query rows (dk, dv) in increasing order;
 *   - a row sum (the softmax denominator; sum_j c dP Ppatch): lane l of 64 adds keys l, l + 64, ... in increasing order, then a butterfly
 *     over lane distances 32 .. 1; Ppatch = exp(S - max) * (1 / sum);
 *   - the blend is one fma(c, Ppatch, A) per element, forward and where the backward re-forms P; c dP is one rounded product taken
 *     before the row sum; dS = Ppatch * (c dP - sum);
 *   - q is multiplied by scale as it is loaded; dq and dk are scale * the finished chain;
 *   - no sum is split across workgroups and there are no atomics: reruns repeat the bits, and they depend on neither the frame count nor
 *     the frames a net was planned for. */
#ifndef I2V_CONVIT_H
#define I2V_CONVIT_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct i2v_convit* i2v_convit_handle;

typedef struct {
    int32_t img, patch, in_chans, dim, heads, mlp, blocks;      /* input side, patch side, input channels, width, heads, MLP width, blocks */
    int32_t local_blocks;                                        /* GPSA blocks: the class token joins before block `local_blocks` (1 .. blocks) */
    float ln_eps;
} i2v_convit_config;

/* Weights: host fp32 arrays in this order, for the blocks 0 .. B-1 that run, B = deepest hooked block + 1:
 *   patch_embed.proj.weight (dim, in_chans, patch, patch), patch_embed.proj.bias (dim), pos_embed (T, dim), cls_token (dim);
 *   per block below `local_blocks` 14 arrays: norm1.weight, norm1.bias (dim), [attn.qk.weight; attn.v.weight] (3 dim, dim), a zero qkv bias
 *   (3 dim), c (H), the table A (H, T, ld), attn.proj.weight (dim, dim), attn.proj.bias, norm2.weight, norm2.bias, mlp.fc1.weight (mlp, dim),
 *   mlp.fc1.bias, mlp.fc2.weight (dim, mlp), mlp.fc2.bias;
 *   per block from `local_blocks` on 12 arrays: the same with attn.qkv.weight as it lies and without c and A.
 * hook_blocks: zero-based block indices, distinct, in the order the hooks fire.  Uploads the weights and allocates the activation arena
 * for up to `max_frames` frames on `device` (synchronous: a planning step); sized in 64 bits before anything is allocated, and a plan the
 * device cannot hold is refused with the bytes it needs.  Refused as well: dim / heads no multiple of 4, local_blocks outside 1 .. blocks,
 * and more keys than one workgroup's LDS holds (16 * (T + 1 rounded up to 16, plus 4) floats within 160 KiB). */
int i2v_convit_create(int device, const i2v_convit_config* cfg, const float* const* weights, int n_weights, const int32_t* hook_blocks,
                      int n_hooks, int max_frames, i2v_convit_handle* out);
int i2v_convit_destroy(i2v_convit_handle net);
/* Bytes of device memory the net holds (weights and arena). */
int64_t i2v_convit_workspace_bytes(i2v_convit_handle net);
/* x: (frames, in_chans, img, img), frames <= max_frames.  Runs up to the deepest hooked block, keeping what the backward needs. */
int i2v_convit_forward(i2v_convit_handle net, const float* x, int frames, void* stream);
/* d(cost)/d(x) of the last forward from the hooks' gradient views (all of them are read): written into gx (accumulate = 0) or added to
 * it (accumulate = 1).  gx: (frames, in_chans, img, img).  The class token is a weight and gets no gradient. */
int i2v_convit_backward(i2v_convit_handle net, float* gx, int accumulate, void* stream);
/* D: T * dim for a hook before the join, (T + 1) * dim behind it. */
int i2v_convit_hook_info(i2v_convit_handle net, int hook, float** act, int64_t* act_stride, float** grad, int64_t* grad_stride, int64_t* D);
/* Copy hook `hook`'s activation (which = 0) or gradient (which = 1) for `frames` frames into out (frames, D), on `stream`. */
int i2v_convit_read_hook(i2v_convit_handle net, int hook, int which, float* out, int frames, void* stream);

/* ---- the kernel on its own (tests, tools) --------------------------------------------------------------------------------------
 * qkv: (frames, T, 3 heads dh) as `i2v_vit_attention_f32` takes it (q of head h at column h dh, k at heads dh + h dh, v at 2 heads dh +
 * h dh); c: (heads); table: (heads, T, ld) with ld = i2v_vit_probs_ld(T), any non-negative values (not only a square grid's); both null:
 * plain softmax attention.  probs: (frames, heads, T, ld), written by the forward entry: Ppatch, the softmax before the blend; out:
 * (frames, T, heads dh) = fma(c, Ppatch, table) v.  The backward entry reads qkv, probs and dout (frames, T, heads dh) and writes dqkv
 * (frames, T, 3 heads dh); ds_scratch is an array of probs' size it may overwrite.  All arrays 16-byte aligned.  Refused with
 * hipErrorInvalidValue and the reason: dh no multiple of 4; a table without c or c without a table; more keys than the LDS budget holds;
 * more than 2^31 elements; more than 65 535 frames, heads or tiles of 16 tokens; null or misaligned arrays.  Exported by every build of
 * the C ABI: where the library has no device kernel (the host simulation) the same definitions run as scalar host code. */
int i2v_convit_attention_f32(const float* qkv, int frames, int T, int heads, int dh, float scale, const float* c, const float* table,
                             float* probs, float* out, void* stream);
int i2v_convit_attention_bwd_f32(const float* qkv, const float* probs, const float* dout, int frames, int T, int heads, int dh, float scale,
                                 const float* c, const float* table, float* ds_scratch, float* dqkv, void* stream);
/* The two launches that let the class token join the stream: out (frames, T + 1, C) = [cls (C); x (frames, T, C)] per frame, a copy; and
 * its gradient dx (frames, T, C) = rows 1 .. T of dout (frames, T + 1, C), plus add (frames, T, C) where add is not null (one rounded add
 * per element).  Refused with hipErrorInvalidValue: a null array (but add), frames, T or C not positive, C no multiple of
 * 4, frames (T + 1) C of 2^31 or more, an array not 16-byte aligned. */
int i2v_convit_join_cls_f32(const float* x, const float* cls, float* out, int frames, int T, int C, void* stream);
int i2v_convit_join_cls_bwd_f32(const float* dout, const float* add, float* dx, int frames, int T, int C, void* stream);

#ifdef __cplusplus
}
#endif
#endif
