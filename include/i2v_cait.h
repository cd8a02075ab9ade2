/* libi2v_hip.so -- C ABI of the CaiT surrogates (timm 0.5.0's `Cait` at 224 x 224: cait_xxs24_224, cait_xxs36_224, cait_s24_224), forward
 * to the hooked self-attention blocks and backward to the input, run on the transformer stack.  DESIGN.md section 21 states the model.
 *
 * Same conventions as i2v_hip.h, i2v_vit.h, i2v_swin.h, i2v_convnext.h and i2v_mixer.h: every function returns 0 on success and non-zero on
 * error with the text in `i2v_last_error()`; tensors are caller-owned contiguous fp32 DEVICE pointers; work is enqueued on `stream` (a
 * hipStream_t as void*, 0 = default) and nothing synchronises the host inside a forward or a backward.
 *
 * Model: the stem is a patch x patch convolution with stride patch and bias (in_chans -> dim), then + pos_embed (T, dim): T = (img /
 * patch)^2 tokens and NO prefix token -- CaiT's cls_token joins only in the class-attention stage, which lies behind every hook and is
 * not built.  Then `blocks` pre-norm blocks, LayerNorm eps `ln_eps`, exact erf GELU:
 *   x = x + gamma_1 * proj(THA(LN1 x))        x = x + gamma_2 * fc2(gelu(fc1(LN2 x)))
 * with the two LayerScale vectors folded into proj and fc2 by the caller.  THA is talking-heads attention over H heads of width dh = dim /
 * H, scale = dh^-0.5:
 *   S_h = (scale q_h) k_h^T | S'_g = sum_h Wl[g][h] S_h + bl[g] | P_g = softmax over keys | P'_g = sum_h Ww[g][h] P_h + bw[g] | O_g = P'_g v_g
 * A hook is the residual stream after a block, all tokens: T * dim floats per frame, token-major.
 *
 * ARITHMETIC of the attention launches (csrc/i2v_cait.hip; csrc/i2v_cait_host.h restates the definitions, not the order):
 *   - every product element is ONE fp32 fma chain from 0 (the fp32 MFMA, bitwise an fmaf chain).  Over the head width (q k^T, dout v^T)
 *     and over the keys (P' v, dS k) the contracted index goes in chunks of 16, inside a chunk in the order 0 4 8 12 1 5 9 13 2 6 10 14 3 7
 *     11 15, a chunk past the end filled with zero operands; over the query rows (dk, dv) in increasing order;
 *   - a head mix is acc = 0, acc = fma(w, x, acc) over the summed head index increasing, then + bias;
 *   - a row sum: lane l of 64 adds keys l, l + 64, ... in increasing order, then a butterfly over lane distances 32 .. 1;
 *   - q is multiplied by scale as it is loaded; dq and dk are scale * the finished chain;
 *   - no sum is split across workgroups and there are no atomics: reruns repeat the bits, and they depend on neither the frame count nor
 *     the frames a net was planned for. */
#ifndef I2V_CAIT_H
#define I2V_CAIT_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct i2v_cait* i2v_cait_handle;

typedef struct {
    int32_t img, patch, in_chans, dim, heads, mlp, blocks;      /* input side, patch side, input channels, width, heads, MLP width, blocks */
    float ln_eps;
} i2v_cait_config;

/* Weights: host fp32 arrays in this order, for the blocks 0 .. B-1 that run, B = deepest hooked block + 1:
 *   patch_embed.proj.weight (dim, in_chans, patch, patch), patch_embed.proj.bias (dim), pos_embed (T, dim);
 *   per block 16 arrays: norm1.weight, norm1.bias (dim), attn.qkv.weight (3 dim, dim), attn.qkv.bias (3 dim), attn.proj_l.weight (H, H),
 *   attn.proj_l.bias (H), attn.proj_w.weight (H, H), attn.proj_w.bias (H), attn.proj with gamma_1 folded in -- row o of the weight and
 *   element o of the bias times gamma_1[o] --, norm2.weight, norm2.bias, mlp.fc1.weight (mlp, dim), mlp.fc1.bias, and mlp.fc2 with gamma_2
 *   folded in the same way.
 * hook_blocks: zero-based block indices, distinct, in the order the hooks fire.  Uploads the weights and allocates the activation arena
 * for up to `max_frames` frames on `device` (synchronous: a planning step); sized in 64 bits before anything is allocated, and a plan the
 * device cannot hold is refused with the bytes it needs.  Refused as well: dim / heads no multiple of 4, and more heads than one
 * workgroup's LDS holds (heads * 16 * (T rounded up to 16, plus 4) floats within 160 KiB). */
int i2v_cait_create(int device, const i2v_cait_config* cfg, const float* const* weights, int n_weights, const int32_t* hook_blocks,
                    int n_hooks, int max_frames, i2v_cait_handle* out);
int i2v_cait_destroy(i2v_cait_handle net);
/* Bytes of device memory the net holds (weights and arena). */
int64_t i2v_cait_workspace_bytes(i2v_cait_handle net);
/* x: (frames, in_chans, img, img), frames <= max_frames.  Runs up to the deepest hooked block, keeping what the backward needs. */
int i2v_cait_forward(i2v_cait_handle net, const float* x, int frames, void* stream);
/* d(cost)/d(x) of the last forward from the hooks' gradient views (all of them are read): written into gx (accumulate = 0) or added to
 * it (accumulate = 1).  gx: (frames, in_chans, img, img). */
int i2v_cait_backward(i2v_cait_handle net, float* gx, int accumulate, void* stream);
int i2v_cait_hook_info(i2v_cait_handle net, int hook, float** act, int64_t* act_stride, float** grad, int64_t* grad_stride, int64_t* D);
/* Copy hook `hook`'s activation (which = 0) or gradient (which = 1) for `frames` frames into out (frames, D), on `stream`. */
int i2v_cait_read_hook(i2v_cait_handle net, int hook, int which, float* out, int frames, void* stream);

/* ---- the kernel on its own (tests, tools) --------------------------------------------------------------------------------------
 * qkv: (frames, T, 3 heads dh) as `i2v_vit_attention_f32` takes it (q of head h at column h dh, k at heads dh + h dh, v at 2 heads dh +
 * h dh); Wl, Ww: (heads, heads) row-major, bl, bw: (heads).  probs: (frames, heads, T, ld) with ld = i2v_vit_probs_ld(T), written by the
 * forward entry: P, post-softmax and pre-mix; out: (frames, T, heads dh).  The backward entry reads qkv, probs and dout (frames, T, heads
 * dh) and writes dqkv (frames, T, 3 heads dh); ds_scratch and pm_scratch are two arrays of probs' size it may overwrite.  All arrays 16-byte
 * aligned.  Refused with hipErrorInvalidValue and the reason: dh no multiple of 4; more heads than the LDS budget holds; more than 2^31
 * elements; more than 65 535 frames or tiles of 16 tokens.  Exported by every build of the C ABI: where the library has no device kernel
 * (the host simulation) the same definitions run as scalar host code. */
int i2v_cait_attention_f32(const float* qkv, int frames, int T, int heads, int dh, float scale, const float* Wl, const float* bl,
                           const float* Ww, const float* bw, float* probs, float* out, void* stream);
int i2v_cait_attention_bwd_f32(const float* qkv, const float* probs, const float* dout, int frames, int T, int heads, int dh, float scale,
                               const float* Wl, const float* Ww, const float* bw, float* ds_scratch, float* pm_scratch, float* dqkv,
                               void* stream);
/* x (frames, T, C) += pos (T, C) in place: the `+ pos_embed` launch of every stem without a prefix token (CaiT, ConViT, XCiT), one
 * rounded add per element.  Refused with hipErrorInvalidValue: a null array, frames, T or C not positive, C no multiple of 4, x or pos not
 * 16-byte aligned. */
int i2v_cait_add_pos_f32(float* x, const float* pos, int frames, int T, int C, void* stream);

#ifdef __cplusplus
}
#endif
#endif
