/* libi2v_hip.so -- C ABI of the TNT surrogates (timm 0.5.0's `TNT`, Transformer in Transformer, at 224 x 224: tnt_s_patch16_224 /
 * tnt_b_patch16_224), forward to the hooked blocks and backward to the input, run on the transformer stack.  DESIGN.md section 31 states
 * the model; the key layout is restated from memory of timm 0.5.0's tnt.py and UNCHECKED against timm.
 *
 * Same conventions as i2v_hip.h, i2v_vit.h and the other family headers: every function returns 0 on success and non-zero on error with
 * the text in `i2v_last_error()`; tensors are caller-owned contiguous fp32 DEVICE pointers; work is enqueued on `stream` (a hipStream_t
 * as void*, 0 = default) and nothing synchronises the host inside a forward or a backward.
 *
 * Model: two residual streams.  The INNER stream holds 16 "pixel" tokens of width in_dim for every one of the g^2 = (img / 16)^2 patches:
 * (frames g^2, 16, in_dim).  It starts as a Conv2d(in_chans, in_dim, 7, stride 4, padding 3) of the frame -- pixel token p = 4 i + j of
 * patch n = g py + px is the conv output at (4 py + i, 4 px + j) -- plus `pixel_pos` per (channel, i, j).  The OUTER stream holds 1 + g^2
 * tokens of width dim: patch n is norm2_proj(proj(norm1_proj(the patch's 16 in_dim inner floats, column p in_dim + c))), the class token in
 * front, `patch_pos` added.  Block, LayerNorm eps `ln_eps`, exact GELU, no qkv bias, attention scale (head width)^-0.5:
 *   inner = inner + attn_in(norm_in inner)       inner = inner + mlp_in(norm_mlp_in inner)        in_heads heads over the 16 pixel tokens
 *   outer[:, 1:] = outer[:, 1:] + proj(norm1_proj(inner) as (frames, g^2, 16 in_dim))             norm1_proj over in_dim, per pixel token
 *   outer = outer + attn_out(norm_out outer)     outer = outer + mlp(norm_mlp outer)              heads heads over the 1 + g^2 tokens
 * Both halves are the shared pre-norm block (qk.weight stacked on v.weight as one qkv weight, a zero qkv bias); the MLPs are
 * mlp_ratio x their width.  A hook is the OUTER stream after a block, all tokens with the class token: (1 + g^2) dim floats per frame.
 * The deepest hooked block's inner stream receives gradient only through the proj into the outer stream.
 *
 * ARITHMETIC of the new launches (csrc/i2v_tnt.hip; csrc/i2v_tnt_host.h restates them in the same order, only expf is the host's own):
 *   - attention, per (sequence, head, row i), every sum an fmaf chain from 0 in increasing index: s[j] = (q_i . k_j) scale, the
 *     product summed over the head's columns; m = max s; e[j] = exp(s[j] - m); l = e[0] + e[1] + ...; P[j] = e[j] / l;
 *     out_i[d] = the chain over the keys j of P[j] v_j[d];
 *   - backward, P recomputed as above (nothing of the forward is kept): dP[j] = dout_i . v_j over the columns; delta = the chain over j
 *     of P[j] dP[j]; dS[j] = P[j] (dP[j] - delta); dq_i[d] = (the chain over j of dS[j] k_j[d]) scale, owned by the row;
 *     dk_j[d] = (the chain over the rows i of dS[i][j] q_i[d]) scale and dv_j[d] = the chain over i of P[i][j] dout_i[d], owned by the
 *     key, which forms P[i][j] and dS[i][j] again from the row's (m, l, delta) by the same expressions.  Where a row of P is one-hot,
 *     delta equals that key's dP exactly and the row's dS is 0;
 *   - the pixel gather copies (zeros outside the frame and in the padding columns); the scatter sums the at most 2 x 2 conv outputs whose
 *     window holds the pixel from 0, the output row then the output column increasing, and writes, or adds the finished value once;
 *   - the row add is one addition per element.
 * Every output element has one owner, there are no atomics, a workgroup owns whole sequences and no sum crosses sequences: reruns repeat
 * the bits, and sequence 0 of an n-sequence call has the bits of a 1-sequence call, whatever the other sequences in its workgroup. */
#ifndef I2V_TNT_H
#define I2V_TNT_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct i2v_tnt* i2v_tnt_handle;

typedef struct {
    int32_t img, in_chans;                             /* input side (a multiple of 16), input channels */
    int32_t dim, in_dim, heads, in_heads, mlp_ratio, blocks;
    float ln_eps;
} i2v_tnt_config;

/* Weights: host fp32 arrays in this order, for the blocks 0 .. B-1 that run, B = deepest hooked block + 1.  First 11 arrays:
 *   pixel_embed.proj.weight as (in_dim, Kp), the (in_dim, in_chans 49) filter rows padded with zeros to Kp = in_chans 49 rounded up to 4,
 *   its bias, pixel_pos as (16, in_dim) with row p = 4 i + j, norm1_proj.weight, .bias (16 in_dim), proj.weight (dim, 16 in_dim), .bias,
 *   norm2_proj.weight, .bias (dim), cls_token (dim), patch_pos (1 + g^2, dim);
 *   then per block 28 arrays: the inner half -- norm_in.weight, .bias, [attn_in.qk.weight; attn_in.v.weight] (3 in_dim, in_dim), a zero
 *   bias (3 in_dim), attn_in.proj.weight, .bias, norm_mlp_in.weight, .bias, mlp_in.fc1.weight, .bias, mlp_in.fc2.weight, .bias --,
 *   norm1_proj.weight, .bias (in_dim), proj.weight (dim, 16 in_dim), .bias, and the outer half in the same order of 12 (norm_out,
 *   attn_out, norm_mlp, mlp).
 * hook_blocks: zero-based block indices, distinct, in the order the hooks fire.  Uploads the weights and allocates the activation arena
 * for up to `max_frames` frames on `device` (synchronous: a planning step); sized in 64 bits before anything is allocated, and a plan the
 * device cannot hold is refused with the bytes it needs.  Refused as well: a frame side that is no multiple of 16 or gives more than 208
 * outer tokens; an inner head wider than 16, more than 8 inner heads, in_dim no multiple of 4; an outer head width that is no multiple
 * of 4 or over 64; a hook hooked twice or outside the blocks. */
int i2v_tnt_create(int device, const i2v_tnt_config* cfg, const float* const* weights, int n_weights, const int32_t* hook_blocks, int n_hooks,
                   int max_frames, i2v_tnt_handle* out);
int i2v_tnt_destroy(i2v_tnt_handle net);
/* Bytes of device memory the net holds (weights and arena). */
int64_t i2v_tnt_workspace_bytes(i2v_tnt_handle net);
/* x: (frames, in_chans, img, img), frames <= max_frames.  Runs up to the deepest hooked block, keeping what the backward needs. */
int i2v_tnt_forward(i2v_tnt_handle net, const float* x, int frames, void* stream);
/* d(cost)/d(x) of the last forward from the hooks' gradient views (all of them are read): written into gx (accumulate = 0) or added to
 * it (accumulate = 1).  gx: (frames, in_chans, img, img). */
int i2v_tnt_backward(i2v_tnt_handle net, float* gx, int accumulate, void* stream);
/* D: (1 + g^2) dim. */
int i2v_tnt_hook_info(i2v_tnt_handle net, int hook, float** act, int64_t* act_stride, float** grad, int64_t* grad_stride, int64_t* D);
/* Copy hook `hook`'s activation (which = 0) or gradient (which = 1) for `frames` frames into out (frames, D), on `stream`. */
int i2v_tnt_read_hook(i2v_tnt_handle net, int hook, int which, float* out, int frames, void* stream);

/* ---- the kernels on their own (tests, tools) --------------------------------------------------------------------------------------
 * Exported by every build of the C ABI: where the library has no device kernel (the host simulation) the same definitions run as scalar
 * host code.  Each refuses with hipErrorInvalidValue and the reason, nothing launched.
 *
 * Attention over `seqs` short sequences.  qkv (seqs, T, 3 heads dh) in the layout every family uses; out, dout (seqs, T, heads dh);
 * dqkv as qkv, all of it written.  1 <= T <= 16, 1 <= dh <= 16 (any width), 1 <= heads <= 8, heads dh a multiple of 4, fewer than 2^31
 * elements, 16-byte aligned arrays.  One launch each; the backward takes nothing from the forward. */
int i2v_tnt_attention_f32(const float* qkv, int64_t seqs, int T, int heads, int dh, float scale, float* out, void* stream);
int i2v_tnt_attention_bwd_f32(const float* qkv, const float* dout, int64_t seqs, int T, int heads, int dh, float scale, float* dqkv, void* stream);
/* Sequences one workgroup of those launches owns for this shape (forward and backward alike): what a test brackets. */
int i2v_tnt_attention_group(int T, int heads, int dh);
/* The rows of the 7 x 7, stride 4, padding 3 pixel convolution.  x (frames, in_chans, side, side), side a multiple of 16;
 * rows (frames (side / 16)^2 16, Kp), Kp = in_chans 49 rounded up to 4, in (patch, pixel) order, column c 49 + ky 7 + kx.  The scatter is
 * the transpose: dx written, or added to (accumulate). */
int i2v_tnt_pixel_gather_f32(const float* x, int frames, int in_chans, int side, float* rows, void* stream);
int i2v_tnt_pixel_scatter_f32(const float* rows, int frames, int in_chans, int side, int accumulate, float* dx, void* stream);

#ifdef __cplusplus
}
#endif
#endif
