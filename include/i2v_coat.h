/* libi2v_hip.so -- C ABI of the CoaT-Lite surrogates (timm 0.5.0's `CoaT` with serial blocks only at 224 x 224: coat_lite_tiny /
 * coat_lite_mini / coat_lite_small), forward to the hooked stages and backward to the input, run on the transformer stack.  DESIGN.md
 * section 30 states the model; the key layout is restated from memory of timm 0.5.0's coat.py and UNCHECKED against timm.
 *
 * Same conventions as i2v_hip.h, i2v_vit.h and the other family headers: every function returns 0 on success and non-zero on error with
 * the text in `i2v_last_error()`; tensors are caller-owned contiguous fp32 DEVICE pointers; work is enqueued on `stream` (a hipStream_t
 * as void*, 0 = default) and nothing synchronises the host inside a forward or a backward.
 *
 * Model: four stages.  Stage 0 embeds 4 x 4 patches (a Linear and a LayerNorm) onto a grid of img / 4 a side; every later stage embeds
 * the 2 x 2 cells of its predecessor's grid tokens (the class token dropped), a Linear and a LayerNorm.  Each stage puts its own class
 * token in front: T = 1 + g^2 tokens, dims[k] wide.  There is no position table.  A block, LayerNorm eps `ln_eps`, exact GELU:
 *   x = cpe(x)       the stage's depthwise 3 x 3 on the grid tokens with a residual; the class row passes through
 *   x = x + proj(FA(LN1 x))        x = x + fc2(gelu(fc1(LN2 x)))        MLP width mlp_ratios[k] x dims[k]
 * FA, per head of width dh = dims[k] / heads over all T tokens:  Ks = softmax of k over the TOKENS, per column;  G = Ks^T v (dh x dh);
 *   out = dh^-0.5 q G + q o E.  E is 0 on the class row and on the grid rows the stage's crpe of v as an image: the first win3 heads pass
 *   a depthwise 3 x 3, the next win5 a 5 x 5, the last win7 a 7 x 7, each with "same" padding and a bias.
 * A hook is the residual stream after the last block of a stage, all tokens with the class token, before the next patch embedding:
 * (1 + g^2) * dims[k] floats per frame.
 *
 * ARITHMETIC of the new launches (csrc/i2v_coat.hip; csrc/i2v_coat_host.h restates the definitions, not the attention's order):
 *   - REDUCE, forward: one workgroup owns a (frame, head group) -- max(1, 64 / dh) whole heads -- and walks the tokens in tiles of 64 in
 *     increasing order, ONE sweep under an online rescale.  Per tile and column of k: the tile maximum (order immaterial);
 *     m' = max(m, tile maximum), alpha = exp(m - m'); e = exp(k - m') per token; the tile's sum of e as four partial sums over the tokens
 *     16 n .. 16 n + 15 (increasing, from 0) added as ((p0 + p1) + p2) + p3; l = l alpha + that sum; row a of G is multiplied by alpha[a]
 *     in EVERY tile (alpha is exactly 1 where the maximum has not moved; there is no threshold), then an element of G adds the tile's 64
 *     tokens e[t][a] v[t][b] in increasing token order as ONE fp32 fma chain (the fp32 MFMA, bitwise an fmaf chain; tokens past T are
 *     zero operands).  At the end gram = G / l, kstat = (m, log l);
 *   - REDUCE, backward: the same ownership and token order without the rescale: dG[a][b] is one fma chain from 0 over all tokens of
 *     q[t][a] dout[t][b], then one product with the scale;
 *   - APPLY, forward: an element of q G is one fma chain from 0 over the head index a in chunks of 16, inside a chunk in the order
 *     0 4 8 12 1 5 9 13 2 6 10 14 3 7 11 15 (a chunk past dh filled with zero operands); out = (chain * scale) + (q * E);
 *   - APPLY, backward: dout G^T, Ks dG and v dG^T are chains in the chunk order above; c[a] is one fma chain from 0 of G[a][b] dG[a][b]
 *     over b in that same order (so that where a softmax column is one-hot, v dG^T - c cancels exactly), formed by every workgroup from
 *     the same G and dG (the same bits everywhere);
 *     dq = (chain * scale) + (dout * E), dE = dout * q, dv = chain, dk = Ks * (chain - c), Ks = exp((k - max) - logsum) from kstat:
 *     no reduction over tokens;
 *   - dwmix adds its taps (ky, kx) in increasing order onto the bias (backward: from 0, over the mirrored filter in gather form), a tap
 *     on the padding taking no part; the residual is added last, x + (that sum); accumulate adds the finished value to dx;
 *   - the cell gather copies; the scatter copies or adds once.
 * Every output element has one owner, no sum is split across workgroups, there are no atomics, a workgroup reads its own frame only:
 * reruns repeat the bits, and frame 0 of an n-frame call has the bits of a 1-frame call. */
#ifndef I2V_COAT_H
#define I2V_COAT_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct i2v_coat* i2v_coat_handle;

#define I2V_COAT_STAGES 4

typedef struct {
    int32_t img, in_chans;                             /* input side (a multiple of 32), input channels */
    int32_t dims[I2V_COAT_STAGES], heads, depths[I2V_COAT_STAGES], mlp_ratios[I2V_COAT_STAGES];
    int32_t win3, win5, win7;                          /* heads that pass the 3 x 3, the 5 x 5 and the 7 x 7 of crpe: they sum to heads */
    float ln_eps;
} i2v_coat_config;

/* Weights: host fp32 arrays in this order, for the stages 0 .. S-1 that run, S = deepest hooked stage + 1.  Per stage 12 arrays:
 *   patch_embed.proj.weight as a Linear -- stage 0 (dims[0], in_chans 16) flattened as it stands, later stages (C, 4 C') with column
 *   (dy 2 + dx) C' + c --, its bias, patch_embed.norm.weight, .bias, cls_token (C), a table of ZEROS (1 + g^2, C) (the shared token
 *   assembly adds a table), cpe.proj.weight as (9, C) tap-major, its bias, crpe's three filters as (9, n3), (25, n5), (49, n7) tap-major
 *   with n = window heads x dh, and crpe's biases concatenated in channel order (C);
 *   then per block 12 arrays: norm1.weight, .bias, factoratt_crpe.qkv.weight (3 C, C), .bias, factoratt_crpe.proj.weight, .bias,
 *   norm2.weight, .bias, mlp.fc1.weight (r C, C), .bias, mlp.fc2.weight (C, r C), .bias.
 * hook_stages: zero-based stage indices, distinct, in the order the hooks fire.  Uploads the weights and allocates the activation arena
 * for up to `max_frames` frames on `device` (synchronous: a planning step); sized in 64 bits before anything is allocated, and a plan the
 * device cannot hold is refused with the bytes it needs.  Refused as well: a frame side that is no multiple of 32; a head width that is
 * no multiple of 4 or over 64; window head counts that are not positive or do not sum to heads; a hook hooked twice or outside the
 * stages. */
int i2v_coat_create(int device, const i2v_coat_config* cfg, const float* const* weights, int n_weights, const int32_t* hook_stages, int n_hooks,
                    int max_frames, i2v_coat_handle* out);
int i2v_coat_destroy(i2v_coat_handle net);
/* Bytes of device memory the net holds (weights and arena). */
int64_t i2v_coat_workspace_bytes(i2v_coat_handle net);
/* x: (frames, in_chans, img, img), frames <= max_frames.  Runs up to the deepest hooked stage, keeping what the backward needs. */
int i2v_coat_forward(i2v_coat_handle net, const float* x, int frames, void* stream);
/* d(cost)/d(x) of the last forward from the hooks' gradient views (all of them are read): written into gx (accumulate = 0) or added to
 * it (accumulate = 1).  gx: (frames, in_chans, img, img). */
int i2v_coat_backward(i2v_coat_handle net, float* gx, int accumulate, void* stream);
/* D: tokens * width of the hooked stage. */
int i2v_coat_hook_info(i2v_coat_handle net, int hook, float** act, int64_t* act_stride, float** grad, int64_t* grad_stride, int64_t* D);
/* Copy hook `hook`'s activation (which = 0) or gradient (which = 1) for `frames` frames into out (frames, D), on `stream`. */
int i2v_coat_read_hook(i2v_coat_handle net, int hook, int which, float* out, int frames, void* stream);

/* ---- the kernels on their own (tests, tools) --------------------------------------------------------------------------------------
 * Exported by every build of the C ABI: where the library has no device kernel (the host simulation) the same definitions run as scalar
 * host code.  Each refuses with hipErrorInvalidValue and the reason, nothing launched: dh no multiple of 4 or over 64; a group width no
 * multiple of 4; a grid dimension over 65 535; more than 2^31 elements; null or misaligned (16 bytes) arrays; a non-positive size.
 *
 * Factorized attention.  qkv (frames, T, 3 heads dh) in the layout every family uses; E, out, dout (frames, T, heads dh); the saves
 * gram (frames, heads, dh, dh) = G and kstat (frames, heads, 2, dh) = column maximum and log of the column sum.  T unbounded.  Two
 * launches: the reduce per (frame, head group), the apply per (frame, head group, tile of 64 tokens). */
int i2v_coat_factor_attention_f32(const float* qkv, const float* E, int frames, int T, int heads, int dh, float scale,
                                  float* gram, float* kstat, float* out, void* stream);
/* dqkv (frames, T, 3 heads dh), all of it written; dE (frames, T, heads dh) = dout o q, which the caller sends through the crpe
 * backward onto dv.  dgram: scratch laid out as gram (it leaves holding dG = scale q^T dout).  Two launches. */
int i2v_coat_factor_attention_bwd_f32(const float* qkv, const float* E, const float* gram, const float* kstat, const float* dout,
                                      int frames, int T, int heads, int dh, float scale, float* dgram, float* dqkv, float* dE, void* stream);
/* x: frames of (prefix + g^2) rows at row stride x_rs floats (x_rs = 3 C reads v out of qkv in place); y likewise at y_rs.  Channels
 * 0 .. n3-1 take the 3 x 3 filter, n3 .. n3+n5-1 the 5 x 5, the rest up to C the 7 x 7 ("same" zero padding, taps (ky, kx) increasing,
 * onto the bias); w3 (9, n3), w5 (25, n5), w7 (49, C-n3-n5), a filter without channels may be null; bias (C) or null; residual != 0
 * adds x (cpe).  The prefix rows of y are written 0 (residual 0) or copied (residual 1).  The backward is the same launch on the
 * mirrored filters in gather form, one owner per element, written or added (accumulate) -- dv takes the crpe's gradient by accumulate;
 * its prefix rows: dy's (residual 1) or 0, and under accumulate with residual 0 not touched. */
int i2v_coat_dwmix_f32(const float* x, int64_t x_rs, const float* w3, const float* w5, const float* w7, const float* bias, int frames, int g,
                       int C, int n3, int n5, int prefix, int residual, float* y, int64_t y_rs, void* stream);
int i2v_coat_dwmix_bwd_f32(const float* dy, int64_t dy_rs, const float* w3, const float* w5, const float* w7, int frames, int g, int C, int n3,
                           int n5, int prefix, int residual, int accumulate, float* dx, int64_t dx_rs, void* stream);
/* The s x s cells of a token-major plane behind `prefix` rows.  x: (frames, prefix + g^2, C); rows: (frames (g / s)^2, s^2 C) with column
 * (dy s + dx) C + c; s = 1 strips the prefix rows.  The scatter is the inverse: dx written with its prefix rows 0, or added to
 * (accumulate) with the prefix rows untouched.  Refused as well: cells that do not tile the plane, C no multiple of 4. */
int i2v_coat_cell_gather_f32(const float* x, int frames, int g, int C, int s, int prefix, float* rows, void* stream);
int i2v_coat_cell_scatter_f32(const float* rows, int frames, int g, int C, int s, int prefix, int accumulate, float* dx, void* stream);

#ifdef __cplusplus
}
#endif
#endif
