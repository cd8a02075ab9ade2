/* libi2v_hip.so -- C ABI of the XCiT surrogates (timm 0.5.0's `XCiT` at 224 x 224 with patch 16: xcit_nano_12_p16_224 ...
 * xcit_large_24_p16_224 and their _dist twins), forward to the hooked blocks and backward to the input, run on the transformer stack.
 * DESIGN.md section 23 states the model.
 *
 * Same conventions as i2v_hip.h, i2v_vit.h, i2v_swin.h, i2v_convnext.h, i2v_mixer.h, i2v_cait.h and i2v_convit.h: every function returns 0
 * on success and non-zero on error with the text in `i2v_last_error()`; tensors are caller-owned contiguous fp32 DEVICE pointers; work is
 * enqueued on `stream` (a hipStream_t as void*, 0 = default) and nothing synchronises the host inside a forward or a backward.
 *
 * Model: the stem is four 3 x 3 / stride 2 / pad 1 convolutions (in_chans -> dim / 8 -> dim / 4 -> dim / 2 -> dim), each with a bias
 * (the caller's folded BatchNorm) and the first three followed by the exact erf GELU; T = (img / 16)^2 tokens, token = y * grid + x, no
 * prefix token; then + pos (T, dim).  Then `blocks` blocks, LayerNorm eps `ln_eps`, exact GELU:
 *   x = x + proj(XCA(LN1 x))        x = x + dw2(a * gelu(dw1(LN3 x) + b1) + s) + b2        x = x + fc2(gelu(fc1(LN2 x)))
 * XCA, per head h of width dh = dim / heads, over the T tokens:  nq[i] = max(||q[:, i]||_2, 1e-12), nk[j] likewise |
 *   Gh[i][j] = (sum_t q[t][i] k[t][j]) / nq[i] / nk[j] | A = softmax over j of temperature[h] * Gh | out[t][i] = sum_j A[i][j] v[t][j]
 * dw1, dw2: depthwise 3 x 3, pad 1, on the grid; the zero padding of dw2 is of a * gelu(u) + s, so a tap outside the plane adds 0, not s.
 * A hook is the residual stream after a block: T * dim floats per frame, token-major.
 *
 * WHAT THE CALLER FOLDS (XcitSpec.native_arrays, in float64 at load time): each stem BatchNorm into its convolution's weight and a bias;
 * the Fourier position features through their 1 x 1 convolution into one (T, dim) table; gamma1 into attn.proj, gamma2 into mlp.fc2, gamma3
 * into dw2's filter and bias; the BatchNorm between dw1 and dw2 into the per-channel pair (a, s); temperature as (heads).
 *
 * ARITHMETIC of the new launches (csrc/i2v_xcit.hip; csrc/i2v_xcit_host.h restates the definitions, not the order):
 *   - XCA normalises AFTER the product: the Gram q^T k is accumulated unnormalised and then divided by nq[i], then by nk[j];
 *   - an element of q^T k or dout^T v is ONE fp32 fma chain from 0 over the tokens in increasing order (the fp32 MFMA, bitwise an fmaf
 *     chain); a column's sum of squares likewise;
 *   - an element of out, dv and of the products inside dq and dk is one chain from 0 over the head index in chunks of 16, inside a chunk
 *     in the order 0 4 8 12 1 5 9 13 2 6 10 14 3 7 11 15, a chunk past dh filled with zero operands;
 *   - a row sum (the softmax denominator; sum_j dA A; r[i]): lane j holds element j, then a butterfly over lane distances 32 .. 1; c[j]
 *     adds the rows in increasing order; A = exp(S - max) / sum;
 *   - dS = A (dA - sum_j dA A), dG = temperature dS, r[i] = sum_j dG Gh, c[j] = sum_i dG Gh; dq[t][i] = (sum_j k[t][j] (dG[i][j] / nk[j])
 *     - q[t][i] (r[i] / nq[i])) / nq[i], dk[t][j] = (sum_i q[t][i] (dG[i][j] / nq[i]) - k[t][j] (c[j] / nk[j])) / nk[j], dv = dout A;
 *   - the depthwise launch: the bias, then the nine taps in increasing order (tap = 3 ky + kx), one fma each, the transform a * gelu(u) + s
 *     as one fma; then the residual; then one product with (a * gelu'(u));
 *   - the stem scatter adds its at most four contributions in increasing (ky, kx) order from 0, then multiplies by gelu'(pre);
 *   - no sum is split across workgroups and there are no atomics: reruns repeat the bits, and they depend on neither the frame count nor
 *     the frames a net was planned for. */
#ifndef I2V_XCIT_H
#define I2V_XCIT_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct i2v_xcit* i2v_xcit_handle;

typedef struct {
    int32_t img, in_chans, dim, heads, mlp, blocks;      /* input side (a multiple of 16), input channels, width, heads, MLP width, blocks */
    float ln_eps;
} i2v_xcit_config;

/* Weights: host fp32 arrays in this order, for the blocks 0 .. B-1 that run, B = deepest hooked block + 1:
 *   per stem convolution k = 1 .. 4 the folded weight (C_k, 9 C_{k-1}) with column = (3 ky + kx) C_{k-1} + c, and the folded bias (C_k);
 *   pos (T, dim);
 *   per block 21 arrays: norm1.weight, norm1.bias, attn.qkv.weight (3 dim, dim), attn.qkv.bias, temperature (heads), gamma1-folded
 *   attn.proj.weight (dim, dim) and bias, norm2.weight, norm2.bias, mlp.fc1.weight (mlp, dim), mlp.fc1.bias, gamma2-folded mlp.fc2.weight
 *   (dim, mlp) and bias, norm3.weight, norm3.bias, dw1's filter (9, dim) and bias, a (dim), s (dim), gamma3-folded dw2 filter (9, dim) and
 *   bias.
 * hook_blocks: zero-based block indices, distinct, in the order the hooks fire.  Uploads the weights and allocates the activation arena
 * for up to `max_frames` frames on `device` (synchronous: a planning step); sized in 64 bits before anything is allocated, and a plan the
 * device cannot hold is refused with the bytes it needs.  Refused as well: img no multiple of 16, dim no multiple of 8, dim / heads no
 * multiple of 4 or over 64, a hook hooked twice or outside the blocks. */
int i2v_xcit_create(int device, const i2v_xcit_config* cfg, const float* const* weights, int n_weights, const int32_t* hook_blocks, int n_hooks,
                    int max_frames, i2v_xcit_handle* out);
int i2v_xcit_destroy(i2v_xcit_handle net);
/* Bytes of device memory the net holds (weights and arena). */
int64_t i2v_xcit_workspace_bytes(i2v_xcit_handle net);
/* x: (frames, in_chans, img, img), frames <= max_frames.  Runs up to the deepest hooked block, keeping what the backward needs. */
int i2v_xcit_forward(i2v_xcit_handle net, const float* x, int frames, void* stream);
/* d(cost)/d(x) of the last forward from the hooks' gradient views (all of them are read): written into gx (accumulate = 0) or added to
 * it (accumulate = 1).  gx: (frames, in_chans, img, img). */
int i2v_xcit_backward(i2v_xcit_handle net, float* gx, int accumulate, void* stream);
/* D: T * dim. */
int i2v_xcit_hook_info(i2v_xcit_handle net, int hook, float** act, int64_t* act_stride, float** grad, int64_t* grad_stride, int64_t* D);
/* Copy hook `hook`'s activation (which = 0) or gradient (which = 1) for `frames` frames into out (frames, D), on `stream`. */
int i2v_xcit_read_hook(i2v_xcit_handle net, int hook, int which, float* out, int frames, void* stream);

/* ---- the kernels on their own (tests, tools) -----------------------------------------------------------------------------------
 * Cross-covariance attention.  qkv: (frames, T, 3 heads dh) as `i2v_vit_attention_f32` takes it (q of head h at column h dh, k at heads dh
 * + h dh, v at 2 heads dh + h dh); temperature: (heads).  The forward entry writes gram (frames, heads, dh + 2, dh) -- rows 0 .. dh - 1 the
 * normalised Gram Gh, row dh the clamped norms nq, row dh + 1 the clamped norms nk --, probs (frames, heads, dh, dh) = A, and out (frames, T,
 * heads dh).  The backward entry reads qkv, gram, probs and dout (frames, T, heads dh) and writes dqkv (frames, T, 3 heads dh).  One
 * workgroup owns one (frame, head); T is not bounded.  All arrays 16-byte aligned.  Refused with hipErrorInvalidValue and the reason: dh no
 * multiple of 4; dh over 64 (the dh x dh matrices of one head live in one workgroup's LDS and MFMA accumulators); more than 2^31 elements;
 * more than 65 535 frames or heads; null or misaligned arrays.  Exported by every build of the C ABI: where the library has no device
 * kernel (the host simulation) the same definitions run as scalar host code. */
int i2v_xcit_attention_f32(const float* qkv, int frames, int T, int heads, int dh, const float* temperature, float* gram, float* probs, float* out,
                           void* stream);
int i2v_xcit_attention_bwd_f32(const float* qkv, const float* gram, const float* probs, const float* dout, int frames, int T, int heads, int dh,
                               const float* temperature, float* dqkv, void* stream);
/* Token-major depthwise 3 x 3, pad 1: x, add, mu, y (n, H, W, C); w (9, C) with tap = 3 ky + kx; bias, ta, ts, ma (C).
 *   z = ta ? ta * gelu(x) + ts : x inside the plane, 0 outside | y = bias + sum_taps w z (+ add) | y *= ma * gelu'(mu) where ma is given
 * bias, add, the pair (ta, ts) and the pair (ma, mu) may be null.  y must not be x; add may be y.  Refused: C no multiple of 4, half a
 * pair, more than 2^31 elements, null or misaligned arrays. */
int i2v_xcit_dw3_f32(const float* x, int n, int H, int W, int C, const float* w, const float* bias, const float* ta, const float* ts,
                     const float* add, const float* ma, const float* mu, float* y, void* stream);
/* The stem's 3 x 3 / stride 2 / pad 1 gather: rows (frames Ho Wo, 9 C) with Ho = (H + 1) / 2, Wo = (W + 1) / 2 and column (3 ky + kx) C + c,
 * from src (frames, H, W, C) or, with nchw, (frames, C, H, W); zero outside the plane. */
int i2v_xcit_stem_gather_f32(const float* src, float* rows, int frames, int H, int W, int C, int nchw, void* stream);
/* Its transpose in gather form, one owner per element of dst: dst = (sum of the entries of drows that read the element, ky then kx
 * increasing) (* gelu'(pre), pre (frames, H, W, C), token-major dst only); with nchw dst is (frames, C, H, W) and `accumulate` adds to it. */
int i2v_xcit_stem_scatter_f32(const float* drows, const float* pre, float* dst, int frames, int H, int W, int C, int nchw, int accumulate,
                              void* stream);

#ifdef __cplusplus
}
#endif
#endif
