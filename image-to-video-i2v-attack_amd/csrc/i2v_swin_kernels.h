// Internal interface of the Swin kernels (i2v_swin.hip) to their planner (i2v_swin.cpp).  The linear layers, the LayerNorm pair and the
// patchify kernel are the ViT ones (i2v_vit_kernels.h).
#pragma once
#ifdef __HIP__
#include <hip/hip_runtime.h>
#else
#include "i2v_hip_stub.h"     // (no HIP: the host simulation's build)
#endif
#include <stdint.h>

// Window attention core of one block over qkv (F, H*W, 3*heads*dh), token-major: the grid rolled by (-shift, -shift), cut into ws x ws
// windows, softmax((q dh^-0.5) k^T + B + M) v per (window, head), written to out (F, H*W, heads*dh) at the tokens' own places.
// table: relative_position_bias_table ((2 ws - 1)^2, heads).  Served (ws, dh): (7, 32) and (4, 16).
int swin_window_attention(const float* qkv, int F, int H, int W, int ws, int shift, int heads, int dh, const float* table, float* out,
                          hipStream_t s);
// dqkv (F, H*W, 3*heads*dh) from dout (F, H*W, heads*dh); the probabilities are recomputed from qkv.
int swin_window_attention_bwd(const float* qkv, const float* dout, int F, int H, int W, int ws, int shift, int heads, int dh,
                              const float* table, float* dqkv, hipStream_t s);
// x (F, H, W, C) -> out (F, H/2, W/2, 4C): quarter q of a merged row is the token at (row, column) offset (q & 1, q >> 1) of its 2 x 2 cell
int swin_merge_gather(const float* x, int F, int H, int W, int C, float* out, hipStream_t s);
// dx (F, H, W, C) = the adjoint of the gather applied to dout (F, H/2, W/2, 4C), plus `add` (F, H, W, C) when non-null
int swin_merge_scatter(const float* dout, int F, int H, int W, int C, const float* add, float* dx, hipStream_t s);
