/* libi2v_hip.so -- the grouped 3x3 convolution (csrc/i2v_gconv.hip), the depthwise k x k convolution (csrc/i2v_dwconv.hip) and the
 * squeeze-and-excitation node (csrc/i2v_se.hip) reachable on their own with arbitrary geometry: tests and tools.  No planner calls these
 * entries and they change no launch; they pack, plan and fill the parameter structs with the functions the planner itself calls
 * (csrc/i2v_conv_aux.h), so what they run is what a planned graph runs.
 *
 * Same conventions as i2v_hip.h: every function returns 0 on success and non-zero on error with the text in `i2v_last_error()`, which
 * starts with the entry's name and names the launch that refused; tensors are caller-owned fp32 pointers of the library's memory space
 * (device pointers in libi2v_hip.so, host pointers in the host simulation) unless marked HOST; work is enqueued on `stream` (a
 * hipStream_t as void*, 0 = default).  Unlike the planned launches these entries upload their weights on every call and wait for the
 * stream before they return: they are not for timing.
 */
#ifndef I2V_CONV_AUX_LAUNCH_H
#define I2V_CONV_AUX_LAUNCH_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* One launch of a convolution `Conv2d(C, C, k, stride, k / 2, groups)` over N frames, forward or input gradient.  (H, W) is the
 * convolution's INPUT plane and (Ho, Wo) = ((H - 1) / stride + 1, (W - 1) / stride + 1) its output plane, whichever way the launch runs:
 *   forward   src (N, C, H, W)   -> dst (N, C, Ho, Wo) = epilogue(conv(src))
 *   backward  src (N, C, Ho, Wo) -> dst (N, C, H, W)   = epilogue(the input gradient of conv for the output gradient src)
 * with frame strides `src_nstride`, `dst_nstride` in floats (>= the frame).  Epilogue: + shift[c] (shift null: none), ReLU (`relu`),
 * then zero where the gate of the produced tensor is off: `gate` (1-bit rows, bit n Hd Wd + pixel of row c, `gate_stride` words per
 * row) or else `mask` (an fp32 tensor of dst's shape with frame stride `mask_nstride`: on where mask > 0).  `gate_out`: the launch
 * writes dst's own gate rows, bit = (dst > 0), `gate_out_stride` words per row -- launches that write dst densely only (a forward launch at
 * either stride; a stride-2 input-gradient launch, which writes dst at stride 2 in four classes, is refused).
 * `filter` is a HOST pointer to the torch-layout weight: [C][C / groups][3][3] (grouped) or [C][k][k] (depthwise). */
typedef struct {
    const float* src; int64_t src_nstride;
    float* dst; int64_t dst_nstride;
    const float* plan_src;             /* depthwise only: the source the launch is PLANNED for (null: src); it is launched on src */
    const float* filter;               /* HOST */
    const float* shift;
    uint32_t* gate_out; const uint32_t* gate; const float* mask; int64_t mask_nstride;
    int32_t gate_out_stride, gate_stride;
    int32_t N, C, H, W, stride, backward, relu;
    int32_t groups;                    /* grouped: the group count (C / groups in {4, 8, 16, 32, 64}); depthwise: unused */
    int32_t k;                         /* depthwise: 3 or 5; grouped: unused (3) */
} i2v_conv_aux_desc;

/* The plan the launch ran with (k_gconv_plan / k_dwconv_plan): waves of 64 positions per block, staged source rows, floats per staged
 * row (grouped: W_src + 2), dynamic LDS bytes, 16-byte staging (depthwise only). */
typedef struct { int32_t waves, rows, pitch, lds_bytes, v4; } i2v_conv_aux_plan;

/* libi2v_hip.so only: the host simulation runs such nodes on the dense route and has no twin of these kernels.  `plan` may be null; it
 * is filled as soon as the launch is planned, also when the launch itself is then refused.  N == 0: 0, nothing is launched. */
int i2v_gconv_f32(const i2v_conv_aux_desc* desc, i2v_conv_aux_plan* plan, void* stream);
int i2v_dwconv_f32(const i2v_conv_aux_desc* desc, i2v_conv_aux_plan* plan, void* stream);

/* The packed operands of those launches, HOST in and HOST out, on every build.  fwd: [groups][gw ci][9][gw co] (grouped; depthwise: the
 * filter as it is, no output).  bwd: [stride^2 classes][...] the transposed, mirrored kernel of each stride-parity class with zeros in
 * the slots the class does not own.  classes: stride^2 rows of (Hg, Wg, oh0, ow0, tapmask), the input-gradient launch's classes over an
 * (H, W) destination.  Any output may be null. */
int i2v_gconv_pack_f32(const float* filter, int groups, int gw, int stride, int H, int W, float* fwd, float* bwd, int32_t* classes);
int i2v_dwconv_pack_f32(const float* filter, int C, int k, int stride, int H, int W, float* bwd, int32_t* classes);

/* The three launches of one pass of a squeeze-and-excitation node (timm SEModule + the block's shortcut add and ReLU) over N frames of C
 * planes of HW positions:
 *   forward   m = mean_p x;  h = relu(w1 m + b1);  s = sigmoid(w2 h + b2);  dst = act(x * s + r)      (r null: none; act: `relu`)
 *   backward  t = sum_p g x;  dmh = w1^T ((w2^T (t s (1 - s))) where h > 0) / HW;  dst = g * s + dmh   (h, s as the forward left them)
 * w1 [rd][C], b1 [rd], w2 [C][rd] (torch layout; transposed here as the engine does), b2 [C] are HOST pointers.  m, s, t, dmh (N, C) and
 * h (N, rd) are the caller's scratch vectors in the library's memory space.  `gate_out` (forward with ReLU only): dst's gate rows.
 * `launches`: bit 0 squeeze, bit 1 excite, bit 2 scale; 0 = all three, in that order.  Exported by every build: the host simulation runs
 * the same node as scalar host code (csrc/i2v_se_host.h), which sets and clears gate bits in place. */
typedef struct {
    const float* x; int64_t x_nstride;
    const float* g; int64_t g_nstride;
    const float* r; int64_t r_nstride;
    float* dst; int64_t dst_nstride;
    const float *w1, *b1, *w2, *b2;    /* HOST */
    float *m, *h, *s, *t, *dmh;
    uint32_t* gate_out; int32_t gate_out_stride;
    int32_t N, C, rd, HW, relu, backward, launches;
} i2v_se_desc_f32;
int i2v_se_f32(const i2v_se_desc_f32* desc, void* stream);

#ifdef __cplusplus
}
#endif
#endif
