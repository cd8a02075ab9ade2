/* libi2v_hip.so -- C ABI of the 8-bit export and of the per-frame quality figures (PSNR's SSE, the largest difference in levels, SSIM) of
 * two clips that are on the device.  DESIGN.md section 35 states the definition and what was measured.
 *
 * Same conventions as i2v_hip.h (0 on success, non-zero with the text in `i2v_last_error()`, caller-owned contiguous DEVICE pointers, work
 * enqueued on `stream`, nothing synchronises the host).  Kept in a header of its own.  Every build of the C ABI exports these entries:
 * where the library has no device kernel (the host simulation) the same definitions run as scalar host code, to the same bits.
 *
 * A "level" is one step of the 8-bit grid: 255 x the unnormalised value.  mean = (0.485, 0.456, 0.406), std = (0.229, 0.224, 0.225).
 *
 * SSIM is Wang et al.'s, per colour channel in level units: an 11 x 11 Gaussian window, sigma 1.5, normalised, applied separably (rows,
 * then columns) over the VALID region (h - 10) x (w - 10); C1 = (0.01 * 255)^2, C2 = (0.03 * 255)^2; mu = G * x,
 * var_x = G * x^2 - mu^2, cov = G * xy - mu_a mu_b;
 *   ssim = (2 mu_a mu_b + C1)(2 cov + C2) / ((mu_a^2 + mu_b^2 + C1)(var_a + var_b + C2)),
 * the frame's figure the mean over the three channels and all valid positions.  The levels are fp32; the window sums and the formula
 * are double arithmetic on them (an fp32 sum of x^2 - mu^2 loses the variance of a bright flat region to rounding).  Fixed as well:
 *   - the moments are taken of level - 127.5 and 127.5 is added back to the means (the variances do not move with the centre);
 *   - products are rounded on their own and no fma spans the two operands: 2 (mu_a mu_b) + C1 against (mu_a^2 + mu_b^2) + C1, likewise
 *     2 cov + C2 against (var_a + var_b) + C2, and the division is correctly rounded, so identical operands give exactly 1.0;
 *   - the eleven taps are fp32 literals (csrc/i2v_quality_kernels.h), every window sum an fma chain from 0 over the taps in order.
 * csrc/i2v_quality_kernels.h fixes the tile (`i2v_clip_quality_tile`), the owner of every pixel and the order of every sum; partial sums
 * are doubles, folded in a fixed order by a second small launch, without atomics.  Reruns repeat the bits and a frame's three numbers do
 * not depend on how many frames share the call. */
#ifndef I2V_QUALITY_H
#define I2V_QUALITY_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* normalised clip (b,3,t,h,w) -> frames (b,t,h,w,3):
 *   q = rint(255 * clamp(fmaf(x, std[c], mean[c]), 0, 1))      (round half to even; a NaN becomes 0)
 * the exact inverse of `i2v_clip_from_u8_f32` on all 256 levels of all three channels.
 * ref != NULL (the clean clip's frames, same shape) with levels >= 0:
 *   q is then clamped to [ref - levels, ref + levels] and to [0, 255].
 * Refused, nothing launched: a null video or frames, a count below 1, a negative `levels` with a ref. */
int i2v_clip_to_u8(const float* video, const uint8_t* ref, int levels, uint8_t* frames, int b, int t, int h, int w, void* stream);

/* Bytes of device scratch the two quality entries need for `frames` frames of h x w: three doubles per tile. 0 for a refused shape. */
size_t i2v_clip_quality_scratch_bytes(int64_t frames, int h, int w);

/* The valid SSIM positions one tile covers, rows and columns: what a test brackets. */
void i2v_clip_quality_tile(int* rows, int* cols);

/* out[n][0..2] (doubles, device):
 *   SSE in level^2 over 3*h*w, max |a - b| in levels, mean SSIM.
 * _u8: a, b (frames,h,w,3) bytes at any alignment; SSE and max are formed in integers and are exact.
 * _f32: a, b (clips,3,t,h,w) normalised, frame n = clip*t + f; level = 255 * fmaf(x, std, mean), neither rounded nor clamped; the
 *   difference of an element is (255 * std[c]) * (xa - xb), formed in double.
 * scratch: `scratch_bytes` bytes, at least `i2v_clip_quality_scratch_bytes`, 8-byte aligned like out; free again when the work on
 * `stream` has run.  Any h, w >= 11; any number of frames.  Two launches.
 * Refused, nothing launched: a null pointer, h or w below 11, a count below 1, scratch smaller than the figure, a misaligned array. */
int i2v_clip_quality_u8(const uint8_t* a, const uint8_t* b, double* out, int64_t frames, int h, int w, void* scratch, int64_t scratch_bytes,
                        void* stream);
int i2v_clip_quality_f32(const float* a, const float* b, double* out, int clips, int t, int h, int w, void* scratch, int64_t scratch_bytes,
                         void* stream);

#ifdef __cplusplus
}
#endif
#endif
