/* libi2v_hip.so -- C ABI of the ragged clip transform: whole decoded videos -> the reference's validation batch.
 *
 * Same conventions as i2v_hip.h (0 on success, `i2v_last_error()` for the text, work enqueued on `stream`).  Kept in a header
 * of its own: i2v_hip.h is the ABI that the planner's host simulation implements in full, and this entry has no place there.
 *
 * The Kinetics loader (i2v_amd/clips.py: kinetics_video_batches) selects 32 frames per clip from a whole decoded video by the
 * reference's arithmetic (datasets.py:216-244), which repeats frames and leaves clips of different lengths and sizes in one batch.
 * It uploads the DISTINCT selected frames once, as one uint8 pool, and describes the batch with three host tables:
 *
 *   offsets   int64 (b, t)      byte offset in the pool of frame ti of clip bi: H*W*3 bytes of that clip's frame size;
 *   geometry  int32 (b, 8)      per clip: H, W, resized height rh, resized width rw, crop origin y, crop origin x, first row of its
 *                               resize table in xtab, first row of its resize table in ytab;
 *   xtab/ytab int32 (rows, 3)   the clips' cv2 8-bit bilinear resize tables, concatenated (rw rows per clip in xtab, rh in ytab):
 *                               (source index, weight of it, weight of the next index) in 1/2048 units, as
 *                               `i2v_clip_resize_crop_u8_f32` takes them.
 */
#ifndef I2V_LOADER_H
#define I2V_LOADER_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Device scratch (bytes) that `i2v_clip_gather_resize_crop_u8_f32` needs for a batch of b clips x t frames whose tables hold
 * xtab_rows / ytab_rows rows; -1 for a negative argument. */
int64_t i2v_clip_gather_scratch_bytes(int b, int t, int xtab_rows, int ytab_rows);

/* The validation transform of the reference's loader (datasets.py:86-93, as `i2v_clip_resize_crop_u8_f32`: cv2 8-bit bilinear
 * resize, centre crop, /255, normalise) over a ragged batch in one launch: clip bi, frame ti is read from pool + offsets[bi][ti]
 * with the geometry of row bi, and lands in video (b, 3, t, out_h, out_w) fp32.  Bit-identical to `i2v_clip_resize_crop_u8_f32`
 * on a dense same-size batch.
 *
 * pool (DEVICE, 16-byte aligned, pool_bytes long) and video (DEVICE) are the caller's.  offsets, geometry, xtab and ytab are HOST
 * memory: every offset is checked against pool_bytes, every crop window against its resized frame, every table range against
 * xtab_rows / ytab_rows and every table entry the crop reads against its frame size (source indices inside the frame, and
 * non-decreasing along the axis) BEFORE anything is enqueued; a table that fails returns non-zero and launches nothing.  The
 * checked tables are then staged on `stream` into `scratch` (DEVICE, at least `i2v_clip_gather_scratch_bytes` bytes; it must stay
 * allocated until the launch has run).  The host tables may be released when the call returns.  Frame widths up to 8192. */
int i2v_clip_gather_resize_crop_u8_f32(const uint8_t* pool, int64_t pool_bytes, const int64_t* offsets, const int32_t* geometry,
                                       int b, int t, const int32_t* xtab, int xtab_rows, const int32_t* ytab, int ytab_rows,
                                       int out_h, int out_w, float* video, void* scratch, int64_t scratch_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
