// The loop kernels' C entries: argument checks in front of one backend call each.  None of them touches a net.
#include "i2v_net.h"
#include "../../include/i2v_nl_launch.h"
#ifndef I2V_HAVE_CONVNEXT
#include "i2v_convnext_host.h"   // (the host simulation's one-file build: the token-major depthwise launch as scalar code)
#endif
#ifndef I2V_HAVE_MIXER
#include "i2v_mixer_host.h"      // (... and the token-mixing launch)
#endif

#include <math.h>
#include <string.h>

using namespace eng;

// The shape of an entry: refuse bad arguments under the entry's own name ("<entry>: bad argument<what is expected>"), set the
// parameters up, then one backend call whose failure is reported like any CHECK_BE.
#define BAD_ARG_IF(cond, ...) do { if (cond) return fail("%s: bad argument" __VA_ARGS__, __func__); } while (0)
#define RETURN_BE(call) do { CHECK_BE(call); return 0; } while (0)

// ---------------------------------------------------------------------------------------------
// loop kernels
// ---------------------------------------------------------------------------------------------
extern "C" int i2v_clip_from_u8_f32(const uint8_t* frames, float* video, int b, int t, int hh, int w, void* stream) {
    BAD_ARG_IF(!frames || !video || b <= 0 || t <= 0 || hh <= 0 || w <= 0);
    RETURN_BE(k_clip_from_u8(frames, video, b, t, hh, w, stream));
}

extern "C" int i2v_clip_resize_crop_u8_f32(const uint8_t* frames, float* video, const int32_t* xtab, const int32_t* ytab, int b, int t,
                                           int H, int W, int rh, int rw, int crop_y, int crop_x, int out_h, int out_w, void* stream) {
    BAD_ARG_IF(!frames || !video || !xtab || !ytab || b <= 0 || t <= 0 || H <= 0 || W <= 0 || out_h <= 0 || out_w <= 0);
    if (crop_y < 0 || crop_x < 0 || crop_y + out_h > rh || crop_x + out_w > rw) return fail("i2v_clip_resize_crop_u8_f32: crop window outside the resized frame");
    RETURN_BE(k_clip_resize_crop(frames, video, xtab, ytab, b, t, H, W, crop_y, crop_x, out_h, out_w, stream));
}

extern "C" int i2v_clip_resample_crop_u8_f32(const uint8_t* frames, float* video, const int32_t* xbounds, const int32_t* xcoef, int kx,
                                             const int32_t* ybounds, const int32_t* ycoef, int ky, int b, int t, int H, int W, int rh, int rw,
                                             int crop_y, int crop_x, int out_h, int out_w, void* stream) {
    BAD_ARG_IF(!frames || !video || !xbounds || !xcoef || !ybounds || !ycoef || kx <= 0 || ky <= 0 || b <= 0 || t <= 0 || H <= 0 || W <= 0 || out_h <= 0 || out_w <= 0);
    if (crop_y < 0 || crop_x < 0 || crop_y + out_h > rh || crop_x + out_w > rw) return fail("i2v_clip_resample_crop_u8_f32: crop window outside the resized frame");
    RETURN_BE(k_clip_resample_crop(frames, video, xbounds, xcoef, kx, ybounds, ycoef, ky, b, t, H, W, crop_y, crop_x, out_h, out_w, stream));
}

extern "C" int i2v_frames_from_video_f32(const float* video, float* x, float* u, int b, int f, int hh, int w,
                                         void* stream) {
    BAD_ARG_IF(!video || !x || !u || b <= 0 || f <= 0 || hh <= 0 || w <= 0);
    RETURN_BE(k_frames_from_video(video, x, u, b, f, hh, w, stream));
}

extern "C" int i2v_compose_f32(const float* u, const float* delta, float* x, int b, int f, int hh, int w,
                               float eps, int video_layout, void* stream) {
    BAD_ARG_IF(!u || !delta || !x || b <= 0 || f <= 0 || hh <= 0 || w <= 0);
    RETURN_BE(k_compose(u, delta, x, b, f, hh, w, eps, video_layout, stream));
}

extern "C" size_t i2v_cossim_scratch_bytes(int64_t D, int frames) {
    return ((size_t)frames * cos_nblk(D) * 4 + 2) * sizeof(double);
}

extern "C" int i2v_cossim_fwd_bwd_f32(const float* a, int64_t a_stride, const float* b, int64_t b_stride,
                                      int64_t D, int frames, const float* coef_dev, int coef_index,
                                      float coef_host, int mask_relu, int accumulate, float* cos_out,
                                      float* grad, int64_t grad_stride, void* scratch, void* stream) {
    BAD_ARG_IF(!a || !b || !cos_out || !grad || !scratch || D <= 0 || frames <= 0);
    I2VCosParams p; memset(&p, 0, sizeof p);
    p.a = a; p.a_nstride = a_stride; p.b = b; p.b_nstride = b_stride; p.D = D; p.N = frames;
    p.partial = (float*)scratch; p.nblk = cos_nblk(D); p.cos_out = cos_out; p.grad = grad; p.grad_nstride = grad_stride;
    p.coef_dev = coef_dev; p.coef_index = coef_index; p.coef_host = coef_host; p.mask_relu = mask_relu; p.accumulate = accumulate;
    RETURN_BE(k_cos(p, stream));
}

static void std_params(I2VStdParams& p, const float* a, int64_t a_stride, int64_t D, int frames, void* scratch) {
    memset(&p, 0, sizeof p);
    p.a = a; p.a_nstride = a_stride; p.D = D; p.N = frames; p.nblk = cos_nblk(D);
    // scratch layout: [2] sums, then the per-block partials
    p.sums = (double*)scratch; p.partial = (double*)scratch + 2;
}

extern "C" int i2v_std_reduce_f32(const float* a, int64_t a_stride, int64_t D, int frames, void* scratch, void* stream) {
    BAD_ARG_IF(!a || !scratch || D <= 0 || frames <= 0);
    I2VStdParams p; std_params(p, a, a_stride, D, frames, scratch);
    RETURN_BE(k_std_reduce(p, stream));
}

extern "C" int i2v_std_grad_f32(const float* a, int64_t a_stride, int64_t D, int frames, int64_t total_count,
                                int mask_relu, int accumulate, float* std_out, float* grad, int64_t grad_stride,
                                void* scratch, void* stream) {
    BAD_ARG_IF(!a || !std_out || !grad || !scratch || D <= 0 || frames <= 0 || total_count < 2);
    I2VStdParams p; std_params(p, a, a_stride, D, frames, scratch);
    p.total_count = (double)total_count; p.std_out = std_out; p.grad = grad; p.grad_nstride = grad_stride;
    p.mask_relu = mask_relu; p.accumulate = accumulate;
    RETURN_BE(k_std_grad(p, stream));
}

extern "C" int i2v_std_fwd_bwd_f32(const float* a, int64_t a_stride, int64_t D, int frames, int mask_relu,
                                   int accumulate, float* std_out, float* grad, int64_t grad_stride,
                                   void* scratch, void* stream) {
    BAD_ARG_IF(!a || !std_out || !grad || !scratch || D <= 0 || frames <= 0 || (int64_t)frames * D < 2, " (at least two elements)");
    if (i2v_std_reduce_f32(a, a_stride, D, frames, scratch, stream)) return 1;
    return i2v_std_grad_f32(a, a_stride, D, frames, (int64_t)frames * D, mask_relu, accumulate, std_out, grad,
                            grad_stride, scratch, stream);
}

extern "C" int i2v_adam_step_f32(float* delta, float* m, float* v, const float* gx, const float* u,
                                 int64_t frames, int hw, float eps, double lr, double beta1, double beta2,
                                 double adam_eps, int step_t, void* stream) {
    BAD_ARG_IF(!delta || !m || !v || !gx || !u || frames <= 0 || hw <= 0 || step_t < 1);
    // scalar prep in double, as torch/optim/adam.py does on the host for the non-capturable path
    const double bc1 = 1.0 - pow(beta1, step_t), bc2 = 1.0 - pow(beta2, step_t);
    RETURN_BE(k_adam(delta, m, v, gx, u, frames * 3 * (int64_t)hw, hw, eps, (float)(lr / bc1), (float)sqrt(bc2),
                     (float)(1.0 - beta1), (float)beta2, (float)(1.0 - beta2), (float)adam_eps, stream));
}

extern "C" int i2v_sign_step_f32(float* adv, const float* u, const float* grad, int64_t nel, int64_t chan_stride,
                                 float step, float eps, void* stream) {
    BAD_ARG_IF(!adv || !u || !grad || nel <= 0 || chan_stride <= 0);
    RETURN_BE(k_sign_bim(adv, u, grad, nel, chan_stride, step, eps, stream));
}

extern "C" int i2v_sign_step_delta_f32(float* delta, const float* grad, int64_t nel, float step, void* stream) {
    BAD_ARG_IF(!delta || !grad || nel <= 0);
    RETURN_BE(k_sign_delta(delta, grad, nel, step, stream));
}

extern "C" int i2v_sign_step_delta_gx_f32(float* delta, const float* gx, const float* u, int64_t nel, float eps,
                                          float step, void* stream) {
    BAD_ARG_IF(!delta || !gx || !u || nel <= 0);
    RETURN_BE(k_sign_delta_gx(delta, gx, u, nel, eps, step, stream));
}

static void ilaf_params(I2VIlafParams& p, const float* a, int64_t a_stride, const float* ori, const float* adv0,
                        int64_t D, int frames, void* scratch, int frames_per_seg = 0) {
    memset(&p, 0, sizeof p);
    p.a = a; p.a_nstride = a_stride; p.ori = ori; p.adv0 = adv0; p.D = D; p.N = frames; p.nblk = cos_nblk(D);
    p.fps = frames_per_seg;
    const int nseg = frames_per_seg > 0 ? frames / frames_per_seg : 1;
    p.sums = (double*)scratch; p.partial = (double*)scratch + 2 * nseg;  // [nseg][2] sums, then the per-(frame, block) partials
}

extern "C" int i2v_ilaf_reduce_f32(const float* a, int64_t a_stride, const float* ori, const float* adv0, int64_t D,
                                   int frames, void* scratch, void* stream) {
    BAD_ARG_IF(!a || !ori || !adv0 || !scratch || D <= 0 || frames <= 0);
    I2VIlafParams p; ilaf_params(p, a, a_stride, ori, adv0, D, frames, scratch);
    RETURN_BE(k_ilaf_reduce(p, stream));
}

extern "C" int i2v_ilaf_grad_f32(const float* a, int64_t a_stride, const float* ori, const float* adv0, int64_t D,
                                 int frames, double init_norm, int mask_relu, int accumulate, float* loss_out,
                                 float* grad, int64_t grad_stride, void* scratch, void* stream) {
    BAD_ARG_IF(!a || !ori || !adv0 || !scratch || !loss_out || !grad || D <= 0 || frames <= 0 || !(init_norm > 0.0));
    I2VIlafParams p; ilaf_params(p, a, a_stride, ori, adv0, D, frames, scratch);
    p.init_norm = init_norm; p.mask_relu = mask_relu; p.accumulate = accumulate; p.loss_out = loss_out;
    p.grad = grad; p.grad_nstride = grad_stride;
    RETURN_BE(k_ilaf_grad(p, stream));
}

// K independent one-clip problems in one launch (segments of frames_per_seg frames): per-segment sums / losses; the initial
// norms come from device memory (the squared norms an initial `reduce` left), so the loop needs no read-back at all.
extern "C" size_t i2v_ilaf_scratch_bytes(int64_t D, int frames, int frames_per_seg) {
    const int nseg = frames_per_seg > 0 ? frames / frames_per_seg : 1;
    return ((size_t)2 * nseg + (size_t)2 * frames * cos_nblk(D)) * sizeof(double) + 64;
}

extern "C" int i2v_ilaf_reduce_seg_f32(const float* a, int64_t a_stride, const float* ori, const float* adv0, int64_t D,
                                       int frames, int frames_per_seg, void* scratch, void* stream) {
    BAD_ARG_IF(!a || !ori || !adv0 || !scratch || D <= 0 || frames <= 0 || frames_per_seg <= 0 || frames % frames_per_seg);
    I2VIlafParams p; ilaf_params(p, a, a_stride, ori, adv0, D, frames, scratch, frames_per_seg);
    RETURN_BE(k_ilaf_reduce(p, stream));
}

extern "C" int i2v_ilaf_grad_seg_f32(const float* a, int64_t a_stride, const float* ori, const float* adv0, int64_t D,
                                     int frames, int frames_per_seg, const double* init_sq, int mask_relu, int accumulate,
                                     float* loss_out, float* grad, int64_t grad_stride, void* scratch, void* stream) {
    BAD_ARG_IF(!a || !ori || !adv0 || !scratch || !loss_out || !grad || !init_sq || D <= 0 || frames <= 0 || frames_per_seg <= 0 || frames % frames_per_seg);
    I2VIlafParams p; ilaf_params(p, a, a_stride, ori, adv0, D, frames, scratch, frames_per_seg);
    p.init_sq = init_sq; p.mask_relu = mask_relu; p.accumulate = accumulate; p.loss_out = loss_out;
    p.grad = grad; p.grad_nstride = grad_stride;
    RETURN_BE(k_ilaf_grad(p, stream));
}

extern "C" int i2v_tap_distance_f32(const float* a, int64_t a_stride, const float* clean, int64_t D, int frames, int frames_per_seg,
                                    double coef, int mask_relu, int accumulate, float* dist_out, float* grad, int64_t grad_stride,
                                    void* scratch, void* stream) {
    BAD_ARG_IF(!a || !clean || !scratch || !dist_out || !grad || D <= 0 || frames <= 0 || frames_per_seg <= 0 || frames % frames_per_seg);
    I2VIlafParams p; ilaf_params(p, a, a_stride, clean, clean, D, frames, scratch, frames_per_seg);
    p.mode = 1; p.coef = coef; p.mask_relu = mask_relu; p.accumulate = accumulate; p.loss_out = dist_out;
    p.grad = grad; p.grad_nstride = grad_stride;
    CHECK_BE(k_ilaf_reduce(p, stream));
    RETURN_BE(k_ilaf_grad(p, stream));
}

extern "C" size_t i2v_head_scratch_bytes(int C, int clips) { return (size_t)2 * C * clips * sizeof(float) + 64; }

static void head_feature(I2VHeadParams& p, const float* a, int64_t a_stride, int C, int HW, int T, int clips, int Ctot, int c_off, void* scratch) {
    memset(&p, 0, sizeof p);
    p.a = a; p.a_nstride = a_stride; p.C = C; p.HW = HW; p.T = T; p.clips = clips; p.Ctot = Ctot; p.c_off = c_off;
    p.pooled = (float*)scratch; p.dpooled = (float*)scratch + (size_t)Ctot * clips;
}

extern "C" int i2v_head_ce_f32(const float* a, int64_t a_stride, int C, int HW, int T, int clips, const float* W, const float* bias,
                               int K, const int32_t* labels, float scale, int mask_relu, int accumulate, float* logits, float* loss_each,
                               float* grad, int64_t grad_stride, void* scratch, void* stream) {
    BAD_ARG_IF(!a || !W || !labels || !logits || !loss_each || !grad || !scratch || C <= 0 || HW <= 0 || T <= 0 || clips <= 0 || K <= 0);
    I2VHeadParams p; head_feature(p, a, a_stride, C, HW, T, clips, C, 0, scratch);
    p.K = K; p.W = W; p.bias = bias; p.labels = labels; p.scale = scale; p.logits = logits; p.loss_each = loss_each;
    p.grad = grad; p.grad_nstride = grad_stride; p.mask_relu = mask_relu; p.accumulate = accumulate; p.phase = 7;
    RETURN_BE(k_head_ce(p, stream));
}

// The same head over SEVERAL features (SlowFast pools its two pathways separately and concatenates): pool every feature into
// its columns of the Ctot-wide vector, then one logits / loss call, then every feature's gradient.  scratch >=
// i2v_head_scratch_bytes(Ctot, clips), the same block in all three.
extern "C" int i2v_head_pool_f32(const float* a, int64_t a_stride, int C, int HW, int T, int clips, int Ctot, int c_off, void* scratch,
                                 void* stream) {
    BAD_ARG_IF(!a || !scratch || C <= 0 || HW <= 0 || T <= 0 || clips <= 0 || c_off < 0 || c_off + C > Ctot);
    I2VHeadParams p; head_feature(p, a, a_stride, C, HW, T, clips, Ctot, c_off, scratch); p.phase = 1;
    RETURN_BE(k_head_ce(p, stream));
}

extern "C" int i2v_head_logits_ce_f32(int Ctot, int clips, const float* W, const float* bias, int K, const int32_t* labels, float scale,
                                      float* logits, float* loss_each, void* scratch, void* stream) {
    BAD_ARG_IF(!W || !labels || !logits || !loss_each || !scratch || Ctot <= 0 || clips <= 0 || K <= 0);
    I2VHeadParams p; head_feature(p, nullptr, 0, Ctot, 1, 1, clips, Ctot, 0, scratch);
    p.K = K; p.W = W; p.bias = bias; p.labels = labels; p.scale = scale; p.logits = logits; p.loss_each = loss_each; p.phase = 2;
    RETURN_BE(k_head_ce(p, stream));
}

extern "C" int i2v_head_grad_f32(const float* a, int64_t a_stride, int C, int HW, int T, int clips, int Ctot, int c_off, int mask_relu,
                                 int accumulate, float* grad, int64_t grad_stride, void* scratch, void* stream) {
    BAD_ARG_IF(!a || !grad || !scratch || C <= 0 || HW <= 0 || T <= 0 || clips <= 0 || c_off < 0 || c_off + C > Ctot);
    I2VHeadParams p; head_feature(p, a, a_stride, C, HW, T, clips, Ctot, c_off, scratch);
    p.grad = grad; p.grad_nstride = grad_stride; p.mask_relu = mask_relu; p.accumulate = accumulate; p.phase = 4;
    RETURN_BE(k_head_ce(p, stream));
}

extern "C" int i2v_tt_grad_mix_f32(const float* grads, float* out, const float* kernel, const int32_t* moves, int D, int64_t NC, int T, int HW,
                                  float weight, void* stream) {
    BAD_ARG_IF(!grads || !out || !kernel || !moves || D <= 0 || D > 64 || NC <= 0 || T <= 0 || HW <= 0);
    const float w1 = (float)(1.0 - (double)weight);           // python: (1 - self.weight) in double, then a float32 tensor scalar
    RETURN_BE(k_tt_grad_mix(grads, out, kernel, (const int*)moves, D, NC, T, HW, w1, weight, stream));
}

extern "C" int i2v_resample_nearest_f32(const float* src, float* dst, int64_t planes, int Hs, int Ws, int Hd, int Wd, const int32_t* map_y,
                                        const int32_t* map_x, void* stream) {
    BAD_ARG_IF(!src || !dst || !map_y || !map_x || planes <= 0 || Hs <= 0 || Ws <= 0 || Hd <= 0 || Wd <= 0);
    RETURN_BE(k_resample_nearest(src, dst, planes, Hs, Ws, Hd, Wd, map_y, map_x, stream));
}

extern "C" int i2v_resample_nearest_bwd_f32(const float* g, float* gsrc, int64_t planes, int Hd, int Wd, int Hs, int Ws, const int32_t* ylo,
                                            const int32_t* yhi, const int32_t* xlo, const int32_t* xhi, void* stream) {
    BAD_ARG_IF(!g || !gsrc || !ylo || !yhi || !xlo || !xhi || planes <= 0 || Hs <= 0 || Ws <= 0 || Hd <= 0 || Wd <= 0);
    RETURN_BE(k_resample_nearest_bwd(g, gsrc, planes, Hd, Wd, Hs, Ws, ylo, yhi, xlo, xhi, stream));
}

extern "C" int i2v_dwconv1d_f32(const float* src, float* dst, int64_t outer, int len, int64_t inner, const float* taps, int k, void* stream) {
    BAD_ARG_IF(!src || !dst || src == dst || !taps || outer <= 0 || len <= 0 || inner <= 0 || k <= 0 || k > 64 || !(k & 1), " (odd k <= 64, out of place)");
    RETURN_BE(k_dwconv1d(src, dst, outer, len, inner, taps, k, stream));
}

extern "C" int64_t i2v_grad_post_scratch_bytes(int b, int c, int f, int h, int w, int mode) {
    if (b <= 0 || c <= 0 || f <= 0 || h <= 0 || w <= 0 || mode < 0 || mode > 4) return 0;
    int64_t ge = 0; const int G = k_grad_post_groups(b, c, f, h, w, mode, &ge);
    return (int64_t)(G > 0 ? G : 1) * k_grad_post_splits(ge) * 8 + 64;
}

extern "C" int i2v_grad_post_f32(const float* g, float* momentum, float* out, int b, int c, int f, int h, int w, int frame_major, int mode,
                                 float decay, void* scratch, void* stream) {
    BAD_ARG_IF(!g || !out || g == out || b <= 0 || c <= 0 || f <= 0 || h <= 0 || w <= 0 || mode < 0 || mode > 4 || (mode > 0 && !scratch) ||
               (int64_t)b * c * f * h * w >= (1ll << 31), " (out of place, mode 0..4, < 2^31 elements)");
    RETURN_BE(k_grad_post(g, momentum, out, b, c, f, h, w, frame_major, mode, decay, (double*)scratch, stream));
}

extern "C" int64_t i2v_tap_scratch_bytes(int64_t) { return 1024 * 8 + 64; }

extern "C" int i2v_tap_perts_f32(const float* adv, const float* videos, float* out, int b, int c, int f, int h, int w, void* stream) {
    BAD_ARG_IF(!adv || !videos || !out || b <= 0 || c != 3 || f <= 0 || h <= 0 || w <= 0, " (c == 3)");
    RETURN_BE(k_tap_perts(adv, videos, out, b, c, f, h, w, stream));
}

extern "C" int i2v_tap_sign_abs_f32(const float* smooth, float* sign_out, float* reg, int64_t n, void* scratch, void* stream) {
    BAD_ARG_IF(!smooth || !sign_out || !reg || !scratch || n <= 0);
    RETURN_BE(k_tap_sign_abs(smooth, sign_out, reg, n, (double*)scratch, stream));
}

extern "C" int i2v_tap_grad_f32(const float* gx, const float* boxsign, float* out, int b, int c, int f, int h, int w, float weight, void* stream) {
    BAD_ARG_IF(!gx || !boxsign || !out || gx == out || b <= 0 || c != 3 || f <= 0 || h <= 0 || w <= 0, " (c == 3, out of place)");
    RETURN_BE(k_tap_grad(gx, boxsign, out, b, c, f, h, w, weight, stream));
}

extern "C" int i2v_aens_coeffs_f32(const float* prev, float* coeffs, float momentum, int L, void* stream) {
    BAD_ARG_IF(!prev || !coeffs || L <= 0 || L > 64);
    RETURN_BE(k_aens_coeffs(prev, coeffs, momentum, L, stream));
}

extern "C" int i2v_aens_reduce_f32(const float* cos, const float* coeffs, int L, int frames, float* feat_sum,
                                   float* weighted, void* stream) {
    BAD_ARG_IF(!cos || !coeffs || !feat_sum || !weighted || L <= 0 || frames <= 0);
    RETURN_BE(k_aens_reduce(cos, coeffs, L, frames, feat_sum, weighted, stream));
}

// The ConvNeXt block's token-major depthwise 7 x 7 launch on its own (include/i2v_convnext.h): the device kernel where the library has
// one, the scalar restatement of the same operations in the same order elsewhere.
extern "C" int i2v_convnext_dw_f32(const float* x, const float* filter, const float* bias, const float* add, float* y, int frames, int H,
                                   int W, int C, void* stream) {
    BAD_ARG_IF(!x || !filter || !y || frames <= 0 || H <= 0 || W <= 0 || C <= 0);
    I2VCnDwParams p; memset(&p, 0, sizeof p);
    p.x = x; p.w = filter; p.b = bias; p.add = add; p.y = y; p.N = frames; p.H = H; p.W = W; p.C = C;
#ifdef I2V_HAVE_CONVNEXT
    if (k_convnext_dw_plan(&p) != 0) return fail("i2v_convnext_dw_f32: the shape does not fit the launch");
    RETURN_BE(k_convnext_dw(p, stream));
#else
    (void)stream;
    if (convnext_host::plan(&p) != 0 || convnext_host::dw(p) != 0) return fail("i2v_convnext_dw_f32: the shape does not fit the launch");
    return 0;
#endif
}

// The MLP-Mixer / ResMLP token-mixing launch on its own (include/i2v_mixer.h), forward and input gradient: the device kernel where the
// library has one, the scalar restatement of the same operations in the same order elsewhere.
static int mixer_tokens_launch(const char* entry, I2VMixTokParams& p, void* stream) {
#ifdef I2V_HAVE_MIXER
    if (k_mixer_tokens_plan(&p) != 0)
        return fail("%s: bad arguments, or the (tokens + hidden) x channel-tile floats do not fit the LDS (S %d, Sh %d, C %d, tile %d)", entry,
                    p.S, p.Sh, p.C, p.ct);
    RETURN_BE(k_mixer_tokens(p, stream));
#else
    (void)stream;
    if (mixer_host::plan(&p) != 0 || mixer_host::tokens(p) != 0)
        return fail("%s: bad arguments, or the (tokens + hidden) x channel-tile floats do not fit the LDS (S %d, Sh %d, C %d, tile %d)", entry,
                    p.S, p.Sh, p.C, p.ct);
    return 0;
#endif
}

extern "C" int i2v_mixer_tokens_f32(const float* z, const float* residual, float* out, int frames, int S, int Sh, int C, const float* w1,
                                    const float* b1, const float* w2, const float* b2, const float* in_scale, const float* in_shift,
                                    const float* out_scale, int channel_tile, void* stream) {
    BAD_ARG_IF(!z || !residual || !out || !w1 || !b1 || frames <= 0 || S <= 0 || Sh < 0 || C <= 0 || C % 4 != 0 || (Sh > 0 && (!w2 || !b2)) ||
               (in_scale == nullptr) != (in_shift == nullptr));
    I2VMixTokParams p; memset(&p, 0, sizeof p);
    p.z = z; p.r = residual; p.out = out; p.wa = w1; p.ba = b1; p.wb = Sh > 0 ? w2 : nullptr; p.bb = Sh > 0 ? b2 : nullptr;
    p.in_scale = in_scale; p.in_shift = in_shift; p.out_scale = out_scale; p.F = frames; p.S = S; p.Sh = Sh; p.C = C; p.ct = channel_tile;
    return mixer_tokens_launch(__func__, p, stream);
}

extern "C" int i2v_mixer_tokens_bwd_f32(const float* z, const float* g, const float* add, float* dz, int frames, int S, int Sh, int C,
                                        const float* w1, const float* b1, const float* w2t, const float* w1t, const float* in_scale,
                                        const float* in_shift, const float* out_scale, int channel_tile, void* stream) {
    BAD_ARG_IF(!g || !dz || !w2t || frames <= 0 || S <= 0 || Sh < 0 || C <= 0 || C % 4 != 0 || (Sh > 0 && (!z || !w1 || !b1 || !w1t)) ||
               (in_scale == nullptr) != (in_shift == nullptr));
    I2VMixTokParams p; memset(&p, 0, sizeof p);
    p.z = z; p.r = g; p.add0 = add; p.out = dz; p.wa = w1; p.ba = b1; p.wb = w2t; p.wc = Sh > 0 ? w1t : nullptr;
    p.in_scale = in_scale; p.in_shift = in_shift; p.out_scale = out_scale; p.F = frames; p.S = S; p.Sh = Sh; p.C = C; p.bwd = 1;
    p.ct = channel_tile;
    return mixer_tokens_launch(__func__, p, stream);
}

// ---------------------------------------------------------------------------------------------
// The non-local block's launches and the gated add on their own (include/i2v_nl_launch.h): tests and tools
// ---------------------------------------------------------------------------------------------
static bool nl_view_ok(const i2v_nl_act& v, int count) { return v.p && v.T > 0 && v.HW > 0 && (int64_t)v.T * v.HW == count; }

extern "C" int i2v_nl_gemm_f32(const i2v_nl_gemm_desc* d, void* stream) {
    BAD_ARG_IF(!d, " (null descriptor)");
    BAD_ARG_IF(d->form < 1 || d->form > 3, " (form 1..3)");
    const int rows = d->form == 1 ? d->M : d->Cc, cols = d->form == 2 ? d->M : d->N;
    if (rows <= 0 || cols <= 0 || d->clips <= 0) return 0;
    if (d->form == 1) {
        BAD_ARG_IF(!d->D || d->Cc <= 0 || !nl_view_ok(d->A, d->M) || !nl_view_ok(d->B, d->N), " (form 1: D, channels, A of M and B of N positions)");
    } else {
        BAD_ARG_IF(!d->Din || !d->C || d->c_T <= 0 || d->c_HW <= 0 || (int64_t)d->c_T * d->c_HW != cols ||
                   !nl_view_ok(d->A, d->form == 2 ? d->N : d->M), " (forms 2 / 3: Din, A of the reduced count and C of the column count of positions)");
        BAD_ARG_IF(d->ksplit > 1 && !d->part, " (a K-split launch needs part)");
    }
    I2VAttnGemm g; memset(&g, 0, sizeof g);
    g.form = d->form; g.clips = d->clips; g.Cc = d->Cc; g.M = d->M; g.N = d->N;
    g.A.p = d->A.p; g.A.nstride = d->A.nstride; g.A.T = d->A.T; g.A.HW = d->A.HW;
    g.B.p = d->B.p; g.B.nstride = d->B.nstride; g.B.T = d->B.T; g.B.HW = d->B.HW;
    g.Cact = d->C; g.C_nstride = d->c_nstride; g.C_T = d->c_T; g.C_HW = d->c_HW;
    g.D = d->D; g.Din = d->Din; g.scale = d->scale; g.accumulate = d->accumulate; g.ksplit = d->ksplit; g.part = d->part;
    RETURN_BE(k_attn_gemm(g, stream));
}

extern "C" int i2v_nl_softmax_rows_f32(float* X, const float* P, int64_t rows, int N, int mode, void* stream) {
    BAD_ARG_IF(!X || N <= 0 || mode < 0 || mode > 1 || (mode == 1 && !P), " (mode 0, or 1 with P; N > 0)");
    if (rows <= 0) return 0;
    I2VSoftmaxRows p; memset(&p, 0, sizeof p);
    p.X = X; p.P = P; p.rows = rows; p.N = N; p.mode = mode;
    RETURN_BE(k_softmax_rows(p, stream));
}

extern "C" int i2v_nl_addmask_f32(const i2v_nl_addmask_desc* d, void* stream) {
    BAD_ARG_IF(!d, " (null descriptor)");
    BAD_ARG_IF(!d->out || d->C <= 0 || d->HW <= 0);
    if (d->N <= 0) return 0;
    BAD_ARG_IF(d->gate && (int64_t)d->gate_stride * 32 < (int64_t)d->N * d->HW, " (gate rows of at least N * HW bits)");
    I2VAddMaskParams p; memset(&p, 0, sizeof p);
    p.out = d->out; p.out_nstride = d->out_nstride;
    for (int i = 0; i < 3; ++i) { p.a[i] = d->a[i]; p.a_nstride[i] = d->a_nstride[i]; }
    p.mask = d->mask; p.mask_nstride = d->mask_nstride; p.gate = d->gate; p.gate_stride = d->gate_stride;
    p.N = d->N; p.C = d->C; p.HW = d->HW; p.gain = d->gain;
    RETURN_BE(k_addmask(p, stream));
}
