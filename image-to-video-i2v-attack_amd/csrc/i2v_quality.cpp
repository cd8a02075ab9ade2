// The C entries of the 8-bit export and the quality launches (include/i2v_quality.h): argument checks in front of the launches of
// i2v_quality.hip -- without -DI2V_HAVE_QUALITY (the host simulation's one-file build) their scalar twins, i2v_quality_host.h.
#include "../../include/i2v_quality.h"
#ifdef I2V_HAVE_QUALITY
#include <stdio.h>

#include "i2v_kernels.h"          // i2v_api_fail
#include "i2v_quality_kernels.h"
#else
#include "i2v_quality_host.h"     // (the host simulation's one-file build: the launches as scalar code)
#endif

namespace {

int ql_refuse(const char* who, const char* why) {
    char buf[256];
    snprintf(buf, sizeof buf, "%s: hipErrorInvalidValue: %s", who, why);
    return i2v_api_fail(buf);
}

int ql_quality(const char* who, QlClips p, int64_t scratch_bytes, void* stream) {
    if (const char* why = ql_quality_refusal(p, scratch_bytes < 0 ? 0 : (size_t)scratch_bytes)) return ql_refuse(who, why);
    return ql_clip_quality(p, (hipStream_t)stream);
}

}  // namespace

extern "C" int i2v_clip_to_u8(const float* video, const uint8_t* ref, int levels, uint8_t* frames, int b, int t, int h, int w, void* stream) {
    QlExport p{video, ref, frames, levels > 255 ? 255 : levels, b, t, h, w};
    if (const char* why = ql_export_refusal(p)) return ql_refuse("i2v_clip_to_u8", why);
    return ql_clip_to_u8(p, (hipStream_t)stream);
}

extern "C" size_t i2v_clip_quality_scratch_bytes(int64_t frames, int h, int w) {
    if (frames <= 0 || h < QL_TAPS || w < QL_TAPS || frames * ql_tiles(h, w) >= (1ll << 40)) return 0;
    return ql_scratch_bytes(frames, h, w);
}

extern "C" void i2v_clip_quality_tile(int* rows, int* cols) {
    if (rows) *rows = QL_TR;
    if (cols) *cols = QL_TC;
}

extern "C" int i2v_clip_quality_u8(const uint8_t* a, const uint8_t* b, double* out, int64_t frames, int h, int w, void* scratch,
                                   int64_t scratch_bytes, void* stream) {
    QlClips p{a, b, out, (double*)scratch, frames, 1, h, w, 1};
    return ql_quality("i2v_clip_quality_u8", p, scratch_bytes, stream);
}

extern "C" int i2v_clip_quality_f32(const float* a, const float* b, double* out, int clips, int t, int h, int w, void* scratch,
                                    int64_t scratch_bytes, void* stream) {
    QlClips p{a, b, out, (double*)scratch, (int64_t)clips * t, t, h, w, 0};
    if (clips <= 0) return ql_refuse("i2v_clip_quality_f32", "clips and frames must be positive");
    return ql_quality("i2v_clip_quality_f32", p, scratch_bytes, stream);
}
