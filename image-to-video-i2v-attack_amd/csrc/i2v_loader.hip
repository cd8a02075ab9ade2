// Ragged clip transform (include/i2v_loader.h): the reference's validation transform (datasets.py:86-93) over a batch of clips
// whose frames come from a pool of distinct decoded frames, each clip with its own frame size.  The arithmetic is that of
// clip_resize_crop_kernel (i2v_kernels.hip) term for term, so the two agree bit for bit on a dense batch.
#include "../../include/i2v_loader.h"
#include "i2v_be.h"

#include <stdarg.h>

#include <vector>

namespace {

__constant__ float c_mean[3] = {0.485f, 0.456f, 0.406f};         // the same constants as i2v_kernels.hip
__constant__ float c_std[3] = {0.229f, 0.224f, 0.225f};

constexpr int kGeom = 8;             // H, W, rh, rw, crop_y, crop_x, xtab row, ytab row
constexpr int kMaxWidth = 8192;      // two staged source rows of 3 * 8192 + 32 bytes fit the 64 KB of LDS a block may take
constexpr int kLanes = 64;           // one wave per output row

int64_t row_cap_bytes(int w) { return ((int64_t)3 * w + 32 + 15) & ~(int64_t)15; }

// One wave per output row (clip bi, frame ti, row y).  The two source rows that row reads are staged into LDS with 16-byte loads
// -- only the columns between the crop window's first and last source pixel --, then every lane computes four consecutive output
// columns per pass from LDS and stores each channel as one float4 when the row allows it.  Source bytes past the pool's end are
// never read (the last chunk falls back to byte loads).
__global__ void __launch_bounds__(kLanes) clip_gather_resize_crop_kernel(const uint8_t* __restrict__ pool, int64_t pool_bytes,
                                                                         const int64_t* __restrict__ offs, const int32_t* __restrict__ geom,
                                                                         const int32_t* __restrict__ xtab, const int32_t* __restrict__ ytab,
                                                                         float* __restrict__ video, int t, int oh, int ow, int row_cap,
                                                                         int vec_store) {
    extern __shared__ uint4 lds_words[];
    uint8_t* lds = reinterpret_cast<uint8_t*>(lds_words);
    const int lane = threadIdx.x;
    const int64_t blk = blockIdx.x;
    const int y = (int)(blk % oh);
    const int64_t ft = blk / oh;                                   // bi * t + ti
    const int ti = (int)(ft % t);
    const int64_t bi = ft / t;
    const int32_t* g = geom + kGeom * bi;
    const int H = g[0], W = g[1], cy = g[4], cx = g[5];
    const int32_t* xt = xtab + 3 * (int64_t)(g[6] + cx);           // the crop window's columns
    const int32_t* ye = ytab + 3 * (int64_t)(g[7] + cy + y);
    const int sy0 = ye[0], b0 = ye[1], b1 = ye[2];
    const int sy1 = min(sy0 + 1, H - 1);
    const int sx_lo = xt[0];
    const int sx_hi = min(xt[3 * (ow - 1)] + 1, W - 1);          // tables are non-decreasing (checked by the entry)
    const int64_t frame = offs[ft];

    int skew[2];
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const int64_t s = frame + ((int64_t)(r ? sy1 : sy0) * W + sx_lo) * 3;
        const int64_t e = frame + ((int64_t)(r ? sy1 : sy0) * W + sx_hi) * 3 + 3;
        const int64_t a = s & ~(int64_t)15;
        skew[r] = (int)(s - a);
        const int chunks = (int)((e - a + 15) >> 4);
        uint8_t* dst = lds + r * row_cap;
        for (int k = lane; k < chunks; k += kLanes) {
            const int64_t p = a + 16 * (int64_t)k;
            uint4 v;
            if (p + 16 <= pool_bytes) {
                v = *reinterpret_cast<const uint4*>(pool + p);
            } else {
                uint32_t w[4] = {0, 0, 0, 0};
                for (int j = 0; j < 16; ++j)
                    if (p + j < pool_bytes) w[j >> 2] |= (uint32_t)pool[p + j] << (8 * (j & 3));
                v = make_uint4(w[0], w[1], w[2], w[3]);
            }
            *reinterpret_cast<uint4*>(dst + 16 * k) = v;
        }
    }
    __syncthreads();

    const uint8_t* r0 = lds + skew[0] - sx_lo * 3;                  // r0[sx * 3 + c] = source row sy0, column sx, channel c
    const uint8_t* r1 = lds + row_cap + skew[1] - sx_lo * 3;
    const int64_t plane = (int64_t)t * oh * ow;
    float* out = video + bi * 3 * plane + ((int64_t)ti * oh + y) * ow;
    for (int x4 = lane * 4; x4 < ow; x4 += kLanes * 4) {
        float o[3][4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int x = min(x4 + j, ow - 1);
            const int sx0 = xt[3 * x], a0 = xt[3 * x + 1], a1 = xt[3 * x + 2];
            const int sx1 = min(sx0 + 1, W - 1);
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const int S0 = r0[sx0 * 3 + c] * a0 + r0[sx1 * 3 + c] * a1;
                const int S1 = r1[sx0 * 3 + c] * a0 + r1[sx1 * 3 + c] * a1;
                const int d = (((b0 * (S0 >> 4)) >> 16) + ((b1 * (S1 >> 4)) >> 16) + 2) >> 2;
                const float v = __fdiv_rn((float)d, 255.f);
                o[c][j] = __fdiv_rn(__fsub_rn(v, c_mean[c]), c_std[c]);
            }
        }
        if (vec_store) {              // ow % 4 == 0 and a 16-byte aligned output: x4 + 3 < ow
#pragma unroll
            for (int c = 0; c < 3; ++c)
                *reinterpret_cast<float4*>(out + c * plane + x4) = make_float4(o[c][0], o[c][1], o[c][2], o[c][3]);
        } else {
#pragma unroll
            for (int c = 0; c < 3; ++c)
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (x4 + j < ow) out[c * plane + x4 + j] = o[c][j];
        }
    }
}

int api_fail(const char* fmt, ...) __attribute__((format(printf, 1, 2)));
int api_fail(const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    return i2v_api_fail(buf);
}

// every entry of tab[first, first + n) has a source index in [0, limit) and they do not decrease
bool table_ok(const int32_t* tab, int64_t first, int n, int limit) {
    int prev = 0;
    for (int i = 0; i < n; ++i) {
        const int s = tab[3 * (first + i)];
        if (s < 0 || s >= limit || s < prev) return false;
        prev = s;
    }
    return true;
}

}  // namespace

extern "C" int64_t i2v_clip_gather_scratch_bytes(int b, int t, int xtab_rows, int ytab_rows) {
    if (b < 0 || t < 0 || xtab_rows < 0 || ytab_rows < 0) return -1;
    return (int64_t)b * t * 8 + ((int64_t)b * kGeom + 3 * (int64_t)xtab_rows + 3 * (int64_t)ytab_rows) * 4;
}

extern "C" int i2v_clip_gather_resize_crop_u8_f32(const uint8_t* pool, int64_t pool_bytes, const int64_t* offsets, const int32_t* geometry,
                                                  int b, int t, const int32_t* xtab, int xtab_rows, const int32_t* ytab, int ytab_rows,
                                                  int out_h, int out_w, float* video, void* scratch, int64_t scratch_bytes, void* stream) {
    static const char* fn = "i2v_clip_gather_resize_crop_u8_f32";
    if (!pool || !offsets || !geometry || !xtab || !ytab || !video || !scratch || pool_bytes <= 0 || b <= 0 || t <= 0 || xtab_rows <= 0 ||
        ytab_rows <= 0 || out_h <= 0 || out_w <= 0)
        return api_fail("%s: bad argument", fn);
    if (reinterpret_cast<uintptr_t>(pool) % 16 || reinterpret_cast<uintptr_t>(scratch) % 16)
        return api_fail("%s: pool and scratch must be 16-byte aligned", fn);
    if ((int64_t)b * t * out_h >= (1ll << 31)) return api_fail("%s: more than 2^31 output rows", fn);
    const int64_t need = i2v_clip_gather_scratch_bytes(b, t, xtab_rows, ytab_rows);
    if (scratch_bytes < need) return api_fail("%s: scratch of %lld bytes, %lld needed", fn, (long long)scratch_bytes, (long long)need);
    int wmax = 1;
    for (int bi = 0; bi < b; ++bi) {
        const int32_t* g = geometry + kGeom * bi;
        const int H = g[0], W = g[1], rh = g[2], rw = g[3], cy = g[4], cx = g[5], xr = g[6], yr = g[7];
        if (H <= 0 || W <= 0 || W > kMaxWidth || rh <= 0 || rw <= 0)
            return api_fail("%s: clip %d: frame %d x %d resized to %d x %d (widths 1..%d)", fn, bi, H, W, rh, rw, kMaxWidth);
        if (cy < 0 || cx < 0 || (int64_t)cy + out_h > rh || (int64_t)cx + out_w > rw)
            return api_fail("%s: clip %d: crop window %d x %d at (%d, %d) outside the resized frame %d x %d", fn, bi, out_h, out_w, cy, cx, rh, rw);
        if (xr < 0 || yr < 0 || (int64_t)xr + rw > xtab_rows || (int64_t)yr + rh > ytab_rows)
            return api_fail("%s: clip %d: resize table rows [%d, %d + %d) / [%d, %d + %d) outside the tables (%d / %d rows)", fn, bi, xr, xr, rw,
                            yr, yr, rh, xtab_rows, ytab_rows);
        if (!table_ok(xtab, (int64_t)xr + cx, out_w, W) || !table_ok(ytab, (int64_t)yr + cy, out_h, H))
            return api_fail("%s: clip %d: a resize table entry of the crop window is outside the %d x %d frame or decreasing", fn, bi, H, W);
        const int64_t frame_bytes = (int64_t)H * W * 3;
        for (int ti = 0; ti < t; ++ti) {
            const int64_t o = offsets[(int64_t)bi * t + ti];
            if (o < 0 || o > pool_bytes - frame_bytes)
                return api_fail("%s: clip %d frame %d: offset %lld + %lld bytes outside the pool of %lld bytes", fn, bi, ti, (long long)o,
                                (long long)frame_bytes, (long long)pool_bytes);
        }
        if (W > wmax) wmax = W;
    }
    // the checked tables, packed: offsets (int64), geometry, xtab, ytab (int32).  A copy from pageable memory completes before
    // hipMemcpyAsync returns, so the packed host copy may go out of scope.
    std::vector<uint8_t> host((size_t)need);
    uint8_t* h = host.data();
    const size_t n_off = (size_t)b * t * 8, n_geom = (size_t)b * kGeom * 4, n_x = (size_t)xtab_rows * 12, n_y = (size_t)ytab_rows * 12;
    memcpy(h, offsets, n_off);
    memcpy(h + n_off, geometry, n_geom);
    memcpy(h + n_off + n_geom, xtab, n_x);
    memcpy(h + n_off + n_geom + n_x, ytab, n_y);
    hipError_t e = hipMemcpyAsync(scratch, h, (size_t)need, hipMemcpyHostToDevice, (hipStream_t)stream);
    if (e != hipSuccess) return api_fail("%s: staging the tables: %s", fn, hipGetErrorString(e));
    uint8_t* d = static_cast<uint8_t*>(scratch);
    const int row_cap = (int)row_cap_bytes(wmax);
    const int vec_store = out_w % 4 == 0 && reinterpret_cast<uintptr_t>(video) % 16 == 0;
    hipLaunchKernelGGL(clip_gather_resize_crop_kernel, dim3((unsigned)((int64_t)b * t * out_h)), dim3(kLanes), 2 * row_cap, (hipStream_t)stream,
                       pool, pool_bytes, reinterpret_cast<const int64_t*>(d), reinterpret_cast<const int32_t*>(d + n_off),
                       reinterpret_cast<const int32_t*>(d + n_off + n_geom), reinterpret_cast<const int32_t*>(d + n_off + n_geom + n_x), video, t,
                       out_h, out_w, row_cap, vec_store);
    e = hipGetLastError();
    if (e != hipSuccess) return api_fail("%s: launch: %s", fn, hipGetErrorString(e));
    return 0;
}
