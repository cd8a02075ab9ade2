// TEST INFRASTRUCTURE -- scalar host implementation of csrc/i2v_kernels.h.
//
// Linked with the engine units (csrc/i2v_engine.cpp, i2v_pack.cpp, i2v_plan.cpp, i2v_tune.cpp, i2v_run.cpp,
// i2v_loop_api.cpp) into tests/hostsim/libi2v_hostsim.so so that the graph planner
// (weight packing, k-tables, stride-parity classes, addend/mask fusion, arena layout) can be
// checked against the oracle WITHOUT a GPU (`pytest -m "not gpu"`).  It is never loaded by the
// product package: `i2v_amd.lib` only accepts a library whose `i2v_backend()` is "hip:gfx950".
// Every routine is the literal definition of the launch-parameter structs in i2v_params.h.
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <limits>
#include <vector>

#include "../../image-to-video-i2v-attack_amd/csrc/i2v_kernels.h"

static const float MEAN[3] = {0.485f, 0.456f, 0.406f};
static const float STD[3] = {0.229f, 0.224f, 0.225f};

const char* be_name() { return "hostsim"; }
int be_set_device(int) { return 0; }
void* be_malloc(size_t b) { return malloc(b ? b : 16); }
void be_free(void* p) { free(p); }
int be_h2d(void* d, const void* s, size_t b) { memcpy(d, s, b); return 0; }
int be_d2d_2d(void* d, size_t dp, const void* s, size_t sp, size_t w, size_t rows, i2v_stream_t) {
    for (size_t r = 0; r < rows; ++r) memcpy((char*)d + r * dp, (const char*)s + r * sp, w);
    return 0;
}
int be_memset0(void* p, size_t b, i2v_stream_t) { memset(p, 0, b); return 0; }
const char* be_error() { return nullptr; }
static long long g_fastblock_launches = 0;
long long be_stat(const char* name) { return !strcmp(name, "fastblock_launches") ? g_fastblock_launches : -1; }
void* be_event_create() { return malloc(8); }
void be_event_destroy(void* e) { free(e); }
int be_event_record(void*, i2v_stream_t) { return 0; }
int be_event_elapsed_ms(void*, void*, float* ms) { *ms = 0.f; return 0; }
int be_stream_sync(i2v_stream_t) { return 0; }
int be_device_sync() { return 0; }
i2v_stream_t be_stream_create() { return malloc(8); }       // (the host simulation runs every launch synchronously, in ISSUE order: a hoisted launch really runs early)
void be_stream_destroy(i2v_stream_t s) { free(s); }
int be_stream_wait_event(i2v_stream_t, void*) { return 0; }
int cos_nblk(int64_t D) { return (int)std::min<int64_t>(64, std::max<int64_t>(1, D / 4096)); }

int k_conv_candidates(const I2VConvParams&, int* out) { out[0] = 0; return 1; }

// the fused pair on the host: the two convolutions one after the other (the intermediate IS written here; the device kernel keeps
// it in LDS -- same values either way); eligibility is the shared structural rule of i2v_kernels.h (no halo staging here) and never chosen without the device autotuner
int k_conv(const I2VConvParams& p, i2v_stream_t);
int k_conv_fusable(const I2VConvParams& a, const I2VConvParams& b) { return i2v_conv_pair_fusable(a, b) ? 1 : 0; }
int k_conv_fused(const I2VConvParams& a, const I2VConvParams& b, int, i2v_stream_t s) {
    if (k_conv(a, s) || k_conv(b, s)) return 1;
    // the device kernel never stores the intermediate: poison it here, so that any reader the planner overlooked shows up as NaN
    // in the CPU tests instead of passing on values the GPU would not have
    for (int64_t f = 0; f < (int64_t)a.N / a.Tg * a.To; ++f)
        std::fill(a.dst + f * a.dst_nstride, a.dst + f * a.dst_nstride + (int64_t)a.Cd * a.Ho * a.Wo, std::numeric_limits<float>::quiet_NaN());
    return 0;
}
// the fused fast-pathway block on the host: its convolutions one after the other (the device kernel keeps the intermediates in LDS /
// registers -- same values either way), then the intermediates POISONED: a reader the planner overlooked shows up as NaN here instead
// of passing on values the GPU would not have.  Forward order: a, b, [d], c; backward: a, b.
int k_fastblock(const I2VConvParams& a, const I2VConvParams& b, const I2VConvParams* c, const I2VConvParams* d, i2v_stream_t s) {
    if (i2v_fastblock_rows(a, b, c, d) <= 0) return 1;
    ++g_fastblock_launches;
    if (k_conv(a, s) || k_conv(b, s) || (d && k_conv(*d, s)) || (c && k_conv(*c, s))) return 1;
    auto poison = [](const I2VConvParams& q) {
        for (int64_t f = 0; f < (int64_t)q.N / q.Tg * q.To; ++f)
            std::fill(q.dst + f * q.dst_nstride, q.dst + f * q.dst_nstride + (int64_t)q.Cd * q.Ho * q.Wo, std::numeric_limits<float>::quiet_NaN());
    };
    poison(a);
    if (c) poison(b);
    if (d) poison(*d);
    return 0;
}
int k_conv(const I2VConvParams& p, i2v_stream_t) {
    if (!p.temporal) {      // image variant of the kernel: the temporal fields are ignored (a launch that needs them
        I2VConvParams q = p; // but is not flagged must therefore FAIL the planner tests, as it would on the GPU)
        q.temporal = 1; q.Tg = q.Ts = q.To = q.st = q.ost = 1; q.ot0 = 0; q.blkt = 1; q.oct = 1;
        std::vector<I2VKEntry> kt(p.ktab, p.ktab + (p.Kpad ? p.Kpad : 0));
        for (auto& e : kt) e.valid &= 1;
        q.ktab = kt.data();
        return k_conv(q, nullptr);
    }
    for (int ng = 0; ng < p.N; ++ng) {
        // grid frame (clip, tg) reads source frame clip*Ts + tg*st + dt and writes frame clip*To + tg*ost + ot0 (+ class)
        const int clip = ng / p.Tg, tg = ng % p.Tg, t0 = tg * p.st;
        const size_t nsrc = (size_t)clip * p.Ts + t0;
        for (int i = 0; i < p.Hg; ++i)
            for (int j = 0; j < p.Wg; ++j) {
                int oh = i * p.osh + p.oh0, ow = j * p.osw + p.ow0;
                if (p.blk <= 1 && (oh >= p.Ho || ow >= p.Wo)) continue;
                for (int cd = 0; cd < p.Cd; ++cd) {
                    float acc = 0.f;
                    for (int k = 0; k < p.Kpad; ++k) {
                        const I2VKEntry& e = p.ktab[k];
                        if (!(e.valid & 1)) continue;
                        const int dt = e.valid >> 1;
                        int hs = i * p.sh + e.dh, ws = j * p.sw + e.dw;
                        if (hs < 0 || hs >= p.Hs || ws < 0 || ws >= p.Ws || t0 + dt < 0 || t0 + dt >= p.Ts) continue;
                        float xv = p.src[(int64_t)(nsrc + dt) * p.src_nstride + e.chan_off + (size_t)hs * p.Ws + ws];
                        if (p.pre_scale) { xv = fmaf(xv, p.pre_scale[k], p.pre_shift[k]); xv = xv > 0.f ? xv : 0.f; }
                        acc = fmaf(p.wp[(size_t)k * p.Cdpad + cd], xv, acc);      // one fused multiply-add per K row, in packed-K order: what an fp32 MFMA chain computes
                    }
                    if (p.blk > 1 || p.blkt > 1) {            // class-packed Cd (image gradient; frame-paired forward stems: blk = 1)
                        int Creal = p.Cd / (p.blkt * p.blk * p.blk), cls3 = cd / Creal, c = cd % Creal;
                        int ct = cls3 / (p.blk * p.blk), cls = cls3 % (p.blk * p.blk);
                        int bh = i * p.osh + cls / p.blk + p.oh0, bw = j * p.osw + cls % p.blk + p.ow0;
                        int ot = tg * p.ost + p.ot0 + ct * p.oct;
                        if (bh >= p.Ho || bw >= p.Wo || ot >= p.To) continue;
                        size_t n = (size_t)clip * p.To + ot;
                        size_t o = (size_t)c * p.Ho * p.Wo + (size_t)bh * p.Wo + bw;
                        float v = acc;
                        if (p.shift) v += p.shift[c];
                        if (p.add1) v += p.add1[(size_t)n * p.add1_nstride + o];
                        if (p.relu) v = v > 0.f ? v : 0.f;
                        if (p.mask && !(p.mask[(size_t)n * p.mask_nstride + o] > 0.f)) v = 0.f;
                        p.dst[(size_t)n * p.dst_nstride + o] = v;
                        continue;
                    }
                    const int ot = tg * p.ost + p.ot0;
                    if (ot >= p.To) continue;
                    const size_t n = (size_t)clip * p.To + ot;
                    size_t oidx = (size_t)cd * p.Ho * p.Wo + (size_t)oh * p.Wo + ow;
                    float v = acc;
                    if (p.gate_scale) {     // pre-activation gate: applies to THIS contribution only, before the adds
                        float m = fmaf(p.mask[(size_t)n * p.mask_nstride + oidx], p.gate_scale[cd], p.gate_shift[cd]);
                        if (!(m > 0.f)) v = 0.f;
                    }
                    if (p.shift) v += p.shift[cd];
                    if (p.add0) {
                        if (p.add0_stride == 1) v += p.add0[(size_t)n * p.add0_nstride + oidx];
                        else if (oh % p.add0_stride == 0 && ow % p.add0_stride == 0 &&
                                 oh / p.add0_stride < p.add0_H && ow / p.add0_stride < p.add0_W)
                            v += p.add0[(size_t)n * p.add0_nstride + (size_t)cd * p.add0_H * p.add0_W +
                                        (size_t)(oh / p.add0_stride) * p.add0_W + ow / p.add0_stride];
                    }
                    if (p.add1) v += p.add1[(size_t)n * p.add1_nstride + oidx];
                    if (p.relu) v = v > 0.f ? v : 0.f;
                    const size_t bit = (size_t)n * p.Ho * p.Wo + (size_t)oh * p.Wo + ow;     // element's bit in a gate row of channel cd
                    if (p.gate) {
                        const size_t b = (size_t)p.gate_pix0 + bit;
                        if (!((p.gate[(size_t)cd * p.gate_stride + (b >> 5)] >> (b & 31)) & 1u)) v = 0.f;
                    } else if (p.mask && !p.gate_scale && !(p.mask[(size_t)n * p.mask_nstride + oidx] > 0.f)) v = 0.f;
                    p.dst[(size_t)n * p.dst_nstride + oidx] = v;
                    if (p.gate_out) {       // 1-bit ReLU gate of the value just stored
                        const size_t b = (size_t)p.gate_out_pix0 + bit;
                        uint32_t& w = p.gate_out[(size_t)cd * p.gate_out_stride + (b >> 5)];
                        w = v > 0.f ? (w | (1u << (b & 31))) : (w & ~(1u << (b & 31)));
                    }
                }
            }
    }
    return 0;
}

int k_pool_fwd(const I2VPoolParams& p, i2v_stream_t) {
    for (int n = 0; n < p.N; ++n)
        for (int c = 0; c < p.C; ++c) {
            const float* pl = p.x + (size_t)n * p.x_nstride + (size_t)c * p.Hs * p.Ws;
            for (int ho = 0; ho < p.Ho; ++ho)
                for (int wo = 0; wo < p.Wo; ++wo) {
                    // first maximum in scan order (ATen max_pool2d: update on `val > max || isnan(val)`)
                    int best = -1; float bv = 0.f;
                    for (int r = 0; r < p.k; ++r) {
                        int h = ho * p.stride - p.pad + r; if (h < 0 || h >= p.Hs) continue;
                        for (int s = 0; s < p.k; ++s) {
                            int w = wo * p.stride - p.pad + s; if (w < 0 || w >= p.Ws) continue;
                            float v = pl[h * p.Ws + w];
                            if (best < 0 || v > bv || v != v) { bv = v; best = r * p.k + s; }
                        }
                    }
                    p.y[(size_t)n * p.y_nstride + ((size_t)c * p.Ho + ho) * p.Wo + wo] = bv;
                    p.idx[(((size_t)n * p.C + c) * p.Ho + ho) * p.Wo + wo] = (uint8_t)best;
                }
        }
    return 0;
}

int k_pool_bwd(const I2VPoolParams& p, i2v_stream_t) {
    for (int n = 0; n < p.N; ++n)
        for (int c = 0; c < p.C; ++c) {
            const float* pl = p.x + (size_t)n * p.x_nstride + (size_t)c * p.Hs * p.Ws;
            float* g = p.gx + (size_t)n * p.gx_nstride + (size_t)c * p.Hs * p.Ws;
            for (int i = 0; i < p.Hs * p.Ws; ++i) g[i] = 0.f;
            for (int ho = 0; ho < p.Ho; ++ho)
                for (int wo = 0; wo < p.Wo; ++wo) {
                    int code = p.idx[(((size_t)n * p.C + c) * p.Ho + ho) * p.Wo + wo];
                    int h = ho * p.stride - p.pad + code / p.k, w = wo * p.stride - p.pad + code % p.k;
                    g[h * p.Ws + w] += p.y[(size_t)n * p.y_nstride + ((size_t)c * p.Ho + ho) * p.Wo + wo];
                }
            if (p.mask_relu) for (int i = 0; i < p.Hs * p.Ws; ++i) if (!(pl[i] > 0.f)) g[i] = 0.f;
        }
    return 0;
}

int k_pool3d_fwd(const I2VPoolParams& p, i2v_stream_t) {
    for (int n = 0; n < p.N; ++n) {
        const int clip = n / p.To, to = n % p.To;
        for (int c = 0; c < p.C; ++c) for (int ho = 0; ho < p.Ho; ++ho) for (int wo = 0; wo < p.Wo; ++wo) {
            int best = -1; float bv = 0.f;
            for (int q = 0; q < p.kt; ++q) {
                int ts = to * p.stride_t - p.pad_t + q; if (ts < 0 || ts >= p.Ts) continue;
                const float* pl = p.x + ((size_t)clip * p.Ts + ts) * p.x_nstride + (size_t)c * p.Hs * p.Ws;
                for (int r = 0; r < p.k; ++r) {
                    int h = ho * p.stride - p.pad + r; if (h < 0 || h >= p.Hs) continue;
                    for (int s = 0; s < p.k; ++s) {
                        int w = wo * p.stride - p.pad + s; if (w < 0 || w >= p.Ws) continue;
                        float v = pl[h * p.Ws + w];
                        if (best < 0 || v > bv || v != v) { bv = v; best = (q * p.k + r) * p.k + s; }
                    }
                }
            }
            p.y[(size_t)n * p.y_nstride + ((size_t)c * p.Ho + ho) * p.Wo + wo] = bv;
            p.idx[(((size_t)n * p.C + c) * p.Ho + ho) * p.Wo + wo] = (uint8_t)best;
        }
    }
    return 0;
}

int k_pool3d_bwd(const I2VPoolParams& p, i2v_stream_t) {
    const int clips = p.N / p.To;
    for (int ns = 0; ns < clips * p.Ts; ++ns) for (int c = 0; c < p.C; ++c) {
        float* g = p.gx + (size_t)ns * p.gx_nstride + (size_t)c * p.Hs * p.Ws;
        for (int i = 0; i < p.Hs * p.Ws; ++i) g[i] = 0.f;
    }
    for (int n = 0; n < p.N; ++n) {
        const int clip = n / p.To, to = n % p.To;
        for (int c = 0; c < p.C; ++c) for (int ho = 0; ho < p.Ho; ++ho) for (int wo = 0; wo < p.Wo; ++wo) {
            int code = p.idx[(((size_t)n * p.C + c) * p.Ho + ho) * p.Wo + wo];
            int q = code / (p.k * p.k), r = code / p.k % p.k, s = code % p.k;
            int ts = to * p.stride_t - p.pad_t + q, h = ho * p.stride - p.pad + r, w = wo * p.stride - p.pad + s;
            p.gx[((size_t)clip * p.Ts + ts) * p.gx_nstride + ((size_t)c * p.Hs + h) * p.Ws + w] +=
                p.y[(size_t)n * p.y_nstride + ((size_t)c * p.Ho + ho) * p.Wo + wo];
        }
    }
    if (p.mask_relu)
        for (int ns = 0; ns < clips * p.Ts; ++ns) for (int c = 0; c < p.C; ++c) for (int i = 0; i < p.Hs * p.Ws; ++i) {
            size_t o = (size_t)c * p.Hs * p.Ws + i;
            if (!(p.x[(size_t)ns * p.x_nstride + o] > 0.f)) p.gx[(size_t)ns * p.gx_nstride + o] = 0.f;
        }
    return 0;
}

int k_avgpool_fwd(const I2VPoolParams& p, i2v_stream_t) {
    const float inv = 1.f / (float)(p.k * p.k);
    for (int n = 0; n < p.N; ++n) for (int c = 0; c < p.C; ++c) for (int ho = 0; ho < p.Ho; ++ho) for (int wo = 0; wo < p.Wo; ++wo) {
        float s = 0.f;
        for (int r = 0; r < p.k; ++r) for (int q = 0; q < p.k; ++q)
            s += p.x[(size_t)n * p.x_nstride + ((size_t)c * p.Hs + ho * p.stride + r) * p.Ws + wo * p.stride + q];
        p.y[(size_t)n * p.y_nstride + ((size_t)c * p.Ho + ho) * p.Wo + wo] = s * inv;
    }
    return 0;
}

// every window covering the element, in (output row, output column) order, then one multiplication by 1 / k^2; the ReLU gate of the
// averaged tensor where this launch finalises its gradient (mask_relu)
int k_avgpool_bwd(const I2VPoolParams& p, i2v_stream_t) {
    const float inv = 1.f / (float)(p.k * p.k);
    for (int n = 0; n < p.N; ++n) for (int c = 0; c < p.C; ++c) for (int h = 0; h < p.Hs; ++h) for (int w = 0; w < p.Ws; ++w) {
        float g = 0.f; bool first = true;
        if (!p.mask_relu || p.x[(size_t)n * p.x_nstride + ((size_t)c * p.Hs + h) * p.Ws + w] > 0.f)
            for (int ho = std::max(0, (h - p.k) / p.stride); ho <= std::min(h / p.stride, p.Ho - 1); ++ho)       // (a loose range: the test below decides)
            for (int wo = std::max(0, (w - p.k) / p.stride); wo <= std::min(w / p.stride, p.Wo - 1); ++wo) {
                if (h < ho * p.stride || h >= ho * p.stride + p.k || w < wo * p.stride || w >= wo * p.stride + p.k) continue;
                const float v = p.y[(size_t)n * p.y_nstride + ((size_t)c * p.Ho + ho) * p.Wo + wo];
                g = first ? v : g + v; first = false;
            }
        p.gx[(size_t)n * p.gx_nstride + ((size_t)c * p.Hs + h) * p.Ws + w] = first ? 0.f : g * inv;
    }
    return 0;
}

int k_addmask(const I2VAddMaskParams& p, i2v_stream_t) {
    size_t plane = (size_t)p.C * p.HW;
    for (int n = 0; n < p.N; ++n)
        for (size_t i = 0; i < plane; ++i) {
            float v = 0.f;
            for (int a = 0; a < 3; ++a) if (p.a[a]) v += p.a[a][(size_t)n * p.a_nstride[a] + i];
            if (p.gate) {
                const size_t c = i / p.HW, bit = (size_t)n * p.HW + (i - c * p.HW);
                if (!((p.gate[c * p.gate_stride + (bit >> 5)] >> (bit & 31)) & 1u)) v = 0.f;
            } else if (p.mask && !(p.mask[(size_t)n * p.mask_nstride + i] > 0.f)) v = 0.f;
            if (p.gain != 0.f) { volatile float w = p.gain * v; v = w; }
            p.out[(size_t)n * p.out_nstride + i] = v;
        }
    return 0;
}

// Cosine similarity: the SAME reduction tree as the device kernels (cos_reduce_kernel / cos_grad_kernel) -- per-thread fp32
// partial sums over the float4-strided slices of a block, 64-lane shuffle-down trees, four wave results combined as
// (r0+r1)+(r2+r3), then the per-block partials summed in double over a 64-lane tree -- so that a whole attack run on this
// backend is bit-identical to the run on the GPU (tests/test_gpu_video.py).  volatile keeps the host compiler from
// re-associating or contracting.
static float tree64(const float* v) {          // lane 0 of: for o in 32,16,..,1: v[l] += v[l+o]
    volatile float t[64];
    for (int l = 0; l < 64; ++l) t[l] = v[l];
    for (int o = 32; o > 0; o >>= 1) for (int l = 0; l < o; ++l) t[l] = t[l] + t[l + o];
    return t[0];
}
static double tree64d(const double* v) {
    volatile double t[64];
    for (int l = 0; l < 64; ++l) t[l] = v[l];
    for (int o = 32; o > 0; o >>= 1) for (int l = 0; l < o; ++l) t[l] = t[l] + t[l + o];
    return t[0];
}

int k_cos(const I2VCosParams& p, i2v_stream_t) {
    const bool vec = ((p.a_nstride | p.b_nstride) & 3) == 0 && (((uintptr_t)p.a | (uintptr_t)p.b) & 15) == 0;      // as the device: strides AND bases
    std::vector<float> part((size_t)p.N * p.nblk * 4, 0.f);
    for (int n = 0; n < p.N; ++n) {
        const float* a = p.a + (size_t)n * p.a_nstride; const float* b = p.b + (size_t)n * p.b_nstride;
        for (int blk = 0; blk < p.nblk; ++blk) {
            const int64_t chunk = ((p.D + p.nblk - 1) / p.nblk + 3) & ~(int64_t)3;
            const int64_t lo = blk * chunk, hi = (lo + chunk < p.D) ? lo + chunk : p.D;
            float dot[256], aa[256], bb[256];
            for (int t = 0; t < 256; ++t) {
                volatile float d = 0.f, x2 = 0.f, y2 = 0.f;
                auto one = [&](int64_t i) {
                    volatile float m;
                    m = a[i] * b[i]; d = d + m; m = a[i] * a[i]; x2 = x2 + m; m = b[i] * b[i]; y2 = y2 + m;
                };
                if (vec) {
                    const int64_t hi4 = lo + ((hi - lo) & ~(int64_t)3);
                    for (int64_t i = lo + t * 4; i < hi4; i += 1024) {
                        volatile float s, m;
                        s = a[i] * b[i]; m = a[i + 1] * b[i + 1]; s = s + m; m = a[i + 2] * b[i + 2]; s = s + m; m = a[i + 3] * b[i + 3]; s = s + m; d = d + s;
                        s = a[i] * a[i]; m = a[i + 1] * a[i + 1]; s = s + m; m = a[i + 2] * a[i + 2]; s = s + m; m = a[i + 3] * a[i + 3]; s = s + m; x2 = x2 + s;
                        s = b[i] * b[i]; m = b[i + 1] * b[i + 1]; s = s + m; m = b[i + 2] * b[i + 2]; s = s + m; m = b[i + 3] * b[i + 3]; s = s + m; y2 = y2 + s;
                    }
                    for (int64_t i = hi4 + t; i < hi; i += 256) one(i);
                } else {
                    for (int64_t i = lo + t; i < hi; i += 256) one(i);
                }
                dot[t] = d; aa[t] = x2; bb[t] = y2;
            }
            float* o = &part[((size_t)n * p.nblk + blk) * 4];
            volatile float r[3][4];
            for (int w = 0; w < 4; ++w) { r[0][w] = tree64(dot + 64 * w); r[1][w] = tree64(aa + 64 * w); r[2][w] = tree64(bb + 64 * w); }
            for (int q = 0; q < 3; ++q) { volatile float u = r[q][0] + r[q][1], v = r[q][2] + r[q][3]; o[q] = u + v; }
        }
    }
    for (int n = 0; n < p.N; ++n) {
        double d[64] = {0}, x[64] = {0}, y[64] = {0};
        for (int t = 0; t < 64 && t < p.nblk; ++t) { const float* o = &part[((size_t)n * p.nblk + t) * 4]; d[t] = o[0]; x[t] = o[1]; y[t] = o[2]; }
        const double fd = tree64d(d), fx = tree64d(x), fy = tree64d(y);
        const double n1 = std::max(sqrt(fx), 1e-8), n2 = std::max(sqrt(fy), 1e-8);
        volatile double nn = n1 * n2;
        const double cs = fd / nn;
        p.cos_out[n] = (float)cs;
        double coef = (double)p.coef_host;
        if (p.coef_dev) coef *= (double)p.coef_dev[p.coef_index];
        volatile double c1 = coef / nn;
        volatile double c2a = coef * cs, n11 = n1 * n1;
        volatile double c2 = c2a / n11;
        const float* a = p.a + (size_t)n * p.a_nstride; const float* b = p.b + (size_t)n * p.b_nstride;
        float* g = p.grad + (size_t)n * p.grad_nstride;
        for (int64_t i = 0; i < p.D; ++i) {
            volatile double t1 = c1 * (double)b[i], t2 = c2 * (double)a[i];
            float v = (float)(t1 - t2);
            if (p.mask_relu && !(a[i] > 0.f)) v = 0.f;
            g[i] = p.accumulate ? g[i] + v : v;
        }
    }
    return 0;
}

// Whole-tensor reductions (DR loss, ILAF loss): the device kernels' trees replayed -- per-thread double sums over a block's
// slice with stride 256, 64-lane shuffle-down trees, (r0+r1)+(r2+r3), then the block partials summed the same way.
static void block_sums2(const std::vector<double>& t0, const std::vector<double>& t1, double* o0, double* o1) {
    volatile double r0[4], r1[4];
    for (int w = 0; w < 4; ++w) { r0[w] = tree64d(t0.data() + 64 * w); r1[w] = tree64d(t1.data() + 64 * w); }
    volatile double a = r0[0] + r0[1], b = r0[2] + r0[3]; *o0 = a + b;
    volatile double c = r1[0] + r1[1], d = r1[2] + r1[3]; *o1 = c + d;
}
static void finish_sums2(const std::vector<double>& partial, int np, double* sums) {
    std::vector<double> t0(256, 0.0), t1(256, 0.0);
    for (int t = 0; t < 256; ++t) {
        volatile double s = 0, q = 0;
        for (int i = t; i < np; i += 256) { s = s + partial[2 * i]; q = q + partial[2 * i + 1]; }
        t0[t] = s; t1[t] = q;
    }
    block_sums2(t0, t1, &sums[0], &sums[1]);
}

int k_std_reduce(const I2VStdParams& p, i2v_stream_t) {
    std::vector<double> partial((size_t)p.N * p.nblk * 2);
    for (int n = 0; n < p.N; ++n) for (int blk = 0; blk < p.nblk; ++blk) {
        const int64_t chunk = (p.D + p.nblk - 1) / p.nblk, lo = blk * chunk, hi = (lo + chunk < p.D) ? lo + chunk : p.D;
        const float* a = p.a + (size_t)n * p.a_nstride;
        std::vector<double> t0(256), t1(256);
        for (int t = 0; t < 256; ++t) {
            volatile double s = 0, ss = 0;
            for (int64_t i = lo + t; i < hi; i += 256) { const double v = a[i]; volatile double v2 = v * v; s = s + v; ss = ss + v2; }
            t0[t] = s; t1[t] = ss;
        }
        block_sums2(t0, t1, &partial[((size_t)n * p.nblk + blk) * 2], &partial[((size_t)n * p.nblk + blk) * 2 + 1]);
    }
    finish_sums2(partial, p.N * p.nblk, p.sums);
    return 0;
}

int k_std_grad(const I2VStdParams& p, i2v_stream_t) {
    const double s = p.sums[0], ss = p.sums[1], cnt = p.total_count;
    volatile double mu = s / cnt;
    volatile double cm = cnt * mu, cmm = cm * mu, num = ss - cmm, var0 = num / (cnt - 1.0);
    const double var = var0 > 0.0 ? var0 : 0.0;
    const double sd = sqrt(var);
    p.std_out[0] = (float)sd;
    volatile double den = (cnt - 1.0) * sd;
    volatile double inv = 1.0 / den;
    for (int n = 0; n < p.N; ++n) {
        const float* a = p.a + (size_t)n * p.a_nstride; float* g = p.grad + (size_t)n * p.grad_nstride;
        for (int64_t i = 0; i < p.D; ++i) {
            volatile double c = (double)a[i] - mu, r = c * inv;
            float v = (float)r;
            if (p.mask_relu && !(a[i] > 0.f)) v = 0.f;
            g[i] = p.accumulate ? g[i] + v : v;
        }
    }
    return 0;
}

static float tap_root(float x) { return x > 0.f ? sqrtf(x) : (x < 0.f ? -sqrtf(-x) : 0.f); }
int k_ilaf_reduce(const I2VIlafParams& p, i2v_stream_t) {
    std::vector<double> partial((size_t)p.N * p.nblk * 2);
    for (int n = 0; n < p.N; ++n) for (int blk = 0; blk < p.nblk; ++blk) {
        const int64_t chunk = (p.D + p.nblk - 1) / p.nblk, lo = blk * chunk, hi = (lo + chunk < p.D) ? lo + chunk : p.D;
        const float* a = p.a + (size_t)n * p.a_nstride; const float* o = p.ori + (size_t)n * p.D; const float* a0 = p.adv0 + (size_t)n * p.D;
        std::vector<double> t0(256), t1(256);
        for (int t = 0; t < 256; ++t) {
            volatile double dd = 0, dq = 0;
            for (int64_t i = lo + t; i < hi; i += 256) {
                volatile float df = p.mode == 1 ? tap_root(a[i]) - tap_root(o[i]) : a[i] - o[i], d0f = p.mode == 1 ? 0.f : a0[i] - o[i];
                const double d = df, d0 = d0f;
                volatile double m1 = d * d, m2 = d * d0;
                dd = dd + m1; dq = dq + m2;
            }
            t0[t] = dd; t1[t] = dq;
        }
        block_sums2(t0, t1, &partial[((size_t)n * p.nblk + blk) * 2], &partial[((size_t)n * p.nblk + blk) * 2 + 1]);
    }
    // one finishing block per segment (I2VIlafParams::fps), over that segment's partials only
    const int fps = p.fps > 0 ? p.fps : p.N, nseg = p.N / fps;
    for (int seg = 0; seg < nseg; ++seg) {
        std::vector<double> part(partial.begin() + (size_t)seg * fps * p.nblk * 2, partial.begin() + (size_t)(seg + 1) * fps * p.nblk * 2);
        finish_sums2(part, fps * p.nblk, p.sums + 2 * seg);
    }
    return 0;
}

int k_ilaf_grad(const I2VIlafParams& p, i2v_stream_t) {
    const int fps = p.fps > 0 ? p.fps : p.N, nseg = p.N / fps;
    for (int seg = 0; seg < nseg; ++seg) {
    if (p.mode == 1) {                        // TAP feature distance (I2VIlafParams::mode)
        const double dist = sqrt(p.sums[2 * seg]);
        p.loss_out[seg] = (float)dist;
        volatile double c = dist > 0.0 ? p.coef / dist : 0.0;
        for (int n = seg * fps; n < (seg + 1) * fps; ++n) {
            const float* a = p.a + (size_t)n * p.a_nstride; const float* o = p.ori + (size_t)n * p.D;
            float* g = p.grad + (size_t)n * p.grad_nstride;
            for (int64_t i = 0; i < p.D; ++i) {
                float v = 0.f;
                if (a[i] != 0.f && !(p.mask_relu && !(a[i] > 0.f))) {
                    volatile float df = tap_root(a[i]) - tap_root(o[i]);
                    volatile double t1 = c * (double)df, t2 = t1 * 0.5, t3 = t2 / (double)sqrtf(fabsf(a[i]));
                    v = (float)t3;
                }
                g[i] = p.accumulate ? g[i] + v : v;
            }
        }
        continue;
    }
    const double s = sqrt(p.sums[2 * seg]), q = p.sums[2 * seg + 1], n0 = p.init_sq ? sqrt(p.init_sq[seg]) : p.init_norm;
    {
        volatile double t1 = 0.5 * s, t2 = t1 / n0, t3 = n0 * s, t4 = q / t3, t5 = t2 + t4;
        p.loss_out[seg] = (float)(-t5);
    }
    volatile double h = 0.5 / s, ss = s * s, sss = ss * s, qs = q / sss, hd = h - qs, nhd = -hd;
    volatile double cd = nhd / n0;
    volatile double sn = s * n0;
    volatile double c0 = -1.0 / sn;
    for (int n = seg * fps; n < (seg + 1) * fps; ++n) {
        const float* a = p.a + (size_t)n * p.a_nstride; const float* o = p.ori + (size_t)n * p.D; const float* a0 = p.adv0 + (size_t)n * p.D;
        float* g = p.grad + (size_t)n * p.grad_nstride;
        for (int64_t i = 0; i < p.D; ++i) {
            volatile float df = a[i] - o[i], d0f = a0[i] - o[i];
            volatile double t1 = cd * (double)df, t2 = c0 * (double)d0f, r = t1 + t2;
            float v = (float)r;
            if (p.mask_relu && !(a[i] > 0.f)) v = 0.f;
            g[i] = p.accumulate ? g[i] + v : v;
        }
    }
    }
    return 0;
}

int k_head_ce(const I2VHeadParams& p, i2v_stream_t) {
    for (int clip = 0; clip < p.clips; ++clip) {
        if (p.phase & 1)
            for (int c = 0; c < p.C; ++c) {
                double s = 0;
                for (int t = 0; t < p.T; ++t) for (int px = 0; px < p.HW; ++px)
                    s += (double)p.a[((size_t)clip * p.T + t) * p.a_nstride + (size_t)c * p.HW + px];
                p.pooled[(size_t)clip * p.Ctot + p.c_off + c] = (float)(s / ((double)p.T * p.HW));
            }
        if (p.phase & 2) {
            float* lg = p.logits + (size_t)clip * p.K;
            double mx = -1e300;
            for (int k = 0; k < p.K; ++k) {
                double acc = p.bias ? (double)p.bias[k] : 0.0;
                for (int c = 0; c < p.Ctot; ++c) acc += (double)p.W[(size_t)k * p.Ctot + c] * (double)p.pooled[(size_t)clip * p.Ctot + c];
                lg[k] = (float)acc; mx = std::max(mx, (double)lg[k]);
            }
            double se = 0; for (int k = 0; k < p.K; ++k) se += exp((double)lg[k] - mx);
            const int lab = p.labels[clip];
            p.loss_each[clip] = (float)(-((double)lg[lab] - mx - log(se)));
            const double f = (double)p.scale / (double)p.clips;
            for (int c = 0; c < p.Ctot; ++c) {
                double acc = 0;
                for (int k = 0; k < p.K; ++k) acc += (double)p.W[(size_t)k * p.Ctot + c] * (exp((double)lg[k] - mx) / se - (k == lab ? 1.0 : 0.0));
                p.dpooled[(size_t)clip * p.Ctot + c] = (float)(f * acc);
            }
        }
        if (p.phase & 4)
            for (int t = 0; t < p.T; ++t) {
                const size_t n = (size_t)clip * p.T + t;
                const float cnt = (float)(p.T * p.HW);
                for (size_t i = 0; i < (size_t)p.C * p.HW; ++i) {
                    volatile float q = p.dpooled[(size_t)clip * p.Ctot + p.c_off + i / p.HW] / cnt;
                    float v = q;
                    if (p.mask_relu && !(p.a[n * p.a_nstride + i] > 0.f)) v = 0.f;
                    float* g = p.grad + n * p.grad_nstride + i;
                    *g = p.accumulate ? *g + v : v;
                }
            }
    }
    return 0;
}

int k_clip_resample_crop(const uint8_t* frames, float* video, const int32_t* xb, const int32_t* xk, int kx, const int32_t* yb, const int32_t* yk,
                         int ky, int b, int t, int H, int W, int cy, int cx, int oh, int ow, i2v_stream_t) {
    auto clip8 = [](int v) { return std::min(std::max(v >> 22, 0), 255); };
    for (int bi = 0; bi < b; ++bi) for (int ti = 0; ti < t; ++ti) for (int y = 0; y < oh; ++y) for (int x = 0; x < ow; ++x) {
        const int x0 = xb[2 * (x + cx)], nx = xb[2 * (x + cx) + 1], y0 = yb[2 * (y + cy)], ny = yb[2 * (y + cy) + 1];
        const int32_t* kxr = xk + (size_t)(x + cx) * kx; const int32_t* kyr = yk + (size_t)(y + cy) * ky;
        const uint8_t* f = frames + ((size_t)bi * t + ti) * H * W * 3;
        for (int c = 0; c < 3; ++c) {
            int v = 1 << 21;
            for (int j = 0; j < ny; ++j) {
                int h = 1 << 21;
                for (int i = 0; i < nx; ++i) h += f[((size_t)(y0 + j) * W + x0 + i) * 3 + c] * kxr[i];
                v += clip8(h) * kyr[j];
            }
            volatile float q = (float)clip8(v) / 255.f;
            volatile float u = q - MEAN[c];
            video[((((size_t)bi * 3 + c) * t + ti) * oh + y) * ow + x] = u / STD[c];
        }
    }
    return 0;
}

int k_clip_resize_crop(const uint8_t* frames, float* video, const int32_t* xtab, const int32_t* ytab, int b, int t, int H, int W,
                       int cy, int cx, int oh, int ow, i2v_stream_t) {
    for (int bi = 0; bi < b; ++bi) for (int ti = 0; ti < t; ++ti) for (int y = 0; y < oh; ++y) for (int x = 0; x < ow; ++x) {
        const int32_t* xe = xtab + 3 * (x + cx); const int32_t* ye = ytab + 3 * (y + cy);
        const int sx0 = xe[0], sx1 = std::min(sx0 + 1, W - 1), sy0 = ye[0], sy1 = std::min(sy0 + 1, H - 1);
        const uint8_t* f = frames + ((size_t)bi * t + ti) * H * W * 3;
        for (int c = 0; c < 3; ++c) {
            const int S0 = f[((size_t)sy0 * W + sx0) * 3 + c] * xe[1] + f[((size_t)sy0 * W + sx1) * 3 + c] * xe[2];
            const int S1 = f[((size_t)sy1 * W + sx0) * 3 + c] * xe[1] + f[((size_t)sy1 * W + sx1) * 3 + c] * xe[2];
            const int d = (((ye[1] * (S0 >> 4)) >> 16) + ((ye[2] * (S1 >> 4)) >> 16) + 2) >> 2;
            volatile float v = (float)d / 255.f;
            volatile float u = v - MEAN[c];
            video[((((size_t)bi * 3 + c) * t + ti) * oh + y) * ow + x] = u / STD[c];
        }
    }
    return 0;
}

int k_clip_from_u8(const uint8_t* frames, float* video, int b, int t, int h, int w, i2v_stream_t) {
    size_t hw = (size_t)h * w;
    for (int bi = 0; bi < b; ++bi) for (int c = 0; c < 3; ++c) for (int ti = 0; ti < t; ++ti) for (size_t i = 0; i < hw; ++i) {
        volatile float v = (float)frames[(((size_t)bi * t + ti) * hw + i) * 3 + c] / 255.f;
        volatile float d = v - MEAN[c];
        video[(((size_t)bi * 3 + c) * t + ti) * hw + i] = d / STD[c];
    }
    return 0;
}

int k_frames_from_video(const float* video, float* x, float* u, int b, int f, int h, int w, i2v_stream_t) {
    size_t hw = (size_t)h * w;
    for (int bi = 0; bi < b; ++bi) for (int c = 0; c < 3; ++c) for (int fi = 0; fi < f; ++fi)
        for (size_t i = 0; i < hw; ++i) {
            float v = video[(((size_t)bi * 3 + c) * f + fi) * hw + i];
            size_t o = (((size_t)bi * f + fi) * 3 + c) * hw + i;
            x[o] = v;
            volatile float t = v * STD[c];          // mul_ then add_, two roundings
            u[o] = t + MEAN[c];
        }
    return 0;
}

int k_compose(const float* u, const float* d, float* x, int b, int f, int h, int w, float eps, int video_layout, i2v_stream_t) {
    size_t hw = (size_t)h * w;
    for (int bi = 0; bi < b; ++bi) for (int fi = 0; fi < f; ++fi) for (int c = 0; c < 3; ++c)
        for (size_t i = 0; i < hw; ++i) {
            size_t o = (((size_t)bi * f + fi) * 3 + c) * hw + i;
            float dc = std::min(std::max(d[o], -eps), eps);
            float s = u[o] + dc;
            float xi = std::min(std::max(s, 0.f), 1.f);
            float v = (xi - MEAN[c]) / STD[c];
            size_t oo = video_layout ? (((size_t)bi * 3 + c) * f + fi) * hw + i : o;
            x[oo] = v;
        }
    return 0;
}

int k_adam(float* delta, float* m, float* v, const float* gx, const float* u, int64_t n, int hw, float eps,
           float step_size, float bc2_sqrt, float w1, float beta2, float w2, float adam_eps, i2v_stream_t) {
    for (int64_t i = 0; i < n; ++i) {
        int c = (int)((i / hw) % 3);
        float d = delta[i];
        float dc = std::min(std::max(d, -eps), eps);
        float s = u[i] + dc;
        bool pass = d >= -eps && d <= eps && s >= 0.f && s <= 1.f;
        float g = pass ? gx[i] / STD[c] : 0.f;
        float mm = fmaf(w1, g - m[i], m[i]);
        volatile float v1 = v[i] * beta2;
        volatile float t1 = w2 * g;
        volatile float t2 = t1 * g;
        float vv = v1 + t2;
        volatile float den0 = sqrtf(vv) / bc2_sqrt;
        float den = den0 + adam_eps;
        volatile float q = mm / den;
        volatile float upd = -step_size * q;
        delta[i] = d + upd;
        m[i] = mm; v[i] = vv;
    }
    return 0;
}

int k_sign_bim(float* adv, const float* u, const float* grad, int64_t n, int64_t cs, float step, float eps, i2v_stream_t) {
    for (int64_t i = 0; i < n; ++i) {
        int c = (int)((i / cs) % 3);
        volatile float t = adv[i] * STD[c];
        float a = t + MEAN[c];
        float g = grad[i];
        float sg = g > 0.f ? 1.f : (g < 0.f ? -1.f : 0.f);
        volatile float st = step * sg;
        a = a + st;
        float d = std::min(std::max(a - u[i], -eps), eps);
        float r = std::min(std::max(u[i] + d, 0.f), 1.f);
        adv[i] = (r - MEAN[c]) / STD[c];
    }
    return 0;
}

int k_sign_delta(float* delta, const float* grad, int64_t n, float step, i2v_stream_t) {
    for (int64_t i = 0; i < n; ++i) {
        float g = grad[i];
        delta[i] -= step * (g > 0.f ? 1.f : (g < 0.f ? -1.f : 0.f));
    }
    return 0;
}

int k_sign_delta_gx(float* delta, const float* gx, const float* u, int64_t n, float eps, float step, i2v_stream_t) {
    for (int64_t i = 0; i < n; ++i) {
        float d = delta[i];
        float s = u[i] + std::min(std::max(d, -eps), eps);
        bool pass = d >= -eps && d <= eps && s >= 0.f && s <= 1.f;
        float g = pass ? gx[i] : 0.f;
        delta[i] = d - step * (g > 0.f ? 1.f : (g < 0.f ? -1.f : 0.f));
    }
    return 0;
}

int k_tt_grad_mix(const float* grads, float* out, const float* kern, const int* moves, int D, int64_t NC, int T, int HW, float w1, float w,
                  i2v_stream_t) {
    const int64_t per = (int64_t)T * HW, M = NC * per;
    for (int64_t i = 0; i < M; ++i) {
        const int64_t nc = i / per; const int r = (int)(i - nc * per); const int t = r / HW, x = r - t * HW;
        float s = 0.f, d = 0.f;
        for (int k = 0; k < D; ++k) {
            const float* gk = grads + (int64_t)k * M + nc * per;
            int ts = (t + moves[k]) % T; if (ts < 0) ts += T;
            s = fmaf(kern[k], gk[r], s);
            d = fmaf(kern[k], gk[(int64_t)ts * HW + x], d);
        }
        volatile float a = w1 * s; volatile float b = w * d;
        out[i] = a + b;
    }
    return 0;
}

static inline const float* act_addr(const I2VActMat& a, int clip, int c, int pos) {
    const int t = pos / a.HW, r = pos - t * a.HW;
    return a.p + ((int64_t)clip * a.T + t) * a.nstride + (int64_t)c * a.HW + r;
}

// the three product forms of the non-local block: one fmaf chain per output element, in k order (what an MFMA chain computes)
int k_attn_gemm(const I2VAttnGemm& p, i2v_stream_t) {
    for (int b = 0; b < p.clips; ++b) {
        const float* Dn = p.Din ? p.Din + (int64_t)b * p.M * p.N : nullptr;
        if (p.form == 1) {
            for (int i = 0; i < p.M; ++i) for (int j = 0; j < p.N; ++j) {
                float acc = 0.f;
                for (int c = 0; c < p.Cc; ++c) acc = fmaf(*act_addr(p.A, b, c, i), *act_addr(p.B, b, c, j), acc);
                volatile float v = p.scale == 1.f ? acc : p.scale * acc;
                p.D[((int64_t)b * p.M + i) * p.N + j] = v;
            }
        } else {
            const int cols = p.form == 2 ? p.M : p.N, K = p.form == 2 ? p.N : p.M;
            const int split = p.ksplit > 1 ? p.ksplit : 1, kseg = attn_kseg(K, split);
            for (int c = 0; c < p.Cc; ++c) for (int x = 0; x < cols; ++x) {
                float acc = 0.f;
                for (int z = 0; z < split; ++z) {                // K-split launches: one chain per segment, segments added in order
                    float seg = 0.f;
                    for (int k = std::min(z * kseg, K); k < std::min((z + 1) * kseg, K); ++k)
                        seg = p.form == 2 ? fmaf(*act_addr(p.A, b, c, k), Dn[(int64_t)x * p.N + k], seg)      // C[c][i] = sum_j A[c][j] D[i][j]
                                          : fmaf(*act_addr(p.A, b, c, k), Dn[(int64_t)k * p.N + x], seg);      // C[c][j] = sum_i A[c][i] D[i][j]
                    volatile float v2 = z == 0 ? seg : acc + seg;
                    acc = v2;
                }
                const int tt = x / p.C_HW, rr = x - tt * p.C_HW;
                float* o = p.Cact + ((int64_t)b * p.C_T + tt) * p.C_nstride + (int64_t)c * p.C_HW + rr;
                volatile float v = p.accumulate ? *o + acc : acc;
                *o = v;
            }
        }
    }
    return 0;
}

// row softmax / its backward with the device's summation order: thread t owns columns t, t + 256, ...; a wave's 64 partial sums
// are folded by shuffles (offsets 32, 16, ... 1), then the four wave values are added pairwise
static float block_sum256(const std::vector<float>& part) {
    float w[4];
    for (int wv = 0; wv < 4; ++wv) {
        float v[64];
        for (int l = 0; l < 64; ++l) v[l] = part[wv * 64 + l];
        for (int o = 32; o > 0; o >>= 1) for (int l = 0; l < 64; ++l) { volatile float t = v[l] + (l + o < 64 ? v[l + o] : v[l]); v[l] = t; }
        w[wv] = v[0];
    }
    volatile float a = w[0] + w[1], b = w[2] + w[3], r = a + b;
    return r;
}

int k_softmax_rows(const I2VSoftmaxRows& p, i2v_stream_t) {
    for (int64_t r = 0; r < p.rows; ++r) {
        float* x = p.X + r * p.N;
        std::vector<float> part(256, 0.f);
        if (p.mode == 0) {
            float m = -INFINITY;
            for (int j = 0; j < p.N; ++j) m = std::max(m, x[j]);
            for (int t = 0; t < 256; ++t) {
                volatile float s = 0.f;
                for (int j = t; j < p.N; j += 256) { volatile float d = x[j] - m; const float e = expf(d); x[j] = e; s = s + e; }
                part[t] = s;
            }
            const float tot = block_sum256(part);
            for (int j = 0; j < p.N; ++j) { volatile float q = x[j] / tot; x[j] = q; }
        } else {
            const float* P = p.P + r * p.N;
            for (int t = 0; t < 256; ++t) {
                volatile float s = 0.f;
                for (int j = t; j < p.N; j += 256) { volatile float q = x[j] * P[j]; s = s + q; }
                part[t] = s;
            }
            const float dot = block_sum256(part);
            for (int j = 0; j < p.N; ++j) { volatile float d = x[j] - dot; volatile float q = P[j] * d; x[j] = q; }
        }
    }
    return 0;
}

int k_resample_nearest(const float* src, float* dst, int64_t planes, int Hs, int Ws, int Hd, int Wd, const int32_t* my, const int32_t* mx, i2v_stream_t) {
    for (int64_t pl = 0; pl < planes; ++pl)
        for (int y = 0; y < Hd; ++y)
            for (int x = 0; x < Wd; ++x)
                dst[(pl * Hd + y) * Wd + x] = (my[y] >= 0 && mx[x] >= 0) ? src[(pl * Hs + my[y]) * Ws + mx[x]] : 0.f;
    return 0;
}

int k_resample_nearest_bwd(const float* g, float* gs, int64_t planes, int Hd, int Wd, int Hs, int Ws, const int32_t* ylo, const int32_t* yhi,
                           const int32_t* xlo, const int32_t* xhi, i2v_stream_t) {
    for (int64_t pl = 0; pl < planes; ++pl)
        for (int sy = 0; sy < Hs; ++sy)
            for (int sx = 0; sx < Ws; ++sx) {
                volatile float acc = 0.f;
                for (int y = ylo[sy]; y < yhi[sy]; ++y)
                    for (int x = xlo[sx]; x < xhi[sx]; ++x) acc = acc + g[(pl * Hd + y) * Wd + x];
                gs[(pl * Hs + sy) * Ws + sx] = acc;
            }
    return 0;
}

int k_dwconv1d(const float* src, float* dst, int64_t outer, int len, int64_t inner, const float* taps, int k, i2v_stream_t) {
    const int half = k / 2;
    for (int64_t o = 0; o < outer; ++o)
        for (int pos = 0; pos < len; ++pos)
            for (int64_t j = 0; j < inner; ++j) {
                volatile float acc = 0.f;
                for (int t = 0; t < k; ++t) {
                    const int pp = pos + t - half;
                    if (pp >= 0 && pp < len) { volatile float m = taps[t] * src[(o * len + pp) * inner + j]; acc = acc + m; }
                }
                dst[(o * len + pos) * inner + j] = acc;
            }
    return 0;
}

// i2v_grad_post_f32 on the host: the same group enumeration, double sums, fp32 quotients
int k_grad_post_groups(int b, int c, int f, int h, int w, int mode, int64_t* ge) {
    const int64_t HW = (int64_t)h * w;
    switch (mode) {
        case 1: *ge = c * HW; return b * f;
        case 2: *ge = (int64_t)c * f * HW; return b;
        case 3: *ge = (int64_t)c * f * h; return b * w;
        case 4: *ge = (int64_t)b * c * f * HW; return 1;
        default: *ge = 0; return 0;
    }
}
int k_grad_post_splits(int64_t) { return 1; }
int k_grad_post(const float* g, float* momentum, float* out, int B, int C, int F, int H, int W, int fm, int mode, float decay, double*, i2v_stream_t) {
    const int64_t HW = (int64_t)H * W, CFHW = (int64_t)C * F * HW, total = (int64_t)B * CFHW;
    auto src = [&](int64_t o) -> int64_t {
        if (!fm) return o;
        const int64_t i = o % HW; int64_t r = o / HW; const int64_t f = r % F; r /= F; const int64_t c = r % C, b = r / C;
        return ((b * F + f) * C + c) * HW + i;
    };
    auto group = [&](int64_t o) -> int64_t {
        const int64_t b = o / CFHW;
        return mode == 1 ? b * F + (o / HW) % F : mode == 2 ? b : mode == 3 ? b * W + o % W : 0;
    };
    int64_t ge = 0; const int G = k_grad_post_groups(B, C, F, H, W, mode, &ge);
    std::vector<double> sum(G > 0 ? G : 1, 0.0);
    if (mode) for (int64_t o = 0; o < total; ++o) sum[group(o)] += (double)fabsf(g[src(o)]);
    for (int64_t o = 0; o < total; ++o) {
        volatile float v = g[src(o)];
        if (mode) { const float den = mode == 4 ? (float)sum[group(o)] : (float)sum[group(o)] / (float)ge; v = v / den; }
        if (momentum) { volatile float m = momentum[o] * decay; v = v + m; momentum[o] = v; }
        out[o] = v;
    }
    return 0;
}

static const float kStdH[3] = {0.229f, 0.224f, 0.225f};
int k_tap_perts(const float* adv, const float* videos, float* out, int b, int c, int f, int h, int w, i2v_stream_t) {
    const int64_t fhw = (int64_t)f * h * w, n = (int64_t)b * c * fhw;
    for (int64_t i = 0; i < n; ++i) { volatile float d = adv[i] - videos[i]; out[i] = d / kStdH[(i / fhw) % 3]; }
    return 0;
}
int k_tap_sign_abs(const float* smooth, float* sign_out, float* reg, int64_t n, double*, i2v_stream_t) {
    double s = 0.0;
    for (int64_t i = 0; i < n; ++i) { const float v = smooth[i]; sign_out[i] = v > 0.f ? 1.f : (v < 0.f ? -1.f : (v == 0.f ? 0.f : v)); s += (double)fabsf(v); }
    *reg = (float)s;
    return 0;
}
int k_tap_grad(const float* gx, const float* bs, float* out, int B, int C, int F, int H, int W, float weight, i2v_stream_t) {
    const int64_t HW = (int64_t)H * W, n = (int64_t)B * C * F * HW;
    for (int64_t o = 0; o < n; ++o) {
        const int64_t i = o % HW; int64_t r = o / HW; const int64_t f = r % F; r /= F; const int64_t c = r % C, b = r / C;
        volatile float t = weight * bs[o]; volatile float q = t / kStdH[c];
        out[o] = gx[((b * F + f) * C + c) * HW + i] + q;
    }
    return 0;
}

int k_aens_coeffs(const float* prev, float* coeffs, float momentum, int L, i2v_stream_t) {
    std::vector<float> a(L), b(L);
    float mx = -INFINITY, sum = 0.f;
    for (int i = 0; i < L; ++i) mx = std::max(mx, prev[i]);
    for (int i = 0; i < L; ++i) { a[i] = expf(prev[i] - mx); sum += a[i]; }
    for (int i = 0; i < L; ++i) b[i] = a[i] / sum + momentum * coeffs[i];
    mx = -INFINITY; sum = 0.f;
    for (int i = 0; i < L; ++i) mx = std::max(mx, b[i]);
    for (int i = 0; i < L; ++i) { a[i] = expf(b[i] - mx); sum += a[i]; }
    for (int i = 0; i < L; ++i) coeffs[i] = a[i] / sum;
    return 0;
}

int k_aens_reduce(const float* cos, const float* coeffs, int L, int frames, float* feat_sum, float* weighted, i2v_stream_t) {
    for (int l = 0; l < L; ++l) {
        double s = 0; for (int n = 0; n < frames; ++n) s += cos[(size_t)l * frames + n];
        feat_sum[l] = (float)s; weighted[l] = coeffs[l] * (float)s;
    }
    return 0;
}
