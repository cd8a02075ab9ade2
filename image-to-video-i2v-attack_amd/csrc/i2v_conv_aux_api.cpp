// The grouped, depthwise and squeeze-and-excitation launches on their own (include/i2v_conv_aux_launch.h): thin C entries that pack with
// i2v_conv_aux.h -- the planner's own packing -- fill the parameter struct, plan, launch and wait.  Tests and tools; none of them touches
// a net.  The two convolution entries exist where the kernels do (-DI2V_HAVE_GCONV, -DI2V_HAVE_DWCONV: the product build); the pack
// entries and i2v_se_f32 exist on every build, the latter on k_se_* or, without -DI2V_HAVE_SE, on the scalar code of i2v_se_host.h.
#include "i2v_net.h"
#include "i2v_conv_aux.h"
#include "../../include/i2v_conv_aux_launch.h"
#ifndef I2V_HAVE_SE
#include "i2v_se_host.h"
#endif

#include <vector>

using namespace eng;

namespace {

const char* aux_be_text() { return be_error() ? be_error() : "backend error"; }

// a host vector in the library's memory space for the length of one entry call
struct AuxUpload {
    void* p = nullptr;
    ~AuxUpload() { if (p) be_free(p); }
    int put(const std::vector<float>& h) {
        const size_t bytes = h.size() * sizeof(float);
        p = be_malloc(bytes ? bytes : 16);
        return (!p || (bytes && be_h2d(p, h.data(), bytes))) ? 1 : 0;
    }
    const float* f() const { return (const float*)p; }
};

int aux_out_plane(int v, int st) { return (v - 1) / st + 1; }

void aux_classes_out(int st, int H, int W, const int* tapmask, int32_t* classes) {
    if (!classes) return;
    I2VDwConvParams q{};            // (the class geometry is the same code for both kernels)
    q.Ho = H; q.Wo = W;
    conv_aux::conv_classes(q, true, st, 9, tapmask);
    for (int k = 0; k < q.ncls; ++k) {
        int32_t* o = classes + 5 * k;
        o[0] = q.cls[k].Hg; o[1] = q.cls[k].Wg; o[2] = q.cls[k].oh0; o[3] = q.cls[k].ow0; o[4] = q.cls[k].tapmask;
    }
}

}  // namespace

extern "C" int i2v_gconv_pack_f32(const float* filter, int groups, int gw, int stride, int H, int W, float* fwd, float* bwd, int32_t* classes) {
    if (!filter || groups < 1 || gw < 1 || stride < 1 || stride > 2 || H < 1 || W < 1) return fail("i2v_gconv_pack_f32: bad argument");
    if (fwd) conv_aux::gconv_pack_fwd(filter, groups, gw, fwd);
    int tapmask[4] = {0, 0, 0, 0};
    std::vector<float> tmp;
    if (!bwd) { tmp.resize(conv_aux::gconv_bwd_floats(groups, gw, stride)); bwd = tmp.data(); }
    conv_aux::gconv_pack_bwd(filter, groups, gw, stride, bwd, tapmask);
    aux_classes_out(stride, H, W, tapmask, classes);
    return 0;
}

extern "C" int i2v_dwconv_pack_f32(const float* filter, int C, int k, int stride, int H, int W, float* bwd, int32_t* classes) {
    if (!filter || C < 1 || (k != 3 && k != 5) || stride < 1 || stride > 2 || H < 1 || W < 1) return fail("i2v_dwconv_pack_f32: bad argument");
    int tapmask[4] = {0, 0, 0, 0};
    std::vector<float> tmp;
    if (!bwd) { tmp.resize(conv_aux::dwconv_bwd_floats(C, k, stride)); bwd = tmp.data(); }
    conv_aux::dwconv_pack_bwd(filter, C, k, stride, bwd, tapmask);
    aux_classes_out(stride, H, W, tapmask, classes);
    return 0;
}

#if defined(I2V_HAVE_GCONV) || defined(I2V_HAVE_DWCONV)
namespace {
// the views and the epilogue, common to I2VGConvParams and I2VDwConvParams
template <class Params>
void aux_fill(Params& q, const i2v_conv_aux_desc& d) {
    const int Ho = aux_out_plane(d.H, d.stride), Wo = aux_out_plane(d.W, d.stride);
    q.src = d.src; q.src_nstride = d.src_nstride; q.Hs = d.backward ? Ho : d.H; q.Ws = d.backward ? Wo : d.W;
    q.dst = d.dst; q.dst_nstride = d.dst_nstride; q.Ho = d.backward ? d.H : Ho; q.Wo = d.backward ? d.W : Wo;
    q.N = d.N;
    q.shift = d.shift; q.relu = d.relu;
    q.gate_out = d.gate_out; q.gate_out_stride = d.gate_out_stride;
    q.gate = d.gate; q.gate_stride = d.gate_stride;
    q.mask = d.mask; q.mask_nstride = d.mask_nstride;
}
}  // namespace
#endif

#ifdef I2V_HAVE_GCONV
extern "C" int i2v_gconv_f32(const i2v_conv_aux_desc* d, i2v_conv_aux_plan* plan, void* stream) {
    if (!d) return fail("i2v_gconv_f32: null descriptor");
    if (!d->src || !d->dst || !d->filter || d->N < 0 || d->C < 1 || d->groups < 1 || d->C % d->groups || d->H < 1 || d->W < 1 || d->stride < 1 || d->stride > 2)
        return fail("i2v_gconv_f32: bad argument (src, dst, filter, N >= 0, C a multiple of groups, a plane, stride 1 or 2)");
    const int G = d->groups, gw = d->C / G, st = d->stride;
    if (gw != 4 && gw != 8 && gw != 16 && gw != 32 && gw != 64) return fail("i2v_gconv_f32: k_gconv_plan: group width %d not in {4, 8, 16, 32, 64}", gw);
    I2VGConvParams q{};
    aux_fill(q, *d);
    q.groups = G; q.gw = gw;
    int tapmask[4] = {0, 0, 0, 0};
    std::vector<float> w;
    if (d->backward) { w.resize(conv_aux::gconv_bwd_floats(G, gw, st)); conv_aux::gconv_pack_bwd(d->filter, G, gw, st, w.data(), tapmask); }
    else { w.resize(conv_aux::gconv_fwd_floats(G, gw)); conv_aux::gconv_pack_fwd(d->filter, G, gw, w.data()); }
    conv_aux::conv_classes(q, d->backward != 0, st, 9, tapmask);
    if (k_gconv_plan(&q)) return fail("i2v_gconv_f32: k_gconv_plan: the shape does not fit the kernel");
    if (plan) { plan->waves = q.waves; plan->rows = q.rows; plan->pitch = q.Ws + 2; plan->lds_bytes = q.lds_bytes; plan->v4 = 0; }
    if (d->N == 0) return 0;
    AuxUpload up;
    if (up.put(w)) return fail("i2v_gconv_f32: cannot upload the packed kernel: %s", aux_be_text());
    q.w = up.f();
    if (k_gconv(q, stream)) return fail("i2v_gconv_f32: %s", aux_be_text());
    if (be_stream_sync(stream)) return fail("i2v_gconv_f32: k_gconv: %s", aux_be_text());      // (the packed kernel is freed on return)
    return 0;
}
#endif

#ifdef I2V_HAVE_DWCONV
extern "C" int i2v_dwconv_f32(const i2v_conv_aux_desc* d, i2v_conv_aux_plan* plan, void* stream) {
    if (!d) return fail("i2v_dwconv_f32: null descriptor");
    if (!d->src || !d->dst || !d->filter || d->N < 0 || d->C < 1 || d->H < 1 || d->W < 1)
        return fail("i2v_dwconv_f32: bad argument (src, dst, filter, N >= 0, C >= 1, a plane)");
    if (d->k != 3 && d->k != 5) return fail("i2v_dwconv_f32: k_dwconv_plan: filter size %d not in {3, 5}", d->k);
    if (d->stride < 1 || d->stride > 2) return fail("i2v_dwconv_f32: k_dwconv_plan: stride %d not in {1, 2}", d->stride);
    const int C = d->C, k = d->k, st = d->stride;
    I2VDwConvParams q{};
    aux_fill(q, *d);
    q.C = C; q.k = k;
    int tapmask[4] = {0, 0, 0, 0};
    std::vector<float> w;
    if (d->backward) { w.resize(conv_aux::dwconv_bwd_floats(C, k, st)); conv_aux::dwconv_pack_bwd(d->filter, C, k, st, w.data(), tapmask); }
    else w.assign(d->filter, d->filter + (size_t)C * k * k);
    conv_aux::conv_classes(q, d->backward != 0, st, k * k, tapmask);
    if (d->plan_src) q.src = d->plan_src;            // planned for one source ...
    if (k_dwconv_plan(&q)) return fail("i2v_dwconv_f32: k_dwconv_plan: the shape does not fit the kernel");
    q.src = d->src;                                  // ... launched on another: k_dwconv refuses where the two differ in alignment
    if (plan) { plan->waves = q.waves; plan->rows = q.rows; plan->pitch = q.pitch; plan->lds_bytes = q.lds_bytes; plan->v4 = q.v4; }
    if (d->N == 0) return 0;
    AuxUpload up;
    if (up.put(w)) return fail("i2v_dwconv_f32: cannot upload the packed filter: %s", aux_be_text());
    q.w = up.f();
    if (k_dwconv(q, stream)) return fail("i2v_dwconv_f32: %s", aux_be_text());
    if (be_stream_sync(stream)) return fail("i2v_dwconv_f32: k_dwconv: %s", aux_be_text());
    return 0;
}
#endif

extern "C" int i2v_se_f32(const i2v_se_desc_f32* d, void* stream) {
    if (!d) return fail("i2v_se_f32: null descriptor");
    if (!d->w1 || !d->b1 || !d->w2 || !d->b2) return fail("i2v_se_f32: bad argument (w1, b1, w2, b2)");
    if (d->C < 1 || d->rd < 1 || d->HW < 1 || d->N < 0) return fail("i2v_se_f32: k_se_plan: C, rd and HW must be positive, N not negative");
    I2VSeParams q{};
    q.x = d->x; q.x_nstride = d->x_nstride; q.g = d->g; q.g_nstride = d->g_nstride; q.r = d->r; q.r_nstride = d->r_nstride;
    q.dst = d->dst; q.dst_nstride = d->dst_nstride;
    q.m = d->m; q.h = d->h; q.s = d->s; q.t = d->t; q.dmh = d->dmh;
    q.N = d->N; q.C = d->C; q.rd = d->rd; q.HW = d->HW; q.relu = d->relu; q.backward = d->backward ? 1 : 0;
    q.gate_out = d->gate_out; q.gate_out_stride = d->gate_out_stride;
    const int which = d->launches ? d->launches : 7;
    const size_t C = (size_t)d->C, rd = (size_t)d->rd;
    AuxUpload w1, b1, w2t, b2;
    if (which & 2) {            // (only the excite launch reads the weights)
        std::vector<float> t(rd * C);
        for (size_t c = 0; c < C; ++c) for (size_t j = 0; j < rd; ++j) t[j * C + c] = d->w2[c * rd + j];
        if (w1.put(std::vector<float>(d->w1, d->w1 + rd * C)) || b1.put(std::vector<float>(d->b1, d->b1 + rd)) || w2t.put(t) ||
            b2.put(std::vector<float>(d->b2, d->b2 + C)))
            return fail("i2v_se_f32: cannot upload the weights: %s", aux_be_text());
        q.w1 = w1.f(); q.b1 = b1.f(); q.w2t = w2t.f(); q.b2 = b2.f();
    }
#ifdef I2V_HAVE_SE
    if (k_se_plan(&q)) return fail("i2v_se_f32: k_se_plan: the shape does not fit the kernels");
    if ((which & 1) && k_se_squeeze(q, stream)) return fail("i2v_se_f32: %s", aux_be_text());
    if ((which & 2) && k_se_excite(q, stream)) return fail("i2v_se_f32: %s", aux_be_text());
    if ((which & 4) && k_se_scale(q, stream)) return fail("i2v_se_f32: %s", aux_be_text());
#else
    if (se_host::plan(&q)) return fail("i2v_se_f32: the shape does not fit");
    if ((which & 1) && se_host::squeeze(q)) return fail("i2v_se_f32: squeeze failed");
    if ((which & 2) && se_host::excite(q)) return fail("i2v_se_f32: excite failed");
    if ((which & 4) && se_host::scale(q)) return fail("i2v_se_f32: scale failed");
#endif
    if (be_stream_sync(stream)) return fail("i2v_se_f32: %s", aux_be_text());                   // (the uploaded weights are freed on return)
    return 0;
}
