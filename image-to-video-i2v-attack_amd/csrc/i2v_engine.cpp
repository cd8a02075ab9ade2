// Graph planner + executor behind the C ABI of include/i2v_hip.h.
//
// The host declares a backbone as buffers, channel-slice tensor views and conv/maxpool nodes.
// `i2v_net_plan` then
//   * packs every convolution twice -- forward [K=(tap,cin)][cout] and input-gradient
//     [K=(tap,cout)][cin] per stride-parity class -- with the eval-mode BatchNorm scale folded in
//     (reference: image_attacks.py:253-256 freezes BN; autograd's BN backward is a per-channel
//     multiply by the same scale),
//   * lays out one arena (activations + gradients + temporaries) for `max_frames` frames,
//   * emits a flat launch list for the forward pass to the deepest hook and one for the
//     input-gradient pass.  Only d(cost)/d(input) is produced: the reference's weight gradients
//     (image_attacks.py:352, wasted -- weights are frozen) are never computed.
//
// Backward fusion rule: every tensor's gradient is finalised by exactly one launch -- the dgrad of
// its FIRST consumer in forward order -- whose epilogue adds the pending contributions of the
// other consumers (residual alias, downsample dgrad, hook gradient) and applies the tensor's own
// ReLU mask.  Non-final contributions are written raw into temporaries.
#include "i2v_net.h"

#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

using namespace eng;

#define I2V_MAX_NETS 4096
thread_local std::string eng::g_err;

int eng::fail(const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return 1;
}

// the error slot of i2v_last_error() for C entry points defined in other translation units (i2v_loader.hip)
int i2v_api_fail(const char* msg) { return fail("%s", msg); }

// ---------------------------------------------------------------------------------------------
// C ABI: lifetime
// ---------------------------------------------------------------------------------------------
extern "C" const char* i2v_last_error(void) { return g_err.c_str(); }
extern "C" int i2v_abi_version(void) { return 1; }
extern "C" const char* i2v_backend(void) { return be_name(); }
extern "C" long long i2v_backend_stat(const char* name) {
    if (name && !strcmp(name, "overlap_launches")) return __atomic_load_n(&g_overlap_launches, __ATOMIC_RELAXED);
    return name ? be_stat(name) : -1;
}

extern "C" int i2v_create(int device, i2v_handle* out) {
    if (!out) return fail("i2v_create: null out");
    if (be_set_device(device)) return fail("i2v_create: cannot select device %d: %s", device,
                                           be_error() ? be_error() : "?");
    *out = new i2v_ctx(); (*out)->device = device;
    (*out)->nets.reserve(I2V_MAX_NETS);     // the table never reallocates: other threads may be executing planned nets while one is added
    return 0;
}

static void free_net(Net* n) {
    if (!n) return;
    for (void* p : n->dev_allocs) be_free(p);
    if (n->arena) be_free(n->arena);
    for (void* e : n->ov_ev) be_event_destroy(e);
    if (n->side) be_stream_destroy(n->side);
    delete n;
}

extern "C" int i2v_destroy(i2v_handle h) {
    if (!h) return 0;
    for (Net* n : h->nets) free_net(n);
    for (auto& t : h->timed) { be_event_destroy(t.start); be_event_destroy(t.stop); }
    delete h;
    return 0;
}

// ---------------------------------------------------------------------------------------------
// C ABI: description
// ---------------------------------------------------------------------------------------------
extern "C" int i2v_net_create(i2v_handle h, int* net) {
    if (!h || !net) return fail("i2v_net_create: null argument");
    std::lock_guard<std::mutex> lock(h->nets_mu);
    for (size_t i = 0; i < h->nets.size(); ++i)       // a long run re-plans whenever its batch grows: reuse the ids it gave back
        if (!h->nets[i]) { h->nets[i] = new Net(); *net = (int)i; return 0; }
    if (h->nets.size() >= I2V_MAX_NETS) return fail("more than %d backbones alive on one handle", I2V_MAX_NETS);
    h->nets.push_back(new Net());
    *net = (int)h->nets.size() - 1;
    return 0;
}

extern "C" int i2v_net_destroy(i2v_handle h, int net) {
    Net* n = get_net(h, net); if (!n) return 1;
    free_net(n);
    std::lock_guard<std::mutex> lock(h->nets_mu);
    h->nets[net] = nullptr;          // the id may be handed out again by i2v_net_create
    return 0;
}

extern "C" int i2v_net_add_buffer3d(i2v_handle h, int net, int C, int T, int H, int W, int* buf) {
    Net* n = get_net(h, net); if (!n) return 1;
    if (n->planned) return fail("net already planned");
    if (C <= 0 || T <= 0 || H <= 0 || W <= 0 || !buf) return fail("bad buffer shape %dx%dx%dx%d", C, T, H, W);
    Buffer b{C, H, W}; b.T = T;
    n->bufs.push_back(b);
    *buf = (int)n->bufs.size() - 1;
    return 0;
}

extern "C" int i2v_net_add_buffer(i2v_handle h, int net, int C, int H, int W, int* buf) {
    return i2v_net_add_buffer3d(h, net, C, 1, H, W, buf);
}

extern "C" int i2v_net_add_tensor(i2v_handle h, int net, int buf, int c_off, int C, int post_relu, int* tensor) {
    Net* n = get_net(h, net); if (!n) return 1;
    if (buf < 0 || buf >= (int)n->bufs.size()) return fail("bad buffer id %d", buf);
    if (c_off < 0 || C <= 0 || c_off + C > n->bufs[buf].C) return fail("tensor view outside buffer");
    n->tens.push_back(Tensor{buf, c_off, C, post_relu != 0});
    *tensor = (int)n->tens.size() - 1;
    return 0;
}

extern "C" int i2v_net_tensor_frames(i2v_handle h, int net, int tensor, int* T) {
    Net* n = get_net(h, net); if (!n) return 1;
    if (tensor < 0 || tensor >= (int)n->tens.size() || !T) return fail("bad tensor id");
    *T = n->bufs[n->tens[tensor].buf].T;
    return 0;
}

extern "C" int i2v_net_set_input(i2v_handle h, int net, int tensor) {
    Net* n = get_net(h, net); if (!n) return 1;
    if (tensor < 0 || tensor >= (int)n->tens.size()) return fail("bad tensor id");
    n->input = tensor;
    n->bufs[n->tens[tensor].buf].is_input = true;
    return 0;
}

extern "C" int i2v_net_set_relu_gain(i2v_handle h, int net, int tensor, float gain) {
    Net* n = get_net(h, net); if (!n) return 1;
    if (n->planned) return fail("net already planned");
    if (tensor < 0 || tensor >= (int)n->tens.size()) return fail("bad tensor id");
    if (!n->tens[tensor].post_relu) return fail("i2v_net_set_relu_gain: tensor %d is not the output of a ReLU", tensor);
    if (!(gain > 0.f) || !isfinite(gain)) return fail("i2v_net_set_relu_gain: the gain must be positive and finite");
    n->tens[tensor].bwd_gain = gain;
    return 0;
}

// what every convolution entry checks of a node: the net open, the tensor ids, the channel counts, the geometry against the buffers
static int check_conv(Net* n, const i2v_conv3d_desc* d) {
    if (n->planned) return fail("net already planned");
    int nt = (int)n->tens.size();
    if (d->src < 0 || d->src >= nt || d->dst < 0 || d->dst >= nt || d->residual >= nt)
        return fail("i2v_net_add_conv: bad tensor id");
    const Tensor& S = n->tens[d->src]; const Tensor& D = n->tens[d->dst];
    const Buffer& sb = n->bufs[S.buf]; const Buffer& db = n->bufs[D.buf];
    if (S.C != d->cin || D.C != d->cout) return fail("conv channel mismatch");
    if (d->stride < 1 || d->kh < 1 || d->kw < 1 || d->pad < 0 || d->kt < 1 || d->stride_t < 1 || d->pad_t < 0 || d->dil_t < 1)
        return fail("bad conv geometry");
    int Ho = (sb.H + 2 * d->pad - d->kh) / d->stride + 1, Wo = (sb.W + 2 * d->pad - d->kw) / d->stride + 1;
    int To = (sb.T + 2 * d->pad_t - d->dil_t * (d->kt - 1) - 1) / d->stride_t + 1;
    if (Ho != db.H || Wo != db.W) return fail("conv output %dx%d does not match buffer %dx%d", Ho, Wo, db.H, db.W);
    if (To != db.T) return fail("conv output has %d frames per clip, buffer has %d", To, db.T);
    if (d->residual >= 0) {
        const Tensor& R = n->tens[d->residual]; const Buffer& rb = n->bufs[R.buf];
        if (R.C != d->cout || rb.H != db.H || rb.W != db.W || rb.T != db.T) return fail("residual shape mismatch");
    }
    return 0;
}

extern "C" int i2v_net_add_conv3d(i2v_handle h, int net, const i2v_conv3d_desc* d, const float* weight,
                                  const float* scale, const float* shift) {
    Net* n = get_net(h, net); if (!n) return 1;
    if (!d || !weight || !scale || !shift) return fail("i2v_net_add_conv: null argument");
    if (check_conv(n, d)) return 1;
    Node nd; nd.type = 0; nd.cd = *d; memset(&nd.pd, 0, sizeof nd.pd);
    size_t per = (size_t)d->cin * d->kt * d->kh * d->kw;
    nd.w.resize((size_t)d->cout * per);
    for (int co = 0; co < d->cout; ++co)
        for (size_t i = 0; i < per; ++i) nd.w[co * per + i] = weight[co * per + i] * scale[co];
    nd.shift.assign(shift, shift + d->cout);
    n->nodes.push_back(std::move(nd));
    return 0;
}

extern "C" int i2v_net_add_conv(i2v_handle h, int net, const i2v_conv_desc* d, const float* weight,
                                const float* scale, const float* shift) {
    if (!d) return fail("i2v_net_add_conv: null argument");
    i2v_conv3d_desc q{d->src, d->dst, d->cin, d->cout, 1, d->kh, d->kw, 1, d->stride, 0, d->pad, 1, d->relu, d->residual};
    return i2v_net_add_conv3d(h, net, &q, weight, scale, shift);
}

// A grouped 3x3 convolution.  The node is stored with its block-diagonal dense weight -- the dense route (I2V_GCONV=0, and the host
// simulation) packs and runs it as any other convolution -- and with the compact kernel k_gconv reads.
extern "C" int i2v_net_add_conv_grouped(i2v_handle h, int net, const i2v_conv_desc* d, int groups, const float* weight,
                                        const float* scale, const float* shift) {
    if (!d || !weight || !scale || !shift) return fail("i2v_net_add_conv_grouped: null argument");
    if (groups == 1) return i2v_net_add_conv(h, net, d, weight, scale, shift);
    if (groups < 1 || d->cin % groups || d->cout % groups)
        return fail("i2v_net_add_conv_grouped: %d input and %d output channels are not divisible by %d groups", d->cin, d->cout, groups);
    if (d->kh != 3 || d->kw != 3 || d->pad != 1 || (d->stride != 1 && d->stride != 2))
        return fail("i2v_net_add_conv_grouped: only 3x3 / pad 1 / stride 1 or 2 is supported (got %dx%d, pad %d, stride %d)", d->kh, d->kw, d->pad, d->stride);
    const int gi = d->cin / groups, go = d->cout / groups;
    if (gi != go || (gi != 4 && gi != 8 && gi != 16 && gi != 32 && gi != 64))
        return fail("i2v_net_add_conv_grouped: group width %d -> %d is not one of 4, 8, 16, 32, 64 in and out (depthwise is not supported)", gi, go);
    if (d->residual >= 0) return fail("i2v_net_add_conv_grouped: a residual addend on a grouped convolution is not supported");
    std::vector<float> dense((size_t)d->cout * d->cin * 9, 0.f);
    for (int co = 0; co < d->cout; ++co)
        for (int ci = 0; ci < gi; ++ci)
            for (int t = 0; t < 9; ++t)
                dense[((size_t)co * d->cin + (co / go) * gi + ci) * 9 + t] = weight[((size_t)co * gi + ci) * 9 + t];
    if (i2v_net_add_conv(h, net, d, dense.data(), scale, shift)) return 1;
    Node& nd = get_net(h, net)->nodes.back();
    nd.groups = groups;
    nd.wg.resize((size_t)d->cout * gi * 9);
    for (int co = 0; co < d->cout; ++co)
        for (int i = 0; i < gi * 9; ++i) nd.wg[(size_t)co * gi * 9 + i] = weight[(size_t)co * gi * 9 + i] * scale[co];
    std::vector<float>().swap(nd.w);         // the dense expansion (groups times the floats) is rebuilt from `wg` only by a plan on the dense route
    return 0;
}

// the block-diagonal dense weight of a grouped (or depthwise: group width 1) node, for the dense route's packings
static void expand_grouped(Node& nd) {
    const i2v_conv3d_desc& c = nd.cd;
    const int gi = c.cin / nd.groups, go = c.cout / nd.groups, nt = c.kh * c.kw;
    nd.w.assign((size_t)c.cout * c.cin * nt, 0.f);
    for (int co = 0; co < c.cout; ++co)
        for (int ci = 0; ci < gi; ++ci)
            for (int t = 0; t < nt; ++t) nd.w[((size_t)co * c.cin + (co / go) * gi + ci) * nt + t] = nd.wg[((size_t)co * gi + ci) * nt + t];
}

// A depthwise k x k convolution (k = 3 or 5).  Only the compact [C][k k] filter is kept: k_dwconv reads it as it is, and the dense
// route (I2V_DWCONV=0, and the host simulation) expands it block-diagonally -- C times the floats -- only while a plan packs the node.
extern "C" int i2v_net_add_conv_depthwise(i2v_handle h, int net, const i2v_conv_desc* d, const float* weight,
                                          const float* scale, const float* shift) {
    if (!d || !weight || !scale || !shift) return fail("i2v_net_add_conv_depthwise: null argument");
    if (d->cin != d->cout) return fail("i2v_net_add_conv_depthwise: %d input and %d output channels (a depthwise convolution has as many out as in)", d->cin, d->cout);
    if (d->kh != d->kw || (d->kh != 3 && d->kh != 5))
        return fail("i2v_net_add_conv_depthwise: only square 3x3 and 5x5 filters are supported (got %dx%d)", d->kh, d->kw);
    if (d->pad != d->kh / 2) return fail("i2v_net_add_conv_depthwise: the padding must be k / 2 = %d (got pad %d)", d->kh / 2, d->pad);
    if (d->stride != 1 && d->stride != 2) return fail("i2v_net_add_conv_depthwise: only stride 1 or 2 is supported (got stride %d)", d->stride);
    if (d->residual >= 0) return fail("i2v_net_add_conv_depthwise: a residual addend on a depthwise convolution is not supported");
    Net* n = get_net(h, net); if (!n) return 1;
    const i2v_conv3d_desc q{d->src, d->dst, d->cin, d->cout, 1, d->kh, d->kw, 1, d->stride, 0, d->pad, 1, d->relu, d->residual};
    if (check_conv(n, &q)) return 1;
    const int nt = d->kh * d->kw;
    Node nd; nd.type = 0; nd.cd = q; memset(&nd.pd, 0, sizeof nd.pd);
    nd.shift.assign(shift, shift + d->cout);
    nd.groups = d->cin; nd.dw = d->kh;
    nd.wg.resize((size_t)d->cout * nt);
    for (int c = 0; c < d->cout; ++c)
        for (int t = 0; t < nt; ++t) nd.wg[(size_t)c * nt + t] = weight[(size_t)c * nt + t] * scale[c];
    n->nodes.push_back(std::move(nd));
    return 0;
}

extern "C" int i2v_net_add_conv_preact(i2v_handle h, int net, const i2v_conv_desc* d, const float* weight,
                                       const float* scale, const float* shift, const float* pre_scale,
                                       const float* pre_shift) {
    if (!d || !pre_scale || !pre_shift) return fail("i2v_net_add_conv_preact: null argument");
    if (d->kh != 1 || d->kw != 1 || d->stride != 1 || d->pad != 0 || d->residual >= 0)
        return fail("pre-activation is supported on plain 1x1/stride-1 convolutions only");
    if (i2v_net_add_conv(h, net, d, weight, scale, shift)) return 1;
    Net* n = get_net(h, net);
    if (n->tens[d->src].post_relu) return fail("pre-activation input must not be a ReLU output");
    Node& nd = n->nodes.back();
    nd.pre_scale.assign(pre_scale, pre_scale + d->cin);
    nd.pre_shift.assign(pre_shift, pre_shift + d->cin);
    return 0;
}

extern "C" int i2v_net_add_maxpool3d(i2v_handle h, int net, const i2v_pool3d_desc* d) {
    Net* n = get_net(h, net); if (!n) return 1;
    if (n->planned) return fail("net already planned");
    int nt = (int)n->tens.size();
    if (!d || d->src < 0 || d->src >= nt || d->dst < 0 || d->dst >= nt) return fail("bad pool desc");
    if (n->tens[d->src].C != n->tens[d->dst].C) return fail("pool channel mismatch");
    if (d->kt < 1 || d->k < 1 || d->stride_t < 1 || d->stride < 1 || d->pad_t < 0 || d->pad < 0) return fail("bad pool geometry");
    const Buffer& sb = n->bufs[n->tens[d->src].buf]; const Buffer& db = n->bufs[n->tens[d->dst].buf];
    if ((sb.T + 2 * d->pad_t - d->kt) / d->stride_t + 1 != db.T) return fail("pool output frames per clip do not match the buffer");
    {   // the destination plane must be what this window produces (floor, or ceil_mode's one extra row / column)
        const int ho = (sb.H + 2 * d->pad - d->k) / d->stride + 1, hc = (sb.H + 2 * d->pad - d->k + d->stride - 1) / d->stride + 1;
        const int wo = (sb.W + 2 * d->pad - d->k) / d->stride + 1, wc = (sb.W + 2 * d->pad - d->k + d->stride - 1) / d->stride + 1;
        if (sb.H + 2 * d->pad < d->k || sb.W + 2 * d->pad < d->k || db.H < ho || db.H > hc || db.W < wo || db.W > wc)
            return fail("pool output plane %dx%d does not match %dx%d pooled by k=%d stride=%d pad=%d", db.H, db.W, sb.H, sb.W, d->k, d->stride, d->pad);
    }
    Node nd; nd.type = 1; nd.pd = *d; memset(&nd.cd, 0, sizeof nd.cd);
    n->nodes.push_back(std::move(nd));
    return 0;
}

extern "C" int i2v_net_add_maxpool(i2v_handle h, int net, const i2v_pool_desc* d) {
    if (!d) return fail("bad pool desc");
    i2v_pool3d_desc q{d->src, d->dst, 1, d->k, 1, d->stride, 0, d->pad};
    return i2v_net_add_maxpool3d(h, net, &q);
}

extern "C" int i2v_net_add_avgpool(i2v_handle h, int net, const i2v_pool_desc* d) {
    if (i2v_net_add_maxpool(h, net, d)) return 1;
    Net* n = get_net(h, net);
    if (d->pad != 0) return fail("average pooling with padding is not supported");
    n->nodes.back().type = 2;
    return 0;
}

extern "C" int i2v_net_add_attention(i2v_handle h, int net, const i2v_attn_desc* d) {
    Net* n = get_net(h, net); if (!n) return 1;
    if (n->planned) return fail("net already planned");
    const int nt = (int)n->tens.size();
    if (!d) return fail("bad attention desc");
    for (int t : {d->theta, d->phi, d->g, d->dst}) if (t < 0 || t >= nt) return fail("bad attention tensor");
    const Tensor& th = n->tens[d->theta]; const Tensor& ph = n->tens[d->phi]; const Tensor& gg = n->tens[d->g]; const Tensor& ds = n->tens[d->dst];
    if (th.C != ph.C || th.C != gg.C || th.C != ds.C) return fail("attention: theta / phi / g / dst channel counts differ");
    const Buffer& tb = n->bufs[th.buf]; const Buffer& pb = n->bufs[ph.buf]; const Buffer& gb = n->bufs[gg.buf]; const Buffer& db = n->bufs[ds.buf];
    if (tb.T != db.T || tb.H != db.H || tb.W != db.W) return fail("attention: dst must have theta's positions");
    if (pb.T != gb.T || pb.H != gb.H || pb.W != gb.W) return fail("attention: phi and g must have the same positions");
    if (th.post_relu || ph.post_relu || gg.post_relu) return fail("attention: theta / phi / g are linear embeddings (no ReLU)");
    if (!(d->scale > 0.f)) return fail("attention: scale must be positive");
    Node nd; nd.type = 3; nd.ad = *d; memset(&nd.cd, 0, sizeof nd.cd); memset(&nd.pd, 0, sizeof nd.pd);
    n->nodes.push_back(std::move(nd));
    return 0;
}

// A squeeze-and-excitation node.  fc2's weight is kept transposed, [rd][C]: every sum of the excite kernel then walks coalesced rows.
extern "C" int i2v_net_add_se(i2v_handle h, int net, const i2v_se_desc* d, const float* W1, const float* b1, const float* W2, const float* b2) {
    if (!d || !W1 || !b1 || !W2 || !b2) return fail("i2v_net_add_se: null argument");
    Net* n = get_net(h, net); if (!n) return 1;
    if (n->planned) return fail("net already planned");
    const int nt = (int)n->tens.size();
    if (d->src < 0 || d->src >= nt || d->dst < 0 || d->dst >= nt || d->residual >= nt || d->src == d->dst) return fail("i2v_net_add_se: bad tensor id");
    const Tensor& S = n->tens[d->src]; const Tensor& D = n->tens[d->dst];
    const Buffer& sb = n->bufs[S.buf]; const Buffer& db = n->bufs[D.buf];
    if (S.C != d->C || D.C != d->C) return fail("i2v_net_add_se: C = %d, but src has %d channels and dst %d", d->C, S.C, D.C);
    if (d->rd < 1) return fail("i2v_net_add_se: rd = %d (the squeezed width must be at least 1)", d->rd);
    if (d->rd > 8192) return fail("i2v_net_add_se: rd = %d (at most 8192 squeezed channels are supported)", d->rd);
    if (sb.T != 1 || db.T != 1) return fail("i2v_net_add_se: video tensors (more than one frame per clip) are not supported yet");
    if (sb.H != db.H || sb.W != db.W) return fail("i2v_net_add_se: src plane %dx%d and dst plane %dx%d differ", sb.H, sb.W, db.H, db.W);
    if (S.post_relu) return fail("i2v_net_add_se: src must be the linear output of a convolution, not the output of a ReLU");
    if ((d->relu != 0) != D.post_relu) return fail("i2v_net_add_se: relu = %d, but dst is %sdeclared the output of a ReLU", d->relu, D.post_relu ? "" : "not ");
    if (d->residual >= 0) {
        const Tensor& R = n->tens[d->residual]; const Buffer& rb = n->bufs[R.buf];
        if (R.C != d->C || rb.H != db.H || rb.W != db.W || rb.T != db.T)
            return fail("i2v_net_add_se: residual shape %dx%dx%d does not match dst %dx%dx%d", R.C, rb.H, rb.W, d->C, db.H, db.W);
        if (d->residual == d->src || d->residual == d->dst) return fail("i2v_net_add_se: the residual must be a tensor of its own");
    }
    Node nd; nd.type = 4; nd.sd = *d; memset(&nd.cd, 0, sizeof nd.cd); memset(&nd.pd, 0, sizeof nd.pd);
    nd.cd.residual = -1;
    const size_t C = (size_t)d->C, rd = (size_t)d->rd;
    nd.se_w1.assign(W1, W1 + rd * C); nd.se_b1.assign(b1, b1 + rd); nd.se_b2.assign(b2, b2 + C);
    nd.se_w2t.resize(rd * C);
    for (size_t c = 0; c < C; ++c)
        for (size_t j = 0; j < rd; ++j) nd.se_w2t[j * C + c] = W2[c * rd + j];
    n->nodes.push_back(std::move(nd));
    return 0;
}

// ---------------------------------------------------------------------------------------------
// planning
// ---------------------------------------------------------------------------------------------
extern "C" int i2v_net_plan(i2v_handle h, int net, const int* hook_tensors, int n_hooks, int max_frames) {
    Net* np = get_net(h, net); if (!np) return 1;
    Net& n = *np;
    if (n.planned) return fail("net already planned");
    if (n.input < 0) return fail("input tensor not set");
    if (n_hooks <= 0 || max_frames <= 0) return fail("need >=1 hook and >=1 frame");
    // the split-bf16 loop lives in the EXPERIMENTAL build only (i2v_conv_exp.hip): asking the product library for it is an error, not
    // a silent fp32 run under another name
    if (math_bf16x3() && strncmp(be_name(), "hip", 3) == 0 && be_stat("experimental") != 1)
        return fail("I2V_MATH=bf16x3 needs a library built with -DI2V_EXPERIMENTAL (python __graft_entry__.py --experimental, then I2V_LIB=...)");
    for (int i = 0; i < n_hooks; ++i)
        if (hook_tensors[i] < 0 || hook_tensors[i] >= (int)n.tens.size()) return fail("bad hook tensor");
    n.hooks.assign(hook_tensors, hook_tensors + n_hooks);
    n.maxN = max_frames;
    const size_t N = (size_t)max_frames;
    const int Tin = n.Tin();
    if (max_frames % Tin) return fail("max_frames=%d is not a multiple of the input's %d frames per clip", max_frames, Tin);

    for (Node& nd : n.nodes) {
        if (nd.type == 4 && (upload(n, nd.se_w1, &nd.se_w1_d) || upload(n, nd.se_b1, &nd.se_b1_d) || upload(n, nd.se_w2t, &nd.se_w2t_d) || upload(n, nd.se_b2, &nd.se_b2_d))) return 1;
        if (nd.type != 0) continue;
        if (upload(n, nd.shift, &nd.shift_d)) return 1;
        nd.gconv = nd.groups > 1 && !nd.dw && gconv_enabled();
        nd.dwconv = nd.dw && dwconv_enabled();
        if (nd.dwconv) {            // compact operands only: the dense packing (C times the floats) is never made
            if (nd.cd.src == n.input) return fail("a depthwise convolution directly on the input is not planned");
            if (pack_dwconv(n, nd)) return 1;
            continue;
        }
        if (nd.gconv) {             // compact operands only: the dense packing (groups times the floats) is never made
            if (nd.cd.src == n.input) return fail("a grouped convolution directly on the input is not planned");
            if (pack_gconv(n, nd)) return 1;
            continue;
        }
        if (nd.groups > 1 || nd.dw) expand_grouped(nd);
        if (pack_fwd(n, nd)) return 1;
        if (nd.preact()) {          // operand-side affine, padded to Kpad with zeros (relu(0*x+0) = 0 for the K tail)
            std::vector<float> ps(nd.fwd.Kpad > nd.fwd.Cdpad ? nd.fwd.Kpad : nd.fwd.Cdpad, 0.f), pt(ps.size(), 0.f);
            for (int c = 0; c < nd.cd.cin; ++c) { ps[c] = nd.pre_scale[c]; pt[c] = nd.pre_shift[c]; }
            if (upload(n, ps, &nd.pre_scale_d) || upload(n, pt, &nd.pre_shift_d)) return 1;
        }
        if (nd.cd.src == n.input) { if (pack_img(n, nd)) return 1; }
        else if (pack_bwd(n, nd)) return 1;
        if (nd.groups > 1 || nd.dw) std::vector<float>().swap(nd.w);
    }
    size_t off = 64;            // 256 bytes of slack in front of the first tensor (and behind the last, below): the quad-row
                                // staging of conv_igemm (MODE 4) reads a few pixels past either end of a source view
    for (const Node& nd : n.nodes) if (nd.type == 0 && nd.cd.src == n.input && nd.fwd.quad) n.stage_input = true;
    if (n.stage_input) {        // ... which the caller's frame tensor cannot promise: forward() copies it in here first
        const Buffer& ib = n.bufs[n.tens[n.input].buf];
        n.in_stage_off = off; off = align_up(off + N * ib.C * ib.H * ib.W, 64) + 64;
    }
    for (Buffer& b : n.bufs) {
        if (b.is_input) continue;
        size_t sz = N / Tin * b.T * b.C * b.H * b.W;
        b.act_off = off; off = align_up(off + sz, 64);
        b.grad_off = off; off = align_up(off + sz, 64);
    }
    // 1-bit ReLU gates (I2VConvParams::gate*): every buffer holding the output of a ReLU convolution gets one bit per
    // element, rows per channel; the input-gradient pass gates with these instead of re-reading fp32 activations
    const char* gates_env = getenv("I2V_GATES");           // developer knob: I2V_GATES=0 keeps the fp32-activation gates
    const bool use_gates = !(gates_env && gates_env[0] == '0');
    for (const Node& nd : n.nodes)
        if (use_gates && nd.type == 0 && nd.cd.relu && !nd.fwd.tpair) n.bufs[n.tens[nd.cd.dst].buf].gated = true;   // (the class-packed epilogue writes no gate words)
    for (const Node& nd : n.nodes)
        if (use_gates && nd.type == 4 && nd.sd.relu) n.bufs[n.tens[nd.sd.dst].buf].gated = true;   // (the scale launch writes the rows)
    for (Buffer& b : n.bufs) {
        if (!b.gated) continue;
        const size_t pix = N / Tin * b.T * b.H * b.W;
        if (pix + 64 >= (1ull << 31)) return fail("gate rows of more than 2^31 bits are not supported");
        b.gate_words = (int)((pix + 31) / 32 + 2);
        b.gate_off = off; off = align_up(off + (size_t)b.C * b.gate_words, 64);
    }
    for (Node& nd : n.nodes)
        if (nd.type == 1) {
            const Buffer& db = n.bufs[n.tens[nd.pd.dst].buf];
            nd.idx_off = off; off = align_up(off + (N / Tin * db.T * n.tens[nd.pd.dst].C * db.H * db.W + 3) / 4, 64);
        }
    for (Node& nd : n.nodes)
        if (nd.type == 3) {
            const Buffer& tb = n.bufs[n.tens[nd.ad.theta].buf]; const Buffer& pb = n.bufs[n.tens[nd.ad.phi].buf];
            nd.p_off = off; off = align_up(off + N / Tin * ((size_t)tb.T * tb.H * tb.W) * ((size_t)pb.T * pb.H * pb.W), 64);
        }
    for (Node& nd : n.nodes)
        if (nd.type == 4) {     // m, h, s (forward to backward) and t, dm / HW (backward): (4 C + rd) floats per frame, each vector on a 256-byte boundary
            const size_t C = (size_t)nd.sd.C, rd = (size_t)nd.sd.rd;
            nd.se_off = off; nd.se_floats = 4 * align_up(N * C, 64) + align_up(N * rd, 64);
            off += nd.se_floats;
        }
    std::string err;
    size_t end = 0;
    if (!plan_pass(n, true, off, N, &end, &err)) return fail("plan: %s", err.c_str());
    n.arena_floats = end + 64;
    n.arena = (float*)be_malloc(n.arena_floats * sizeof(float));
    if (!n.arena) return fail("arena allocation of %zu bytes failed", n.arena_floats * sizeof(float));
    CHECK_BE(be_memset0(n.arena, n.arena_floats * sizeof(float), nullptr));
    if (!plan_pass(n, false, off, N, &end, &err)) return fail("plan: %s", err.c_str());
    mark_fusable(n);
    if (autotune(n)) return 1;
    mark_overlap(n);
    record_unstored(n);
    // planning works on the null stream (uploads, arena clears, tuning probes); the caller may execute the net on any
    // stream, including non-blocking ones that do not order against it
    CHECK_BE(be_stream_sync(nullptr));
    n.planned = true;
    return 0;
}

extern "C" int i2v_net_fusion_info(i2v_handle h, int net, int32_t out[4]) {
    Net* n = get_net(h, net); if (!n) return 1;
    if (!n->planned || !out) return fail("i2v_net_fusion_info: net not planned");
    out[0] = out[1] = out[2] = out[3] = 0;
    int k = 0;
    for (const std::vector<Launch>* L : {&n->fwd, &n->bwd}) {
        for (const Launch& l : *L) { out[k] += l.fuse_ok ? 1 : 0; out[2 + k] += (l.fuse_ok && l.fuse_b[0]) ? 1 : 0; }
        ++k;
    }
    return 0;
}

extern "C" int i2v_net_scpair_info(i2v_handle h, int net, int32_t out[4]) {
    Net* n = get_net(h, net); if (!n) return 1;
    if (!n->planned || !out) return fail("i2v_net_scpair_info: net not planned");
    out[0] = out[1] = out[2] = out[3] = 0;
    int k = 0;
    for (const std::vector<Launch>* L : {&n->fwd, &n->bwd}) {
        for (const Launch& l : *L) { out[k] += l.sc_ok ? 1 : 0; out[2 + k] += (l.sc_ok && l.sc_b[0]) ? 1 : 0; }
        ++k;
    }
    return 0;
}

extern "C" size_t i2v_net_workspace_bytes(i2v_handle h, int net) {
    Net* n = get_net(h, net); if (!n) return 0;
    return n->arena_floats * sizeof(float) + n->weight_bytes;
}

// The library build compiles the engine units one by one (-DI2V_SEPARATE_UNITS, __graft_entry__.py).  A plain one-file build of this
// unit -- the host simulation's recipe, `g++ i2v_engine.cpp hostsim_backend.cpp` (tests/hostsim/build.sh) -- takes the others in here.
#ifndef I2V_SEPARATE_UNITS
#include "i2v_pack.cpp"
#include "i2v_plan.cpp"
#include "i2v_tune.cpp"
#include "i2v_run.cpp"
#include "i2v_loop_api.cpp"
#include "i2v_conv_aux_api.cpp" // (the grouped / depthwise packers and the squeeze-and-excitation node on their own, include/i2v_conv_aux_launch.h)
// ... and the ConvNeXt planner on the scalar restatements of the transformer launches it uses (i2v_xf_host.h), so that the planner
// tests can run it without a GPU.  i2v_xf.h's file-local `fail` would be ambiguous with eng::fail under this unit's using-directives.
#define fail xf_fail
#include "i2v_convnext.cpp"
#include "i2v_mixer.cpp"        // (... and the MLP-Mixer / ResMLP planner, on the same restatements and i2v_mixer_host.h)
#include "i2v_cait.cpp"         // (... and the CaiT planner, on the same restatements and i2v_cait_host.h)
#include "i2v_convit.cpp"       // (... and the ConViT planner, on the same restatements and i2v_convit_host.h)
#include "i2v_xcit.cpp"         // (... and the XCiT planner, on the same restatements and i2v_xcit_host.h)
#include "i2v_twins.cpp"        // (... and the Twins planner, on the same restatements, i2v_xcit_host.h and i2v_twins_host.h)
#include "i2v_beit.cpp"         // (... and the BEiT planner, on the same restatements and i2v_beit_host.h)
#include "i2v_pit.cpp"          // (... and the PiT planner, on the same restatements and i2v_pit_host.h)
#include "i2v_coat.cpp"         // (... and the CoaT planner, on the same restatements and i2v_coat_host.h)
#include "i2v_tnt.cpp"          // (... and the TNT planner, on the same restatements, i2v_beit_host.h and i2v_tnt_host.h)
#include "i2v_xf_api.cpp"       // (... and the restatements on their own, include/i2v_xf_launch.h)
#include "i2v_quality.cpp"      // (... and the 8-bit export and the quality launches as scalar code, i2v_quality_host.h)
#undef fail
#endif
