// The planner: a net's nodes as a forward and an input-gradient launch list (see the file header of i2v_engine.cpp).
#include "i2v_net.h"
#include "i2v_conv_aux.h"
#ifndef I2V_HAVE_SE
#include "i2v_se_host.h"
#endif

#include <string.h>

#include <algorithm>

namespace eng {

// ---------------------------------------------------------------------------------------------
// views
// ---------------------------------------------------------------------------------------------
View view_of(Net& n, int t, bool grad) {
    const Tensor& T = n.tens[t];
    const Buffer& B = n.bufs[T.buf];
    size_t off = grad ? B.grad_off : B.act_off;
    View v;
    v.p = n.arena + off + (size_t)T.c_off * B.H * B.W;
    v.nstride = (int64_t)B.C * B.H * B.W;
    v.C = T.C; v.H = B.H; v.W = B.W; v.T = B.T;
    return v;
}

// ---------------------------------------------------------------------------------------------
// planning
// ---------------------------------------------------------------------------------------------
static void conv_common(I2VConvParams& p, const Packed& P) {
    memset(&p, 0, sizeof p);
    p.wp = P.wp; p.wpc = P.wpc; p.ktab = P.ktab; p.K = P.K; p.Kpad = P.Kpad; p.tap_uniform = P.tap_uniform; p.Cd = P.Cd; p.Cdpad = P.Cdpad;
    p.wp3 = P.wp3; p.bf3 = P.wp3 ? 1 : 0;
    p.add0_stride = 1;
    p.blkt = 1; p.Tg = p.Ts = p.To = p.st = p.ost = 1; p.ot0 = 0; p.oct = 1;
    p.temporal = P.has_dt;      // conv_run adds the frame-mapping half of the condition
    p.quad = P.quad; p.quad_kw = P.quad_kw; p.quad_dw0 = P.quad_dw0;
    p.halo = P.halo;
    p.ig_tt = P.ig_tt; p.ig_th = P.ig_th; p.ig_tw = P.ig_tw; p.ig_p77 = P.ig_p77;
}

static bool overlaps(const Tensor& a, const Tensor& b) {
    return a.buf == b.buf && a.c_off < b.c_off + b.C && b.c_off < a.c_off + a.C;
}

namespace {

struct Planner {
    Net& n; bool dry; size_t off; size_t N;
    std::vector<int> left; std::vector<std::vector<Addend>> pending;
    std::vector<float*> hook_tmp;      // per hook: temp gradient buffer or null (direct)
    std::vector<View> galias; std::vector<char> has_alias;   // residual gradient that is just a view
    std::vector<char> accum;                                 // per buffer: gradient accumulates (dense blocks)
    std::string err;

    float* base() const { return dry ? (float*)nullptr : n.arena; }
    size_t nf(int T) const { return N / (size_t)n.Tin() * (size_t)T; }      // frames of a tensor with T frames per clip
    size_t carve(size_t floats) { size_t o = off; off = align_up(off + floats, 64); return o; }
    float* temp(size_t floats) { return base() + carve(floats); }

    View view(int t, bool grad) {
        if (grad && has_alias[t]) return galias[t];
        const Tensor& T = n.tens[t]; const Buffer& B = n.bufs[T.buf];
        View v; v.p = base() + (grad ? B.grad_off : B.act_off) + (size_t)T.c_off * B.H * B.W;
        v.nstride = (int64_t)B.C * B.H * B.W; v.C = T.C; v.H = B.H; v.W = B.W; v.T = B.T;
        return v;
    }
    void emit(std::vector<Launch>& L, const Launch& l) { if (!dry) L.push_back(l); }
    // gate rows of tensor t (null when its buffer keeps no gates)
    uint32_t* gate_rows(int t, int* stride) const {
        const Tensor& T = n.tens[t]; const Buffer& B = n.bufs[T.buf];
        if (!B.gated) return nullptr;
        *stride = B.gate_words;
        return (uint32_t*)(base() + B.gate_off) + (size_t)T.c_off * B.gate_words;
    }
    // the ReLU gate of tensor t for a launch that finalises its gradient: bits when available, else the fp32 activation
    void set_gate(I2VConvParams& p, int t) {
        int st = 0;
        if (uint32_t* g = gate_rows(t, &st)) { p.gate = g; p.gate_stride = st; p.gate_pix0 = 0; }
        else { View a = view(t, false); p.mask = a.p; p.mask_nstride = a.nstride; }
    }

    void emit_addmask(View out, const std::vector<Addend>& adds, int t) {
        Launch l; memset(&l.am, 0, sizeof l.am); l.kind = L_ADDMASK;
        l.am.out = out.p; l.am.out_nstride = out.nstride;
        for (size_t i = 0; i < adds.size() && i < 3; ++i) { l.am.a[i] = adds[i].p; l.am.a_nstride[i] = adds[i].nstride; }
        if (n.tens[t].post_relu) {
            int st = 0;
            if (uint32_t* g = gate_rows(t, &st)) { l.am.gate = g; l.am.gate_stride = st; }
            else { View a = view(t, false); l.am.mask = a.p; l.am.mask_nstride = a.nstride; }
        }
        l.am.N = 0; l.am.C = out.C; l.am.HW = out.H * out.W; l.T = out.T;
        emit(n.bwd, l);
    }

    // reduce pending list of tensor t to at most `keep` plain/compact addends
    bool squeeze_pending(int t, size_t keep) {
        auto& P = pending[t];
        while (P.size() > keep) {
            // fold the last two plain addends into a temp
            size_t a = P.size() - 1, b = P.size() - 2;
            if (P[a].stride != 1 || P[b].stride != 1) { err = "cannot fold compact addends"; return false; }
            View g = view(t, true);
            View tv = g; tv.p = temp(nf(g.T) * g.C * g.H * g.W); tv.nstride = (int64_t)g.C * g.H * g.W;
            Launch l; memset(&l.am, 0, sizeof l.am); l.kind = L_ADDMASK; l.T = g.T;
            l.am.out = tv.p; l.am.out_nstride = tv.nstride;
            l.am.a[0] = P[a].p; l.am.a_nstride[0] = P[a].nstride;
            l.am.a[1] = P[b].p; l.am.a_nstride[1] = P[b].nstride;
            l.am.C = g.C; l.am.HW = g.H * g.W;
            emit(n.bwd, l);
            P.pop_back(); P.pop_back();
            P.push_back(Addend{tv.p, tv.nstride, 1, g.H, g.W});
        }
        return true;
    }

    void conv_launches(const Node& nd, View dz, View out, bool raw, int t, bool compact) {
        const i2v_conv3d_desc& c = nd.cd;
        for (const Packed& P : nd.bwd) {
            if (compact && (P.ph || P.pw || P.pt)) continue;
            if (P.Hg <= 0 || P.Wg <= 0 || P.Tg <= 0) continue;
            Launch l; l.kind = L_CONV; conv_common(l.conv, P);
            l.node = (int)(&nd - n.nodes.data());
            I2VConvParams& p = l.conv;
            p.src = dz.p; p.src_nstride = dz.nstride; p.Hs = dz.H; p.Ws = dz.W; p.Cs = dz.C;
            p.Hg = P.Hg; p.Wg = P.Wg; p.sh = 1; p.sw = 1;
            p.Tg = P.Tg; p.Ts = dz.T; p.st = 1; l.T = P.Tg;
            p.dst = out.p; p.dst_nstride = out.nstride;
            if (compact) { p.Ho = P.Hg; p.Wo = P.Wg; p.osh = p.osw = 1; p.oh0 = p.ow0 = 0; p.To = P.Tg; }
            else {
                p.Ho = out.H; p.Wo = out.W; p.osh = p.osw = c.stride; p.oh0 = P.ph; p.ow0 = P.pw;
                p.To = out.T; p.ost = c.stride_t; p.ot0 = P.pt;
            }
            if (!raw) {
                for (const Addend& a : pending[t]) {
                    if (a.stride != 1 || p.add0 == nullptr) {
                        if (p.add0 != nullptr) { p.add1 = p.add0; p.add1_nstride = p.add0_nstride; }
                        p.add0 = a.p; p.add0_nstride = a.nstride; p.add0_stride = a.stride; p.add0_H = a.H; p.add0_W = a.W;
                    } else { p.add1 = a.p; p.add1_nstride = a.nstride; }
                }
                if (n.tens[t].post_relu) set_gate(p, t);
            }
            p.pointwise = (c.kt == 1 && c.stride_t == 1 && c.pad_t == 0 && c.kh == 1 && c.kw == 1 && c.stride == 1 &&
                           c.pad == 0 && (dz.H * dz.W) % 4 == 0 && !compact) ? 1 : 0;
            if (nd.groups > 1) l.alg_flops_per_frame = 2.0 * P.Hg * P.Wg * (double)P.Cd * P.K / nd.groups;    // dense route of a grouped node: its real products
            emit(n.bwd, l);
        }
    }
    // A grouped node as ONE k_gconv launch per pass.  `conv` mirrors the views for the analyses of i2v_tune.cpp and the timing records.
    bool gconv_launch(const Node& nd, bool backward, int t) {
#ifdef I2V_HAVE_GCONV
        const i2v_conv3d_desc& c = nd.cd;
        const int gw = c.cin / nd.groups, st = c.stride;
        View s = view(backward ? c.dst : c.src, backward), d = view(backward ? c.src : c.dst, backward);
        Launch l; l.kind = L_GCONV; l.node = (int)(&nd - n.nodes.data()); l.T = d.T;
        memset(&l.conv, 0, sizeof l.conv); memset(&l.gc, 0, sizeof l.gc);
        I2VGConvParams& q = l.gc;
        q.src = s.p; q.src_nstride = s.nstride; q.Hs = s.H; q.Ws = s.W;
        q.groups = nd.groups; q.gw = gw;
        q.dst = d.p; q.dst_nstride = d.nstride; q.Ho = d.H; q.Wo = d.W;
        conv_aux::conv_classes(q, backward, st, 9, nd.gw_tapmask);
        if (!backward) {
            q.w = nd.gw_fwd;
            q.shift = nd.shift_d; q.relu = c.relu;
            if (c.relu) { int gs = 0; if (uint32_t* g = gate_rows(c.dst, &gs)) { q.gate_out = g; q.gate_out_stride = gs; } }
        } else {
            q.w = nd.gw_bwd;
            if (n.tens[t].post_relu) {
                int gs = 0;
                if (uint32_t* g = gate_rows(t, &gs)) { q.gate = g; q.gate_stride = gs; }
                else { View a = view(t, false); q.mask = a.p; q.mask_nstride = a.nstride; }
            }
        }
        if (k_gconv_plan(&q)) { err = "a grouped convolution does not fit k_gconv (plan with I2V_GCONV=0 for the dense route)"; return false; }
        I2VConvParams& p = l.conv;
        p.src = q.src; p.src_nstride = q.src_nstride; p.Hs = q.Hs; p.Ws = q.Ws; p.Cs = c.cin;
        p.dst = q.dst; p.dst_nstride = q.dst_nstride; p.Ho = q.Ho; p.Wo = q.Wo; p.Hg = q.Ho; p.Wg = q.Wo;
        p.Cd = c.cin; p.Cdpad = c.cin; p.K = p.Kpad = 9 * gw; p.sh = p.sw = q.S; p.osh = p.osw = 1;
        p.Tg = p.Ts = p.To = p.st = p.ost = 1; p.blkt = 1; p.oct = 1; p.add0_stride = 1;
        p.shift = q.shift; p.relu = q.relu; p.gate = q.gate; p.gate_stride = q.gate_stride; p.gate_out = q.gate_out; p.gate_out_stride = q.gate_out_stride;
        p.mask = q.mask; p.mask_nstride = q.mask_nstride;
        const View o = view(c.dst, false);
        l.alg_flops_per_frame = 2.0 * o.H * o.W * (double)c.cout * gw * 9;       // the node's real products: the dense count over `groups`
        emit(backward ? n.bwd : n.fwd, l);
        return true;
#else
        (void)nd; (void)backward; (void)t;
        err = "this build has no grouped-convolution kernel";
        return false;
#endif
    }
    // A depthwise node as ONE k_dwconv launch per pass, in the same way.
    bool dwconv_launch(const Node& nd, bool backward, int t) {
#ifdef I2V_HAVE_DWCONV
        const i2v_conv3d_desc& c = nd.cd;
        const int st = c.stride, k = c.kh;
        View s = view(backward ? c.dst : c.src, backward), d = view(backward ? c.src : c.dst, backward);
        Launch l; l.kind = L_DWCONV; l.node = (int)(&nd - n.nodes.data()); l.T = d.T;
        memset(&l.conv, 0, sizeof l.conv); memset(&l.dc, 0, sizeof l.dc);
        I2VDwConvParams& q = l.dc;
        q.src = s.p; q.src_nstride = s.nstride; q.Hs = s.H; q.Ws = s.W;
        q.C = c.cin; q.k = k;
        q.dst = d.p; q.dst_nstride = d.nstride; q.Ho = d.H; q.Wo = d.W;
        conv_aux::conv_classes(q, backward, st, k * k, nd.gw_tapmask);
        if (!backward) {
            q.w = nd.gw_fwd;
            q.shift = nd.shift_d; q.relu = c.relu;
            if (c.relu) { int gs = 0; if (uint32_t* g = gate_rows(c.dst, &gs)) { q.gate_out = g; q.gate_out_stride = gs; } }
        } else {
            q.w = nd.gw_bwd;
            if (n.tens[t].post_relu) {
                int gs = 0;
                if (uint32_t* g = gate_rows(t, &gs)) { q.gate = g; q.gate_stride = gs; }
                else { View a = view(t, false); q.mask = a.p; q.mask_nstride = a.nstride; }
            }
        }
        if (k_dwconv_plan(&q)) { err = "a depthwise convolution does not fit k_dwconv (plan with I2V_DWCONV=0 for the dense route)"; return false; }
        I2VConvParams& p = l.conv;
        p.src = q.src; p.src_nstride = q.src_nstride; p.Hs = q.Hs; p.Ws = q.Ws; p.Cs = c.cin;
        p.dst = q.dst; p.dst_nstride = q.dst_nstride; p.Ho = q.Ho; p.Wo = q.Wo; p.Hg = q.Ho; p.Wg = q.Wo;
        p.Cd = c.cin; p.Cdpad = c.cin; p.K = p.Kpad = k * k; p.sh = p.sw = q.S; p.osh = p.osw = 1;
        p.Tg = p.Ts = p.To = p.st = p.ost = 1; p.blkt = 1; p.oct = 1; p.add0_stride = 1;
        p.shift = q.shift; p.relu = q.relu; p.gate = q.gate; p.gate_stride = q.gate_stride; p.gate_out = q.gate_out; p.gate_out_stride = q.gate_out_stride;
        p.mask = q.mask; p.mask_nstride = q.mask_nstride;
        const View o = view(c.dst, false);
        l.alg_flops_per_frame = 2.0 * o.H * o.W * (double)c.cout * k * k;        // the node's real products: C k k Ho Wo
        emit(backward ? n.bwd : n.fwd, l);
        return true;
#else
        (void)nd; (void)backward; (void)t;
        err = "this build has no depthwise-convolution kernel";
        return false;
#endif
    }
    // A squeeze-and-excitation node as its three launches of one pass.  Forward: x = the source, dst = the node's output (its gate rows
    // written by the scale launch).  Backward: g = the gradient of the output as the arena holds it, dst = the gradient of the source.
    bool se_launches(const Node& nd, bool backward) {
        const i2v_se_desc& d = nd.sd;
        const View x = view(d.src, false);
        Launch l; l.node = (int)(&nd - n.nodes.data()); l.T = x.T;
        memset(&l.conv, 0, sizeof l.conv); memset(&l.se, 0, sizeof l.se);
        I2VSeParams& q = l.se;
        const size_t C = (size_t)d.C, vc = align_up(N * C, 64), vr = align_up(N * (size_t)d.rd, 64);
        float* vec = base() + nd.se_off;
        q.x = x.p; q.x_nstride = x.nstride;
        q.w1 = nd.se_w1_d; q.b1 = nd.se_b1_d; q.w2t = nd.se_w2t_d; q.b2 = nd.se_b2_d;
        q.m = vec; q.h = vec + vc; q.s = vec + vc + vr; q.t = vec + 2 * vc + vr; q.dmh = vec + 3 * vc + vr;
        q.C = d.C; q.rd = d.rd; q.HW = x.H * x.W; q.backward = backward ? 1 : 0;
        l.se_vec = vec; l.se_vec_floats = nd.se_floats;
        if (!backward) {
            const View o = view(d.dst, false);
            q.dst = o.p; q.dst_nstride = o.nstride; q.relu = d.relu;
            if (d.residual >= 0) { const View r = view(d.residual, false); q.r = r.p; q.r_nstride = r.nstride; }
            if (d.relu) { int gs = 0; if (uint32_t* gr = gate_rows(d.dst, &gs)) { q.gate_out = gr; q.gate_out_stride = gs; } }
        } else {
            const View g = view(d.dst, true), gx = view(d.src, true);
            q.g = g.p; q.g_nstride = g.nstride; q.dst = gx.p; q.dst_nstride = gx.nstride;
        }
#ifdef I2V_HAVE_SE
        if (k_se_plan(&q)) { err = "a squeeze-and-excitation node does not fit its kernels"; return false; }
#else
        if (se_host::plan(&q)) { err = "a squeeze-and-excitation node does not fit"; return false; }
#endif
        std::vector<Launch>& L = backward ? n.bwd : n.fwd;
        const double plane = (double)C * q.HW;
        // algorithmic bytes per frame: squeeze reads the plane (both planes backward); excite the two matrices and the vectors; scale
        // reads the plane (+ the residual) and writes one (+ the gate bits)
        l.kind = L_SE_SQUEEZE; l.alg_flops_per_frame = (backward ? 2.0 : 1.0) * plane; l.se_bytes_per_frame = 4.0 * ((backward ? 2.0 : 1.0) * plane + C);
        emit(L, l);
        l.kind = L_SE_EXCITE; l.alg_flops_per_frame = 4.0 * C * d.rd; l.se_bytes_per_frame = 4.0 * (2.0 * C * d.rd + 3.0 * C + 2.0 * d.rd);
        emit(L, l);
        l.kind = L_SE_SCALE; l.alg_flops_per_frame = 2.0 * plane;
        l.se_bytes_per_frame = 4.0 * (2.0 * plane + 2.0 * C + ((!backward && q.r) ? plane : 0.0)) + (q.gate_out ? plane / 8.0 : 0.0);
        emit(L, l);
        return true;
    }
    bool is_hook(int t) const { for (int hk : n.hooks) if (hk == t) return true; return false; }
    static bool has_compact(const std::vector<Addend>& A) { for (auto& a : A) if (a.stride != 1) return true; return false; }

    bool contribute_conv(int t, const Node& nd, View dz) {
        left[t]--;
        View g = view(t, true);
        const i2v_conv3d_desc& c = nd.cd;
        if (nd.gconv) {
            // a bottleneck's conv1 output has the grouped conv2 as its ONLY consumer: k_gconv's epilogue takes no addends
            if (left[t] > 0 || !pending[t].empty() || has_alias[t]) { err = "the input of a grouped convolution must have it as its only consumer"; return false; }
            return gconv_launch(nd, true, t);
        }
        if (nd.dw) {
            // the 1x1 expansion's output has the depthwise node as its ONLY consumer: k_dwconv writes the gradient, it never accumulates
            // (refused on the dense route too, so that a graph plans on both routes or on neither)
            if (left[t] > 0 || !pending[t].empty() || has_alias[t]) { err = "the input of a depthwise convolution must have it as its only consumer"; return false; }
            if (nd.dwconv) return dwconv_launch(nd, true, t);
        }
        if (left[t] > 0) {
            bool compact = (c.kt == 1 && c.stride_t == 1 && c.pad_t == 0 && c.kh == 1 && c.kw == 1 && c.stride > 1 && c.pad == 0);
            if (compact) {
                const Packed& P = nd.bwd[0];
                View tv; tv.C = g.C; tv.H = P.Hg; tv.W = P.Wg; tv.T = g.T; tv.nstride = (int64_t)g.C * P.Hg * P.Wg;
                tv.p = temp(nf(g.T) * tv.nstride);
                conv_launches(nd, dz, tv, true, t, true);
                pending[t].push_back(Addend{tv.p, tv.nstride, c.stride, P.Hg, P.Wg});
            } else {
                View tv = g; tv.nstride = (int64_t)g.C * g.H * g.W; tv.p = temp(nf(g.T) * tv.nstride);
                conv_launches(nd, dz, tv, true, t, false);
                pending[t].push_back(Addend{tv.p, tv.nstride, 1, g.H, g.W});
            }
            return true;
        }
        // final contributor: at most one compact + one plain, or two plain addends fit the epilogue
        size_t ncompact = 0; for (auto& a : pending[t]) if (a.stride != 1) ncompact++;
        if (ncompact > 1) { err = "more than one strided addend"; return false; }
        if (ncompact == 1) {
            // keep the compact one, fold plain ones down to a single addend
            std::vector<Addend> plain, comp;
            for (auto& a : pending[t]) (a.stride == 1 ? plain : comp).push_back(a);
            pending[t] = plain; if (!squeeze_pending(t, 1)) return false;
            pending[t].push_back(comp[0]);
        } else if (!squeeze_pending(t, 2)) return false;
        conv_launches(nd, dz, g, false, t, false);
        pending[t].clear();
        return true;
    }

    bool contribute_alias(int t, View dz) {
        if (left[t] == 1 && pending[t].empty() && !n.tens[t].post_relu && !is_hook(t)) {
            left[t] = 0; galias[t] = dz; has_alias[t] = 1;     // sole consumer, no gate: alias the view
            return true;
        }
        left[t]--;
        pending[t].push_back(Addend{dz.p, dz.nstride, 1, dz.H, dz.W});
        if (left[t] > 0) return true;
        if (has_compact(pending[t])) { err = "alias finaliser with strided addend"; return false; }
        if (!squeeze_pending(t, 3)) return false;
        emit_addmask(view(t, true), pending[t], t);
        pending[t].clear();
        return true;
    }

    bool run() {
        const int NT = (int)n.tens.size();
        left.assign(NT, 0); pending.assign(NT, {}); galias.assign(NT, View{}); has_alias.assign(NT, 0);
        // Buffers read through a pre-activation conv (DenseNet concatenation buffers) ACCUMULATE their
        // gradient: zeroed at the start of the backward pass, every reader adds into its view.  They stay
        // outside the single-finaliser protocol (`left` / `pending`) of all other tensors.
        accum.assign(n.bufs.size(), 0);
        for (const Node& nd : n.nodes) if (nd.type == 0 && nd.preact()) accum[n.tens[nd.cd.src].buf] = 1;
        for (const Node& nd : n.nodes) {
            if (nd.type == 0) {
                if (accum[n.tens[nd.cd.src].buf] && !nd.preact()) { err = "a dense (accumulating) buffer may only be read by pre-activation convs"; return false; }
                if (!nd.preact()) left[nd.cd.src]++;
                if (nd.cd.residual >= 0) left[nd.cd.residual]++;
            } else if (nd.type == 3) {
                for (int t : {nd.ad.theta, nd.ad.phi, nd.ad.g}) {
                    if (accum[n.tens[t].buf]) { err = "attention over a dense (accumulating) buffer is not supported"; return false; }
                    left[t]++;
                }
            } else if (nd.type == 4) {
                for (int t : {nd.sd.src, nd.sd.residual}) {
                    if (t < 0) continue;
                    if (accum[n.tens[t].buf]) { err = "squeeze-and-excitation over a dense (accumulating) buffer is not supported"; return false; }
                    left[t]++;
                }
            } else {
                if (accum[n.tens[nd.pd.src].buf]) { err = "pooling directly from a dense (accumulating) buffer is not supported"; return false; }
                left[nd.pd.src]++;
            }
        }
        // A ReLU output that is only ever read through a wider concatenation view which is NOT declared post-ReLU
        // (SlowFast: max-pooled slow features ++ ReLU'd lateral features) is gated in place before its producer's
        // input-gradient runs; the covering view's finaliser cannot do it.
        std::vector<char> need_gate(NT, 0);
        for (int t = 0; t < NT; ++t) {
            if (!n.tens[t].post_relu || left[t] > 0 || is_hook(t)) continue;
            for (int u = 0; u < NT; ++u)
                if (u != t && left[u] > 0 && !n.tens[u].post_relu && overlaps(n.tens[u], n.tens[t])) need_gate[t] = 1;
        }
        int img_seen = 0;
        // ---------------- forward ----------------
        for (const Node& nd : n.nodes) {
            Launch l;
            if (nd.type == 4) { if (!se_launches(nd, false)) return false; continue; }
            if (nd.type == 0) {
                const i2v_conv3d_desc& c = nd.cd;
                if (nd.gconv) { if (!gconv_launch(nd, false, c.dst)) return false; continue; }
                if (nd.dwconv) { if (!dwconv_launch(nd, false, c.dst)) return false; continue; }
                l.kind = L_CONV; conv_common(l.conv, nd.fwd);
                l.node = (int)(&nd - n.nodes.data());
                I2VConvParams& p = l.conv;
                View d = view(c.dst, false);
                const Buffer& sb = n.bufs[n.tens[c.src].buf];
                if (c.src == n.input) { l.src_is_input = true; p.src = nullptr; p.src_nstride = (int64_t)sb.C * sb.H * sb.W; }
                else { View s = view(c.src, false); p.src = s.p; p.src_nstride = s.nstride; }
                p.Hs = sb.H; p.Ws = sb.W; p.Cs = c.cin; p.Hg = d.H; p.Wg = d.W; p.sh = p.sw = c.stride;
                p.dst = d.p; p.dst_nstride = d.nstride; p.Ho = d.H; p.Wo = d.W; p.osh = p.osw = 1;
                p.Tg = p.To = d.T; p.Ts = sb.T; p.st = c.stride_t; l.T = d.T;
                if (nd.fwd.tpair) {              // two output frames per grid frame (pack_fwd): class-packed epilogue, blk = 1
                    p.Tg = (d.T + 1) / 2; l.T = p.Tg; p.st = 2 * c.stride_t; p.ost = 2; p.ot0 = 0; p.blkt = 2; p.blk = 1;
                }
                p.shift = nd.shift_d; p.relu = c.relu;
                if (c.residual >= 0) { View r = view(c.residual, false); p.add0 = r.p; p.add0_nstride = r.nstride; p.add0_stride = 1; }
                p.pointwise = (c.kt == 1 && c.stride_t == 1 && c.pad_t == 0 && c.kh == 1 && c.kw == 1 && c.stride == 1 &&
                               c.pad == 0 && (sb.H * sb.W) % 4 == 0 && c.src != n.input) ? 1 : 0;
                if (nd.preact()) { p.pre_scale = nd.pre_scale_d; p.pre_shift = nd.pre_shift_d; }
                if (c.relu) { int st = 0; if (uint32_t* g = gate_rows(c.dst, &st)) { p.gate_out = g; p.gate_out_stride = st; p.gate_out_pix0 = 0; } }
                if (nd.groups > 1) l.alg_flops_per_frame = 2.0 * d.H * d.W * c.cout * (double)c.cin * c.kh * c.kw / nd.groups;    // dense route of a grouped node: its real products
                if (nd.fwd.quad) l.alg_flops_per_frame = 2.0 * d.H * d.W * c.cout * (double)c.cin * c.kt * c.kh * c.kw * d.T / p.Tg;   // per GRID frame
            } else if (nd.type == 3) {
                // S = scale * theta^T phi  ->  P = softmax rows  ->  y = g P^T   (P stays in the arena for the backward pass)
                View th = view(nd.ad.theta, false), ph = view(nd.ad.phi, false), gv = view(nd.ad.g, false), y = view(nd.ad.dst, false);
                const int M = th.T * th.H * th.W, Nn = ph.T * ph.H * ph.W;
                float* P = base() + nd.p_off;
                Launch a; a.kind = L_AGEMM; memset(&a.ag, 0, sizeof a.ag); a.T = th.T;
                a.ag.form = 1; a.ag.Cc = th.C; a.ag.M = M; a.ag.N = Nn; a.ag.scale = nd.ad.scale;
                a.ag.A = I2VActMat{th.p, th.nstride, th.T, th.H * th.W}; a.ag.B = I2VActMat{ph.p, ph.nstride, ph.T, ph.H * ph.W}; a.ag.D = P;
                emit(n.fwd, a);
                Launch sm; sm.kind = L_SOFTMAX; memset(&sm.sm, 0, sizeof sm.sm); sm.T = th.T;
                sm.sm.X = P; sm.sm.N = Nn; sm.sm.mode = 0; sm.sm_rows_per_clip = M;
                emit(n.fwd, sm);
                l.kind = L_AGEMM; memset(&l.ag, 0, sizeof l.ag); l.T = th.T;
                l.ag.form = 2; l.ag.Cc = th.C; l.ag.M = M; l.ag.N = Nn; l.ag.scale = 1.f;
                l.ag.A = I2VActMat{gv.p, gv.nstride, gv.T, gv.H * gv.W}; l.ag.Din = P;
                l.ag.Cact = y.p; l.ag.C_nstride = y.nstride; l.ag.C_T = y.T; l.ag.C_HW = y.H * y.W;
            } else {
                const i2v_pool3d_desc& q = nd.pd;
                const bool vid = q.kt != 1 || q.stride_t != 1 || q.pad_t != 0;
                if (vid && nd.type == 2) { err = "average pooling over time is not supported"; return false; }
                l.kind = nd.type == 2 ? L_AVGF : vid ? L_POOL3F : L_POOLF; memset(&l.pool, 0, sizeof l.pool);
                View s = view(q.src, false), d = view(q.dst, false);
                if (q.src == n.input) { err = "maxpool directly on the input is not supported"; return false; }
                l.pool.x = s.p; l.pool.x_nstride = s.nstride; l.pool.C = s.C; l.pool.Hs = s.H; l.pool.Ws = s.W;
                l.pool.y = d.p; l.pool.y_nstride = d.nstride; l.pool.Ho = d.H; l.pool.Wo = d.W;
                l.pool.k = q.k; l.pool.stride = q.stride; l.pool.pad = q.pad;
                l.pool.kt = q.kt; l.pool.stride_t = q.stride_t; l.pool.pad_t = q.pad_t; l.pool.Ts = s.T; l.pool.To = d.T;
                l.pool.idx = (uint8_t*)(base() + nd.idx_off);
                l.T = d.T;
            }
            emit(n.fwd, l);
        }
        // ---------------- hooks ----------------
        hook_tmp.assign(n.hooks.size(), nullptr);
        for (size_t hk = 0; hk < n.hooks.size(); ++hk) {
            int t = n.hooks[hk];
            bool consumed = false;
            for (const Node& nd : n.nodes) {
                int srcs[3] = {nd.src0(), nd.type == 3 ? nd.ad.phi : nd.residual0(), nd.type == 3 ? nd.ad.g : -1};
                for (int s : srcs) if (s >= 0 && overlaps(n.tens[s], n.tens[t])) consumed = true;
            }
            if (consumed || accum[n.tens[t].buf]) { View g = view(t, true); hook_tmp[hk] = temp(nf(g.T) * g.C * g.H * g.W); }
        }
        // ---------------- backward ----------------
        for (const Node& nd : n.nodes)
            if (nd.type == 0 && nd.cd.src == n.input && !nd.imgs.empty() && nd.imgs[0].skips) {     // a stem gradient that skips frames
                const Buffer& ib = n.bufs[n.tens[n.input].buf];
                Launch l; l.kind = L_MEMSET; l.ms_gx = true; l.ms_floats_per_frame = (size_t)ib.C * ib.H * ib.W; l.T = ib.T;
                emit(n.bwd, l);
                break;
            }
        for (size_t b = 0; b < n.bufs.size(); ++b)
            if (accum[b]) {
                Launch l; l.kind = L_MEMSET;
                l.ms_ptr = base() + n.bufs[b].grad_off; l.ms_floats_per_frame = (size_t)n.bufs[b].C * n.bufs[b].H * n.bufs[b].W;
                l.T = n.bufs[b].T;
                emit(n.bwd, l);
            }
        for (size_t hk = 0; hk < n.hooks.size(); ++hk)          // hook gradients of dense buffers: G += H right away
            if (accum[n.tens[n.hooks[hk]].buf]) {
                const int t = n.hooks[hk];
                View g = view(t, true);
                std::vector<Addend> adds = {Addend{g.p, g.nstride, 1, g.H, g.W},
                                            Addend{hook_tmp[hk], (int64_t)g.C * g.H * g.W, 1, g.H, g.W}};
                emit_addmask(g, adds, t);
            }
        for (int i = (int)n.nodes.size() - 1; i >= 0; --i) {
            const Node& nd = n.nodes[i];
            int dst = nd.dst0();
            // a hook gradient kept in a side buffer joins the gradient of every node output the hooked view COVERS:
            // the hooked tensor itself, or -- a hooked concatenation (SqueezeNet Fire output = expand1x1 ++ expand3x3,
            // TPAMI_attack.py:195-197) -- each branch's channel slice of it
            for (size_t hk = 0; hk < n.hooks.size(); ++hk) {
                const Tensor& HT = n.tens[n.hooks[hk]]; const Tensor& DT = n.tens[dst];
                const bool covers = HT.buf == DT.buf && HT.c_off <= DT.c_off && DT.c_off + DT.C <= HT.c_off + HT.C;
                if (covers && hook_tmp[hk] && !accum[DT.buf]) {
                    View g = view(dst, true);
                    const int64_t hD = (int64_t)HT.C * g.H * g.W;
                    std::vector<Addend> adds = {Addend{g.p, g.nstride, 1, g.H, g.W},
                                                Addend{hook_tmp[hk] + (size_t)(DT.c_off - HT.c_off) * g.H * g.W, hD, 1, g.H, g.W}};
                    emit_addmask(g, adds, dst);
                }
            }
            View dz = view(dst, true);
            if (need_gate[dst]) emit_addmask(dz, {Addend{dz.p, dz.nstride, 1, dz.H, dz.W}}, dst);
            // a backward gain on this node's ReLU (i2v_net_set_relu_gain): G(dst) is complete and gated here -- every consumer and
            // hook has contributed, the finaliser applied the gate -- so the gain is one in-place pass in front of the node's own
            // input-gradient work (the gate is 0 or 1: gain * gate * g, whichever is applied first)
            if (n.tens[dst].bwd_gain != 1.f) {
                if (accum[n.tens[dst].buf] || has_alias[dst]) { err = "a ReLU gain on an accumulating or aliased gradient view is not planned"; return false; }
                Launch l; memset(&l.am, 0, sizeof l.am); l.kind = L_ADDMASK; l.T = dz.T;
                l.am.out = dz.p; l.am.out_nstride = dz.nstride; l.am.a[0] = dz.p; l.am.a_nstride[0] = dz.nstride;
                l.am.C = dz.C; l.am.HW = dz.H * dz.W; l.am.gain = n.tens[dst].bwd_gain;
                emit(n.bwd, l);
            }
            if (nd.type == 0) {
                const i2v_conv3d_desc& c = nd.cd;
                if (c.residual >= 0 && !contribute_alias(c.residual, dz)) return false;
                if (c.src == n.input) {
                    const bool acc_node = img_seen++ > 0;          // (a node's temporal classes write disjoint frames: one flag for all of them)
                    for (const Node::ImgGrad& ig : nd.imgs) {
                    Launch l; l.kind = L_IMGGRAD; conv_common(l.conv, ig.P);
                    l.img_accumulate = acc_node;
                    const Buffer& ib = n.bufs[n.tens[n.input].buf];
                    I2VConvParams& p = l.conv;
                    p.src = dz.p; p.src_nstride = dz.nstride; p.Hs = dz.H; p.Ws = dz.W; p.Cs = dz.C;
                    p.Hg = ig.P.Hg; p.Wg = ig.P.Wg; p.sh = p.sw = ig.sh;
                    p.dst = nullptr; p.dst_nstride = (int64_t)ib.C * ib.H * ib.W; p.Ho = ib.H; p.Wo = ib.W;
                    p.osh = p.osw = ig.blk; p.blk = ig.blk;
                    p.blkt = ig.blkt; p.Tg = ig.P.Tg; p.Ts = dz.T; p.st = ig.st; p.To = ib.T; p.ost = ig.ost; p.ot0 = ig.ot0; p.oct = ig.oct; l.T = ig.P.Tg;
                    l.alg_flops_per_frame = ig.flop_share * 2.0 * dz.T * dz.H * dz.W * c.cout * c.cin * c.kt * c.kh * c.kw / ig.P.Tg;   // per grid frame
                    emit(n.bwd, l);
                    }
                } else if (nd.preact()) {
                    // G(view) += W'^T dz gated by the pre-activation sign; W' carries the BN scale per input channel
                    View g = view(c.src, true), x = view(c.src, false);
                    Launch l; l.kind = L_CONV; conv_common(l.conv, nd.bwd[0]);
                    I2VConvParams& p = l.conv;
                    p.src = dz.p; p.src_nstride = dz.nstride; p.Hs = dz.H; p.Ws = dz.W; p.Cs = dz.C;
                    p.Hg = g.H; p.Wg = g.W; p.sh = p.sw = 1;
                    p.dst = g.p; p.dst_nstride = g.nstride; p.Ho = g.H; p.Wo = g.W; p.osh = p.osw = 1;
                    p.Tg = p.Ts = p.To = g.T; l.T = g.T;
                    p.add1 = g.p; p.add1_nstride = g.nstride;
                    p.mask = x.p; p.mask_nstride = x.nstride; p.gate_scale = nd.pre_scale_d; p.gate_shift = nd.pre_shift_d;
                    p.pointwise = ((dz.H * dz.W) % 4 == 0) ? 1 : 0;
                    emit(n.bwd, l);
                } else if (!contribute_conv(c.src, nd, dz)) return false;
            } else if (nd.type == 4) {
                const i2v_se_desc& q = nd.sd;
                // the residual's share is G itself: the alias a convolution with a residual hands on (its finalising launch adds it)
                if (q.residual >= 0 && !contribute_alias(q.residual, dz)) return false;
                // the node WRITES the gradient of its source and never accumulates: nothing else may contribute to it
                const int t = q.src;
                left[t]--;
                if (left[t] > 0 || !pending[t].empty() || has_alias[t] || is_hook(t)) {
                    err = "the source of a squeeze-and-excitation node (tensor " + std::to_string(t) + ") must have the node as its only consumer";
                    return false;
                }
                if (!se_launches(nd, true)) return false;
            } else if (nd.type == 3) {
                // dY = dz.  dP = dY^T g;  dg = dY P;  dS = P o (dP - rowsum(dP o P));  dtheta = phi dS^T;  dphi = theta dS
                for (int t : {nd.ad.theta, nd.ad.phi, nd.ad.g})
                    if (left[t] != 1 || !pending[t].empty() || is_hook(t)) { err = "attention operands must have the attention node as their only consumer"; return false; }
                View th = view(nd.ad.theta, false), ph = view(nd.ad.phi, false), gv = view(nd.ad.g, false);
                View dth = view(nd.ad.theta, true), dph = view(nd.ad.phi, true), dgv = view(nd.ad.g, true);
                const int M = th.T * th.H * th.W, Nn = ph.T * ph.H * ph.W;
                float* P = base() + nd.p_off;
                float* dP = temp(nf(th.T) / th.T * (size_t)M * Nn);
                auto act = [](const View& v) { return I2VActMat{v.p, v.nstride, v.T, v.H * v.W}; };
                auto gemm = [&](int form, I2VActMat A, const I2VActMat* B, float* D, const float* Din, const View* out) {
                    Launch l; l.kind = L_AGEMM; memset(&l.ag, 0, sizeof l.ag); l.T = th.T;
                    l.ag.form = form; l.ag.Cc = th.C; l.ag.M = M; l.ag.N = Nn; l.ag.scale = form == 1 ? nd.ad.scale : 1.f; l.ag.A = A;
                    if (B) l.ag.B = *B;
                    l.ag.D = D; l.ag.Din = Din;
                    if (out) { l.ag.Cact = out->p; l.ag.C_nstride = out->nstride; l.ag.C_T = out->T; l.ag.C_HW = out->H * out->W; }
                    // few output tiles per clip under a long reduction (dg, dphi: Cc x N outputs summed over the M positions): cut K.
                    // The cut depends on the clip's own shape only, so a clip's result does not depend on the batch it is in.
                    const int cols = form == 2 ? M : Nn, K = form == 2 ? Nn : M;
                    const int tiles = ((th.C + 63) / 64) * ((cols + 63) / 64);
                    if (form != 1 && tiles <= 128 && K >= 512) {
                        l.ag.ksplit = std::min(8, K / 256);
                        l.ag.part = temp(nf(th.T) / th.T * (size_t)l.ag.ksplit * th.C * cols);
                    }
                    emit(n.bwd, l);
                };
                const I2VActMat gA = act(gv);
                // (the softmax backward works on d(scale * theta^T phi): the scale reaches dtheta / dphi through dS below)
                { Launch l; l.kind = L_AGEMM; memset(&l.ag, 0, sizeof l.ag); l.T = th.T; l.ag.form = 1; l.ag.Cc = th.C; l.ag.M = M; l.ag.N = Nn;
                  l.ag.scale = 1.f; l.ag.A = act(dz); l.ag.B = gA; l.ag.D = dP; emit(n.bwd, l); }
                gemm(3, act(dz), nullptr, nullptr, P, &dgv);
                { Launch l; l.kind = L_SOFTMAX; memset(&l.sm, 0, sizeof l.sm); l.T = th.T; l.sm.X = dP; l.sm.P = P; l.sm.N = Nn; l.sm.mode = 1;
                  l.sm_rows_per_clip = M; emit(n.bwd, l); }
                if (nd.ad.scale != 1.f) { err = "attention: only scale 1 is planned (gluoncv's gaussian non-local block has none)"; return false; }
                gemm(2, act(ph), nullptr, nullptr, dP, &dth);
                gemm(3, act(th), nullptr, nullptr, dP, &dph);
                left[nd.ad.theta] = left[nd.ad.phi] = left[nd.ad.g] = 0;
            } else {
                const i2v_pool3d_desc& q = nd.pd;
                const bool vid = q.kt != 1 || q.stride_t != 1 || q.pad_t != 0;
                left[q.src]--;
                const bool shared = left[q.src] > 0 || !pending[q.src].empty();      // other consumers contribute to this gradient too
                Launch l; l.kind = nd.type == 2 ? L_AVGB : vid ? L_POOL3B : L_POOLB; memset(&l.pool, 0, sizeof l.pool);
                View x = view(q.src, false), gx = view(q.src, true);
                if (shared) {       // (non-local block: x feeds theta, the 1x2x2 max-pool in front of phi / g, and the residual)
                    if (left[q.src] == 0) { err = "a max-pool must not be the last contributor to a shared gradient (order the graph's nodes so that a convolution is)"; return false; }
                    gx.nstride = (int64_t)gx.C * gx.H * gx.W; gx.p = temp(nf(gx.T) * gx.nstride);
                    pending[q.src].push_back(Addend{gx.p, gx.nstride, 1, gx.H, gx.W});
                }
                l.pool.x = x.p; l.pool.x_nstride = x.nstride; l.pool.C = x.C; l.pool.Hs = x.H; l.pool.Ws = x.W;
                l.pool.y = dz.p; l.pool.y_nstride = dz.nstride; l.pool.Ho = dz.H; l.pool.Wo = dz.W;
                l.pool.gx = gx.p; l.pool.gx_nstride = gx.nstride;
                l.pool.k = q.k; l.pool.stride = q.stride; l.pool.pad = q.pad;
                l.pool.mask_relu = (n.tens[q.src].post_relu && !shared) ? 1 : 0;        // (shared: the finaliser applies the gate)
                if (l.pool.mask_relu && nd.type == 1) { View ya = view(q.dst, false); l.pool.yact = ya.p; l.pool.yact_nstride = ya.nstride; }
                l.pool.kt = q.kt; l.pool.stride_t = q.stride_t; l.pool.pad_t = q.pad_t; l.pool.Ts = x.T; l.pool.To = dz.T;
                l.pool.idx = (uint8_t*)(base() + nd.idx_off);
                l.T = dz.T;
                emit(n.bwd, l);
            }
        }
        return true;
    }
};

}  // namespace

bool plan_pass(Net& n, bool dry, size_t off, size_t N, size_t* end, std::string* err) {
    Planner p{n, dry, off, N};
    if (!p.run()) { *err = p.err; return false; }
    *end = p.off;
    if (!dry) n.hook_tmp = p.hook_tmp;
    return true;
}

}  // namespace eng
