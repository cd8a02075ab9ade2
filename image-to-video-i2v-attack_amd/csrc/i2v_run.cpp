// The executor: a planned launch list on a stream, its timing instrumentation, and the read-back entries.
#include "i2v_net.h"
#ifndef I2V_HAVE_SE
#include "i2v_se_host.h"         // (the host simulation's one-file build: the squeeze-and-excitation node as scalar code)
#endif
#ifndef I2V_HAVE_SCPAIR
#include "i2v_scpair_host.h"     // (... and the shortcut pair as its two launches)
#endif

#include <stdio.h>
#include <stdlib.h>

#include <algorithm>

using namespace eng;

namespace eng {

// ---------------------------------------------------------------------------------------------
// execution
// ---------------------------------------------------------------------------------------------
// A launch's parameters as the kernel sees them: the caller's input / gradient pointers patched in, the dense-epilogue and temporal
// flags derived (shared by the plain launch and the fused pair)
I2VConvParams conv_prep(const Launch& l, const float* x, float* gx, int accumulate) {
    I2VConvParams p = l.conv;
    if (l.src_is_input) p.src = x;
    if (l.kind == L_IMGGRAD) { p.dst = gx; if (accumulate || l.img_accumulate) { p.add1 = gx; p.add1_nstride = p.dst_nstride; } }
    p.vec_epilogue = (p.blk <= 1 && p.osh == 1 && p.osw == 1 && p.oh0 == 0 && p.ow0 == 0 && p.Hg == p.Ho &&
                      p.Wg == p.Wo && p.Tg == p.To && p.ost == 1 && p.ot0 == 0 &&
                      (p.Ho * p.Wo) % 4 == 0 && p.dst_nstride % 4 == 0 &&
                      (p.add0_stride == 1 || (p.add0_stride == 2 && p.Wo % 4 == 0 && p.add0_W * 2 == p.Wo &&
                                              p.add0_W % 2 == 0 && (p.add0_H * p.add0_W) % 2 == 0)) &&
                      p.add0_nstride % 4 == 0 && p.add1_nstride % 4 == 0 && p.mask_nstride % 4 == 0 &&
                      (((uintptr_t)p.dst | (uintptr_t)p.add0 | (uintptr_t)p.add1 | (uintptr_t)p.mask) & 15) == 0)
                         ? 1 : 0;
    if (!(p.Tg == p.Ts && p.Ts == p.To && p.st == 1 && p.ost == 1 && p.ot0 == 0 && p.blkt == 1)) p.temporal = 1;
    return p;
}

// what a launch over `frames` grid frames addresses of its source, first byte to last (32-bit buffer offsets: it has to stay < 2 GiB)
static int64_t src_span_bytes(const I2VConvParams& p, int frames) {
    return ((int64_t)frames * p.Ts / p.Tg - 1) * p.src_nstride * 4 + (int64_t)p.Cs * p.Hs * p.Ws * 4;
}

// The fused pair: `a` (3x3) and `b` (the pointwise convolution over a's output) as ONE launch; only for pairs mark_fusable admitted.
// A pair whose source would have to be sliced (>= 2 GiB spans) is not fused (the caller falls back to two launches).
bool fused_fits(const Launch& a, const Launch& b, int frames) {
    return src_span_bytes(a.conv, frames) < (1ll << 31) && src_span_bytes(b.conv, frames) < (1ll << 31);
}
int fused_run(const Launch& a, const Launch& b, int frames, const float* x, int halo, i2v_stream_t s) {
    I2VConvParams pa = conv_prep(a, x, nullptr, 0), pb = conv_prep(b, x, nullptr, 0);
    for (I2VConvParams* p : {&pa, &pb}) { p->N = frames; p->src_span_bytes = (int32_t)src_span_bytes(*p, frames); }
    CHECK_BE(k_conv_fused(pa, pb, halo, s));
    return 0;
}

// The shortcut pair: `a` (a 1x1 convolution) and `b` (the pointwise convolution whose plain addend is a's output) as ONE launch that
// never stores that output; only for pairs mark_fusable admitted.  A pair whose sources would have to be sliced runs as two launches.
static void sc_prep(const Launch& a, const Launch& b, int frames, I2VConvParams* pa, I2VConvParams* pb) {
    *pa = conv_prep(a, nullptr, nullptr, 0); *pb = conv_prep(b, nullptr, nullptr, 0);
    for (I2VConvParams* p : {pa, pb}) { p->N = frames; p->src_span_bytes = (int32_t)src_span_bytes(*p, frames); }
}
bool sc_pair_ok(const Launch& a, const Launch& b) {
    if (a.kind != L_CONV || b.kind != L_CONV || a.src_is_input || b.src_is_input || a.T != b.T) return false;
    I2VConvParams pa, pb;
    sc_prep(a, b, a.T, &pa, &pb);
#ifdef I2V_HAVE_SCPAIR
    return k_conv_scpair_ok(pa, pb) != 0;
#else
    return scpair_host::ok(pa, pb) != 0;
#endif
}
bool sc_fits(const Launch& a, const Launch& b, int frames) { return fused_fits(a, b, frames); }
int sc_run(const Launch& a, const Launch& b, int frames, i2v_stream_t s) {
    I2VConvParams pa, pb;
    sc_prep(a, b, frames, &pa, &pb);
#ifdef I2V_HAVE_SCPAIR
    CHECK_BE(k_conv_scpair(pa, pb, s));
#else
    if (scpair_host::run(pa, pb, s)) return fail("shortcut pair: the two launches do not form a pair");
#endif
    return 0;
}

// The fused fast-pathway block: launches L[li] .. L[li + fb_ok - 1] as ONE kernel.  Returns 0 done, 1 error, 2 not eligible at this frame
// count (the caller runs the separate launches).
int fast_run(const std::vector<Launch>& L, size_t li, int frames, const float* x, i2v_stream_t s) {
    const int g = L[li].fb_ok;
    I2VConvParams q[4];
    for (int j = 0; j < g; ++j) { q[j] = conv_prep(L[li + j], x, nullptr, 0); q[j].N = frames; }
    const I2VConvParams* c = g == 3 ? &q[2] : g == 4 ? &q[3] : nullptr;
    const I2VConvParams* d = g == 4 ? &q[2] : nullptr;
    if (i2v_fastblock_rows(q[0], q[1], c, d) <= 0) return 2;
    if (k_fastblock(q[0], q[1], c, d, s)) { fail("k_fastblock: %s", be_error() ? be_error() : "backend error"); return 1; }
    return 0;
}

// One convolution launch over `frames` grid frames (= clips * Tg), possibly sliced over whole clips: 32-bit
// buffer offsets keep a launch's source span < 2 GiB
int conv_run(const Launch& l, int frames, const float* x, float* gx, int accumulate, i2v_stream_t s) {
    I2VConvParams p = conv_prep(l, x, gx, accumulate);
    const int clips = frames / p.Tg;
    const int64_t plane_bytes = (int64_t)p.Cs * p.Hs * p.Ws * 4, stride_bytes = p.src_nstride * 4;
    const int64_t clip_bytes = (int64_t)(p.Ts - 1) * stride_bytes + plane_bytes;        // span of one clip's source frames
    int64_t per = clip_bytes >= (1ll << 31) ? 0 : 1 + ((1ll << 31) - 1 - clip_bytes) / (stride_bytes * p.Ts);
    if (per < 1) return fail("one clip of a convolution input exceeds 2 GiB");
    if (per < clips && (p.gate || p.gate_out)) {        // a slice must start on a 32-bit boundary of the gate rows
        per -= per % 32;
        if (per < 1) return fail("a sliced convolution launch cannot keep its gate rows word-aligned");
    }
    for (int c0 = 0; c0 < clips; c0 += (int)per) {
        I2VConvParams q = p;
        const int nc = clips - c0 < per ? clips - c0 : (int)per;
        q.N = nc * p.Tg;
        q.src += (int64_t)c0 * p.Ts * p.src_nstride; q.dst += (int64_t)c0 * p.To * p.dst_nstride;
        if (q.add0) q.add0 += (int64_t)c0 * p.To * p.add0_nstride;
        if (q.add1) q.add1 += (int64_t)c0 * p.To * p.add1_nstride;
        if (q.mask) q.mask += (int64_t)c0 * p.To * p.mask_nstride;
        q.gate_pix0 = p.gate_pix0 + (int32_t)((int64_t)c0 * p.To * p.Ho * p.Wo);
        q.gate_out_pix0 = p.gate_out_pix0 + (int32_t)((int64_t)c0 * p.To * p.Ho * p.Wo);
        q.src_span_bytes = (int32_t)((int64_t)(nc * p.Ts - 1) * stride_bytes + plane_bytes);
        CHECK_BE(k_conv(q, s));
    }
    return 0;
}

}  // namespace eng

long long eng::g_overlap_launches = 0;

static TimedLaunch* timing_begin(i2v_ctx* h, int kind, double flops, i2v_stream_t s, TimedLaunch* prev) {
    if (!h->timing) return nullptr;
    TimedLaunch* t;
    {
        std::lock_guard<std::mutex> lock(h->timing_mu);
        if (h->timed_used == h->timed.size()) {
            TimedLaunch fresh{be_event_create(), be_event_create(), 0, 0.0, 0, 0, 0, 0, 0, nullptr, 0.0, 1};
            if (!fresh.start || !fresh.stop) return nullptr;
            h->timed.push_back(fresh);
        }
        t = &h->timed[h->timed_used++];
    }
    t->kind = kind; t->flops = flops; t->Cd = t->K = t->HWg = t->frames = t->pw = 0; t->bytes = 0.0; t->count = 1;
    t->chain_from = prev ? prev->stop : nullptr;
    if (!t->chain_from) be_event_record(t->start, s);
    return t;
}

// What the timing instrumentation records about a launch -- or about the fused group it leads: `fb` launches of L from li as one fused
// fast-pathway block, `fuse`: li and li + 1 as one fused pair.  Only computed while launches are being timed.
// `sc`: the launch leads a shortcut pair -- L[sc] (earlier in the list) runs inside it; -1: none.
static double launch_flops(const std::vector<Launch>& L, size_t li, int fb, int fuse, int sc, int frames, int clips) {
    const Launch& l = L[li];
    double flops = 0.0;
    if (sc >= 0) return 2.0 * frames * l.conv.Hg * l.conv.Wg * ((double)l.conv.Cd * l.conv.K + (double)L[sc].conv.Cd * L[sc].conv.K);
    if (fb) { for (int j = 0; j < fb; ++j) { const Launch& m = L[li + j]; flops += m.alg_flops_per_frame > 0 ? m.alg_flops_per_frame * frames : 2.0 * frames * m.conv.Hg * m.conv.Wg * (double)m.conv.Cd * m.conv.K; } }
    else if ((l.kind == L_CONV || l.kind == L_GCONV || l.kind == L_DWCONV) && l.alg_flops_per_frame > 0) flops = l.alg_flops_per_frame * frames;     // quad-row packings pad K; a grouped node counts its real products
    else if (l.kind == L_CONV) flops = 2.0 * frames * l.conv.Hg * l.conv.Wg * ((double)l.conv.Cd * l.conv.K + (fuse ? (double)L[li + 1].conv.Cd * L[li + 1].conv.K : 0.0));
    else if (l.kind == L_IMGGRAD) flops = l.alg_flops_per_frame * frames;
    else if (l.kind == L_AGEMM) flops = 2.0 * clips * (double)l.ag.Cc * l.ag.M * l.ag.N;
    else if (l.kind == L_SE_SQUEEZE || l.kind == L_SE_EXCITE || l.kind == L_SE_SCALE) flops = l.alg_flops_per_frame * frames;
    return flops;
}

// timing kinds: 0 conv fwd, 1 image gradient, 2 pool fwd, 3 pool bwd, 4 addmask, 5 conv input-gradient
static int launch_timing_kind(const Launch& l, bool backward_pass) {
    switch (l.kind) {
        case L_CONV: case L_AGEMM: case L_GCONV: case L_DWCONV: return backward_pass ? 5 : 0;
        case L_IMGGRAD: return 1;
        case L_POOLF: case L_AVGF: case L_POOL3F: return 2;
        case L_POOLB: case L_AVGB: case L_POOL3B: return 3;
        case L_ADDMASK: case L_MEMSET: case L_SOFTMAX: return 4;
        case L_SE_SQUEEZE: case L_SE_EXCITE: case L_SE_SCALE: return 4;        // (elementwise and reductions: with the add / mask launches)
    }
    return 4;
}

// ALGORITHMIC bytes of a convolution launch (or the fused group it leads): every operand once -- the source view, the packed weights,
// the output, each epilogue addend, and the ReLU gate (fp32 activation, or 1 bit per element) -- whatever the tiling re-reads
static double launch_bytes(const std::vector<Launch>& L, size_t li, int fb, int fuse, int sc, int frames, int clips, int accumulate) {
    const Launch& l = L[li];
    const I2VConvParams& q = l.conv;
    const double out = (double)frames * q.Hg * q.Wg * q.Cd;
    const double src = (double)clips * q.Ts * q.Cs * q.Hs * q.Ws;
    double b = 4.0 * (src + (double)q.K * q.Cd + out);
    if (q.add0) b += 4.0 * out / (q.add0_stride * q.add0_stride);
    if (q.add1 || l.kind == L_IMGGRAD) b += (q.add1 || accumulate || l.img_accumulate) ? 4.0 * out : 0.0;
    if (q.mask) b += 4.0 * out;
    if (q.gate) b += out / 8.0;
    if (q.gate_out) b += out / 8.0;
    if (fb) {         // a fused fast-pathway block: its source, every member's weights and gate words, the last member's output (+ an identity residual)
        const I2VConvParams& last = L[li + fb - 1].conv;
        const double outl = (double)frames * last.Hg * last.Wg * last.Cd;
        b = 4.0 * (src + outl);
        for (int j = 0; j < fb; ++j) {
            const I2VConvParams& r = L[li + j].conv;
            const double o = (double)frames * r.Hg * r.Wg * r.Cd;
            b += 4.0 * (double)r.K * r.Cd + (r.gate ? o / 8.0 : 0.0) + (r.gate_out ? o / 8.0 : 0.0);
        }
        if (fb == 3) b += 4.0 * outl;
    }
    if (fuse) {       // + the pointwise half: its weights, output and epilogue operands; the intermediate is neither written nor read
        const I2VConvParams& r = L[li + 1].conv;
        const double out2 = (double)frames * r.Hg * r.Wg * r.Cd;
        b += 4.0 * ((double)r.K * r.Cd + out2) - 4.0 * out;
        if (r.add0) b += 4.0 * out2;
        if (r.add1) b += 4.0 * out2;
        if (r.mask) b += 4.0 * out2;
        if (r.gate) b += out2 / 8.0;
        if (r.gate_out) b += out2 / 8.0;
    }
    if (sc >= 0) {    // + the shortcut half: its source and weights; its output, this launch's add0, is neither written nor read
        const I2VConvParams& r = L[sc].conv;
        b += 4.0 * ((double)clips * r.Ts * r.Cs * r.Hs * r.Ws + (double)r.K * r.Cd) - 4.0 * out;
    }
    return b;
}

namespace {

// The timing entries of one list.  Mode 1: one entry per launch, chained to the entry before it.  Segment mode
// (i2v_timing_enable(h, 2)): consecutive launches of one kind share ONE event pair -- a forward list is three or four segments
// instead of fifty event records -- and the segment accumulates their flops / bytes / count; the per-launch fields of a dump line
// and the low-intensity split need mode 1.
struct ListTiming {
    i2v_ctx* h; i2v_stream_t s; bool backward_pass;
    TimedLaunch* prev = nullptr;        // mode 1: the entry before (null: the next one records its own start event)
    TimedLaunch* seg = nullptr;         // segment mode: the open segment

    // the entry whose stop event is due right behind the launch (mode 1), or null
    TimedLaunch* open(const std::vector<Launch>& L, size_t li, int fb, int fuse, int sc, int frames, int clips, int accumulate) {
        const Launch& l = L[li];
        const int kind = launch_timing_kind(l, backward_pass);
        const double flops = launch_flops(L, li, fb, fuse, sc, frames, clips);
        const bool conv = l.kind == L_CONV || l.kind == L_IMGGRAD || l.kind == L_GCONV || l.kind == L_DWCONV;
        if (h->timing == 2) {
            if (!seg || seg->kind != kind) {
                close();
                seg = timing_begin(h, kind, 0.0, s, seg);
                if (seg) seg->count = 0;
            }
            if (seg) { seg->flops += flops; seg->count += 1; if (conv) seg->bytes += launch_bytes(L, li, fb, fuse, sc, frames, clips, accumulate); else seg->bytes += l.se_bytes_per_frame * frames; }
            return prev = nullptr;
        }
        TimedLaunch* const tl = prev = timing_begin(h, kind, flops, s, prev);
        if (tl && conv) {
            tl->Cd = l.conv.Cd; tl->K = l.conv.K; tl->HWg = l.conv.Hg * l.conv.Wg; tl->frames = frames; tl->pw = l.conv.pointwise;
            tl->bytes = launch_bytes(L, li, fb, fuse, sc, frames, clips, accumulate);
        }
        if (tl && l.kind == L_AGEMM) {                  // (dump fields: channels, reduction length, output columns, 10 + product form)
            const I2VAttnGemm& q = l.ag;
            tl->Cd = q.Cc; tl->K = q.form == 1 ? q.Cc : (q.form == 2 ? q.N : q.M); tl->HWg = q.form == 2 ? q.M : q.N; tl->frames = frames; tl->pw = 10 + q.form;
            tl->bytes = 4.0 * clips * ((double)q.M * q.N + (double)q.Cc * q.M + (double)q.Cc * q.N);
        }
        if (tl && (l.kind == L_SE_SQUEEZE || l.kind == L_SE_EXCITE || l.kind == L_SE_SCALE)) {      // (dump fields: channels, squeezed width, positions, 20 + stage + 3 x backward)
            tl->Cd = l.se.C; tl->K = l.se.rd; tl->HWg = l.se.HW; tl->frames = frames;
            tl->pw = 20 + (l.kind == L_SE_SQUEEZE ? 0 : l.kind == L_SE_EXCITE ? 1 : 2) + 3 * l.se.backward;
            tl->bytes = l.se_bytes_per_frame * frames;
        }
        return tl;
    }
    void close() { if (seg) be_event_record(seg->stop, s); }      // the open segment ends here
};

// Launch overlap (mark_overlap): hoisted launches go to the net's side stream right after the launch they depend on was issued on the
// main stream, which waits for each of them in front of the first launch that touches its operands.
struct SideStream {
    Net& n; std::vector<Launch>& L; const std::vector<std::vector<int>>& at; i2v_stream_t main;
    int clips; const float* x; float* gx; int accumulate;
    struct Pending { int join; void* done; };
    std::vector<Pending> pending;

    void* event() {
        if (n.ov_used == n.ov_ev.size()) { void* e = be_event_create(); if (!e) return nullptr; n.ov_ev.push_back(e); }
        return n.ov_ev[n.ov_used++];
    }
    int issue(int p) {                  // the hoisted launches that follow main launch p (-1: the start of the list)
        for (int i : at[p + 1]) {
            void* ready = event(); void* done = event();
            if (!ready || !done) return fail("launch overlap: event creation failed");
            CHECK_BE(be_event_record(ready, main)); CHECK_BE(be_stream_wait_event(n.side, ready));
            Launch& m = L[i];
            const int fr = clips * m.T;
            if (fr * m.conv.Hg * m.conv.Wg != 0) {
                const int cb = m.cfg_b[cfg_bucket(clips, n.maxN / n.Tin())];
                if (cb) m.conv.cfg = cb;
                if (conv_run(m, fr, x, gx, accumulate, n.side)) return 1;
                __atomic_fetch_add(&g_overlap_launches, 1, __ATOMIC_RELAXED);
            }
            CHECK_BE(be_event_record(done, n.side));
            pending.push_back(Pending{m.ov_join, done});
        }
        return 0;
    }
    int join(int upto) {                // the main stream waits for every hoisted launch whose first dependent is at or before `upto`
        for (size_t i = 0; i < pending.size();) {
            if (pending[i].join <= upto) { CHECK_BE(be_stream_wait_event(main, pending[i].done)); pending[i] = pending.back(); pending.pop_back(); }
            else ++i;
        }
        return 0;
    }
};

}  // namespace

static int run_list(i2v_ctx* h, Net& n, std::vector<Launch>& L, int in_frames, const float* x, float* gx, int accumulate,
                    i2v_stream_t s, bool backward_pass) {
    const int clips = in_frames / n.Tin();
    const int bucket = cfg_bucket(clips, n.maxN / n.Tin());
    ListTiming timing{h, s, backward_pass};
    SideStream side{n, L, n.ov_at[backward_pass ? 1 : 0], s, clips, x, gx, accumulate};
    const bool overlap = !h->timing && n.side && !side.at.empty() && in_frames <= n.ov_max_frames;
    if (overlap) n.ov_used = 0;
    if (overlap && side.issue(-1)) return 1;
    // does launch k lead a fused group (pair or fast-pathway block) at this call's size?
    auto leads_group = [&](size_t k) { return L[k].kind == L_CONV && ((L[k].fuse_ok && L[k].fuse_b[bucket]) || (L[k].fb_ok && L[k].fb_b[bucket])); };
    int sc_from = -1; size_t sc_at = 0;                  // a deferred shortcut launch and the consumer it runs with
    for (size_t li = 0; li < L.size(); ++li) {
        Launch& l = L[li];
        const int frames = clips * l.T;                  // frames this launch iterates over
        const size_t li0 = li;
        if (overlap && l.ov_after != -2) continue;       // hoisted: already issued on the side stream
        // the shortcut of a pair (mark_fusable / autotune): passed over here, it runs inside ONE kernel with its consumer sc_ok entries on
        // -- unless a launch in between leads a fused group of its own, or launches are being hoisted to the side stream (whose issue
        // points are list positions)
        if (l.kind == L_CONV && l.sc_ok && l.sc_b[bucket] && !overlap && sc_from < 0 && li + l.sc_ok < L.size() && frames * l.conv.Hg * l.conv.Wg > 0 &&
            sc_fits(l, L[li + l.sc_ok], frames)) {
            bool clear = !leads_group(li);
            for (size_t k = li + 1; k <= li + l.sc_ok && clear; ++k) clear = !leads_group(k);
            if (clear) { sc_from = (int)li; sc_at = li + l.sc_ok; continue; }
        }
        const int sc = (sc_from >= 0 && li == sc_at) ? sc_from : -1;
        if (sc >= 0) sc_from = -1;
        // this 3x3 launch and the pointwise launch behind it as ONE kernel (mark_fusable / autotune): the next entry is skipped
        const int fuse = (l.kind == L_CONV && l.fuse_ok && li + 1 < L.size() && frames * l.conv.Hg * l.conv.Wg > 0 && fused_fits(l, L[li + 1], frames))
                             ? l.fuse_b[bucket] : 0;
        // this launch and the next fb_ok - 1 as ONE fused fast-pathway block (mark_fusable / autotune): those entries are skipped
        const int fb = (l.kind == L_CONV && l.fb_ok && li + l.fb_ok <= L.size() && frames * l.conv.Hg * l.conv.Wg > 0) ? l.fb_b[bucket] * l.fb_ok : 0;
        if (overlap && side.join((int)li + (fb ? fb - 1 : fuse ? 1 : 0))) return 1;
        TimedLaunch* const tl = h->timing ? timing.open(L, li, fb, fuse, sc, frames, clips, accumulate) : nullptr;
        struct Stop { TimedLaunch* t; i2v_stream_t s; ~Stop() { if (t) be_event_record(t->stop, s); } } stop{tl, s};
        switch (l.kind) {
            case L_CONV:
            case L_IMGGRAD: {
                if (frames * l.conv.Hg * l.conv.Wg == 0) break;
                if (sc >= 0) {      // (the consumer's tuned configuration carries the streaming-store bit the pair was timed with)
                    if (l.cfg_b[bucket]) l.conv.cfg = l.cfg_b[bucket];
                    if (sc_run(L[sc], l, frames, s)) return 1;
                    break;
                }
                if (fuse) { if (fused_run(l, L[li + 1], frames, x, fuse == 2, s)) return 1; ++li; break; }
                if (fb) {
                    const int rc = fast_run(L, li, frames, x, s);
                    if (rc == 1) return 1;
                    if (rc == 0) { li += fb - 1; break; }
                    // (rc == 2: not eligible at this frame count -- the separate launches run, this one now and the others in their turn)
                }
                const int cb = l.cfg_b[bucket];
                if (cb) l.conv.cfg = cb;
                if (conv_run(l, frames, x, gx, accumulate, s)) return 1;
            } break;
            case L_GCONV: {
#ifdef I2V_HAVE_GCONV
                I2VGConvParams p = l.gc; p.N = frames; CHECK_BE(k_gconv(p, s));
#else
                return fail("this build has no grouped-convolution kernel");
#endif
            } break;
            case L_DWCONV: {
#ifdef I2V_HAVE_DWCONV
                I2VDwConvParams p = l.dc; p.N = frames; CHECK_BE(k_dwconv(p, s));
#else
                return fail("this build has no depthwise-convolution kernel");
#endif
            } break;
#ifdef I2V_HAVE_SE
            case L_SE_SQUEEZE: { I2VSeParams p = l.se; p.N = frames; CHECK_BE(k_se_squeeze(p, s)); } break;
            case L_SE_EXCITE: { I2VSeParams p = l.se; p.N = frames; CHECK_BE(k_se_excite(p, s)); } break;
            case L_SE_SCALE: { I2VSeParams p = l.se; p.N = frames; CHECK_BE(k_se_scale(p, s)); } break;
#else               // (no such kernels in this build: the same node as scalar code on the backend's memory, which is host memory here)
            case L_SE_SQUEEZE: { I2VSeParams p = l.se; p.N = frames; if (se_host::squeeze(p)) return fail("squeeze-and-excitation: squeeze failed"); } break;
            case L_SE_EXCITE: { I2VSeParams p = l.se; p.N = frames; if (se_host::excite(p)) return fail("squeeze-and-excitation: excite failed"); } break;
            case L_SE_SCALE: { I2VSeParams p = l.se; p.N = frames; if (se_host::scale(p)) return fail("squeeze-and-excitation: scale failed"); } break;
#endif
            case L_POOLF: { I2VPoolParams p = l.pool; p.N = frames; CHECK_BE(k_pool_fwd(p, s)); } break;
            // A 1 x k x k window with temporal stride st over Ts = st*To frames is the image pooling kernel on every
            // st-th frame (frame stride * st); its backward leaves the skipped frames zero.
            case L_POOL3F: {
                I2VPoolParams p = l.pool; p.N = frames;
                if (p.kt == 1 && p.pad_t == 0 && p.Ts == p.stride_t * p.To) { p.x_nstride *= p.stride_t; CHECK_BE(k_pool_fwd(p, s)); }
                else CHECK_BE(k_pool3d_fwd(p, s));
            } break;
            case L_POOL3B: {
                I2VPoolParams p = l.pool; p.N = frames;
                if (p.kt == 1 && p.pad_t == 0 && p.Ts == p.stride_t * p.To && p.gx_nstride == (int64_t)p.C * p.Hs * p.Ws) {
                    CHECK_BE(be_memset0(p.gx, (size_t)frames * p.stride_t * p.gx_nstride * sizeof(float), s));
                    p.x_nstride *= p.stride_t; p.gx_nstride *= p.stride_t;
                    CHECK_BE(k_pool_bwd(p, s));
                } else CHECK_BE(k_pool3d_bwd(p, s));
            } break;
            case L_AVGF: { I2VPoolParams p = l.pool; p.N = frames; CHECK_BE(k_avgpool_fwd(p, s)); } break;
            case L_AVGB: { I2VPoolParams p = l.pool; p.N = frames; CHECK_BE(k_avgpool_bwd(p, s)); } break;
            case L_MEMSET:
                if (!l.ms_gx) CHECK_BE(be_memset0(l.ms_ptr, l.ms_floats_per_frame * frames * sizeof(float), s));
                else if (!accumulate) CHECK_BE(be_memset0(gx, l.ms_floats_per_frame * frames * sizeof(float), s));
                break;
            case L_POOLB: { I2VPoolParams p = l.pool; p.N = frames; CHECK_BE(k_pool_bwd(p, s)); } break;
            case L_ADDMASK: { I2VAddMaskParams p = l.am; p.N = frames; CHECK_BE(k_addmask(p, s)); } break;
            case L_AGEMM: { I2VAttnGemm p = l.ag; p.clips = clips; CHECK_BE(k_attn_gemm(p, s)); } break;
            case L_SOFTMAX: { I2VSoftmaxRows p = l.sm; p.rows = (int64_t)clips * l.sm_rows_per_clip; CHECK_BE(k_softmax_rows(p, s)); } break;
        }
        if (overlap) for (size_t p = li0; p <= li; ++p) if (side.issue((int)p)) return 1;      // (a fused group advanced li past its members)
    }
    if (overlap && side.join((int)L.size())) return 1;   // nothing of this list is still running on the side stream when the caller's next kernel starts
    timing.close();
    return 0;
}

extern "C" int i2v_net_forward(i2v_handle h, int net, const float* x, int frames, void* stream) {
    Net* n = get_net(h, net); if (!n) return 1;
    if (!n->planned) return fail("net not planned");
    if (frames <= 0 || frames > n->maxN) return fail("frames=%d outside 1..%d", frames, n->maxN);
    if (frames % n->Tin()) return fail("frames=%d is not a multiple of the input's %d frames per clip", frames, n->Tin());
    if (!x) return fail("null input");
    n->frames = frames;
    if (n->stage_input) {
        // The slack around the source is what conv_tile's quad-row staging (MODE 4) needs.  When the autotuner gave every quad-row
        // launch that reads the input the halo-tile kernel for this batch bucket (configuration bit 10: conv_stem_halo stages whole
        // windows and range-checks every piece) and the caller's frames are 16-byte aligned, nothing reads outside them and the copy --
        // 2 % of an ILAF step on SlowFast -- is skipped.
        static const bool always = [] { const char* e = getenv("I2V_STAGE_COPY"); return e && e[0] == '1'; }();      // (developer knob: A/B)
        bool need = always || ((uintptr_t)x & 15) != 0;
        const int bucket = cfg_bucket(frames / n->Tin(), n->maxN / n->Tin());
        for (const Launch& l : n->fwd)
            if (l.kind == L_CONV && l.src_is_input && l.conv.quad && !(l.cfg_b[bucket] > 0 && ((l.cfg_b[bucket] - 1) & 1024))) need = true;
        if (need) {
            const Buffer& ib = n->bufs[n->tens[n->input].buf];
            const size_t bytes = (size_t)frames * ib.C * ib.H * ib.W * sizeof(float);
            float* staged = n->arena + n->in_stage_off;
            CHECK_BE(be_d2d_2d(staged, bytes, x, bytes, bytes, 1, stream));
            x = staged;
        }
    }
    return run_list(h, *n, n->fwd, frames, x, nullptr, 0, stream, false);
}

extern "C" int i2v_net_backward(i2v_handle h, int net, float* gx, int accumulate, void* stream) {
    Net* n = get_net(h, net); if (!n) return 1;
    if (!n->planned || n->frames <= 0) return fail("backward before forward");
    if (!gx) return fail("null gradient output");
    return run_list(h, *n, n->bwd, n->frames, nullptr, gx, accumulate, stream, true);
}

extern "C" int i2v_timing_enable(i2v_handle h, int enable) {
    if (!h) return fail("null handle");
    h->timing = enable == 2 ? 2 : (enable != 0 ? 1 : 0); h->timed_used = 0;
    return 0;
}

// kinds: 0 conv_igemm forward, 1 first-layer image gradient, 2 pool fwd, 3 pool bwd, 4 addmask, 5 conv_igemm dgrad
// fields per kind: 0 ms, 1 algorithmic flops, 2 launches, 3 algorithmic bytes (convolution launches), and the same for the
// LOW-INTENSITY launches alone -- flops/byte below the machine balance 157.3 TFLOP/s / 8 TB/s = 19.7, i.e. the ones the
// HBM roofline bounds --: 4 ms, 5 bytes, 6 launches, 7 flops
#define I2V_TIMING_FIELDS 8
extern "C" int i2v_timing_collect_ex(i2v_handle h, double* out, int n_kinds, int n_fields) {
    if (!h || !out || n_kinds < 6 || n_fields < I2V_TIMING_FIELDS) return fail("i2v_timing_collect_ex: bad argument");
    for (int i = 0; i < n_kinds * n_fields; ++i) out[i] = 0.0;
    if (h->timed_used) CHECK_BE(be_device_sync());
    const char* dump_path = getenv("I2V_TIMING_DUMP");      // debug: one line per launch
    FILE* dump = dump_path ? fopen(dump_path, "a") : nullptr;
    for (size_t i = 0; i < h->timed_used; ++i) {
        const TimedLaunch& t = h->timed[i];
        float ms = 0.f;
        CHECK_BE(be_event_elapsed_ms(t.chain_from ? t.chain_from : t.start, t.stop, &ms));
        if (dump && h->timing != 2) fprintf(dump, "%d %d %d %d %d %d %.4f %.3f %.3f\n", t.kind, t.Cd, t.K, t.HWg, t.frames, t.pw, ms, t.flops * 1e-9, t.bytes * 1e-6);
        if (t.kind < 0 || t.kind >= n_kinds) continue;
        double* o = out + (size_t)t.kind * n_fields;
        o[0] += ms; o[1] += t.flops; o[2] += t.count; o[3] += t.bytes;
        if (h->timing != 2 && t.bytes > 0 && t.flops < 19.7 * t.bytes) { o[4] += ms; o[5] += t.bytes; o[6] += 1; o[7] += t.flops; }
    }
    if (dump) fclose(dump);
    h->timed_used = 0;
    return 0;
}

extern "C" int i2v_timing_collect(i2v_handle h, double* ms_by_kind, double* flops_by_kind, int64_t* launches_by_kind,
                                  int n_kinds) {
    if (!h || !ms_by_kind || !flops_by_kind || !launches_by_kind || n_kinds < 6 || n_kinds > 16) return fail("i2v_timing_collect: bad argument");
    double tmp[16 * I2V_TIMING_FIELDS];
    if (i2v_timing_collect_ex(h, tmp, n_kinds, I2V_TIMING_FIELDS)) return 1;
    for (int i = 0; i < n_kinds; ++i) {
        ms_by_kind[i] = tmp[i * I2V_TIMING_FIELDS]; flops_by_kind[i] = tmp[i * I2V_TIMING_FIELDS + 1];
        launches_by_kind[i] = (int64_t)tmp[i * I2V_TIMING_FIELDS + 2];
    }
    return 0;
}

extern "C" int i2v_net_hook_info(i2v_handle h, int net, int hook, float** act, int64_t* act_stride,
                                 float** grad, int64_t* grad_stride, int64_t* D, int32_t* post_relu) {
    Net* n = get_net(h, net); if (!n) return 1;
    if (!n->planned) return fail("net not planned");
    if (hook < 0 || hook >= (int)n->hooks.size()) return fail("bad hook index");
    int t = n->hooks[hook];
    View a = view_of(*n, t, false), g = view_of(*n, t, true);
    int64_t d = (int64_t)a.C * a.H * a.W;
    if (act) *act = a.p;
    if (act_stride) *act_stride = a.nstride;
    if (grad_stride) *grad_stride = n->hook_tmp[hook] ? d : g.nstride;
    if (grad) *grad = n->hook_tmp[hook] ? n->hook_tmp[hook] : g.p;
    if (D) *D = d;
    if (post_relu) *post_relu = n->tens[t].post_relu ? 1 : 0;
    return 0;
}

extern "C" int i2v_net_read_tensor(i2v_handle h, int net, int tensor, int which, float* out, int frames,
                                   void* stream) {
    Net* n = get_net(h, net); if (!n) return 1;
    if (!n->planned) return fail("net not planned");
    if (tensor < 0 || tensor >= (int)n->tens.size() || tensor == n->input) return fail("bad tensor id");
    View v = view_of(*n, tensor, which != 0);
    if (frames <= 0 || frames > n->maxN / n->Tin() * v.T) return fail("bad frame count");
    // What a fused group never stores (Net::unstored, recorded once by the plan) cannot be read back: the arena holds stale contents
    // there.  A forward shortcut that runs inside a pair is produced on demand instead -- the launch itself, from its source as the
    // forward pass left it: exactly the values the separate launch stores -- because callers read whole networks back activation by
    // activation; a gradient view, a backward pair and a shortcut into scratch that is reused are refused like the others.
    static const char* const never_stored[3] = {
        "i2v_net_read_tensor: this tensor is the intermediate of a fused 3x3 -> pointwise pair and is never stored "
        "(plan without I2V_FUSE / I2V_FORCE_FUSE to read it)",
        "i2v_net_read_tensor: this tensor is an intermediate of a fused fast-pathway block and is never stored "
        "(plan with I2V_FASTBLOCK=0 to read it)",
        "i2v_net_read_tensor: this tensor is the shortcut output of a fused first bottleneck (shortcut pair) and is never stored "
        "(plan with I2V_SCPAIR=0 to read it)"};
    const Range want = extent(v.p, frames, 4 * v.nstride, 4ll * v.C * v.H * v.W);
    for (const Unstored& u : n->unstored) {
        if (!meets(u.bytes, want)) continue;
        if (u.remake < 0 || which != 0) return fail("%s", never_stored[u.group]);
        const Launch& l = n->fwd[u.remake];
        if (conv_run(l, frames / std::max(1, v.T) * l.T, nullptr, nullptr, 0, stream)) return 1;
    }
    size_t row = (size_t)v.C * v.H * v.W * sizeof(float);
    CHECK_BE(be_d2d_2d(out, row, v.p, (size_t)v.nstride * sizeof(float), row, frames, stream));
    return 0;
}
