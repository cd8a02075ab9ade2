// Plan-time decisions over the finished launch lists: what may run fused, what may run on the side stream, which tile runs.
#include "i2v_net.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>

namespace eng {

// The shared analysis: every pass below that merges launches, moves one past another or runs one beside its neighbours asks the same
// question of memory, and access_of is the ONE place that lists the operands of each Kind -- data operands, 1-bit gate rows, arg-max
// bytes, an SE node's vectors -- with the launch's OWN frame count at the planned clip count; the caller's gradient tensor, whose
// address no plan knows, is one opaque range.  A new Kind is taught to this function and to nothing else.
Range conv_dst(const Launch& l, int64_t clips) {
    const I2VConvParams& q = l.conv;
    return extent(q.dst, clips * std::max(1, q.To), 4 * q.dst_nstride, 4ll * (q.blk > 1 ? q.Cd / (q.blk * q.blk) : q.Cd) * q.Ho * q.Wo);
}
Access access_of(const Launch& c, int64_t clips) {
    static const char gx_tag[16] = {0};          // stands for the caller's gradient tensor (every launch that touches it conflicts with every other)
    const Range GX(gx_tag, gx_tag + 16);
    Access o;
    auto rd = [&](const Range& x) { if (x.first) o.r.push_back(x); };
    auto wr = [&](const Range& x) { if (x.first) o.w.push_back(x); };
    if (c.kind == L_CONV || c.kind == L_IMGGRAD || c.kind == L_GCONV || c.kind == L_DWCONV) {
        const I2VConvParams& q = c.conv;
        const int64_t fs = clips * std::max(1, q.Ts), fo = clips * std::max(1, q.To);
        const int64_t dplane = 4ll * (q.blk > 1 ? q.Cd / (q.blk * q.blk) : q.Cd) * q.Ho * q.Wo;
        if (!c.src_is_input) rd(extent(q.src, fs, 4 * q.src_nstride, 4ll * q.Cs * q.Hs * q.Ws));
        rd(extent(q.add0, fo, 4 * q.add0_nstride, dplane)); rd(extent(q.add1, fo, 4 * q.add1_nstride, dplane)); rd(extent(q.mask, fo, 4 * q.mask_nstride, dplane));
        rd(extent(q.gate, 1, 0, 4ll * q.Cd * q.gate_stride)); wr(extent(q.gate_out, 1, 0, 4ll * q.Cd * q.gate_out_stride));
        if (c.kind == L_IMGGRAD) { wr(GX); rd(GX); } else wr(conv_dst(c, clips));
    } else if (c.kind == L_ADDMASK) {
        const int64_t fr = clips * std::max(1, c.T), pl = 4ll * c.am.C * c.am.HW;
        wr(extent(c.am.out, fr, 4 * c.am.out_nstride, pl));
        for (int i = 0; i < 3; ++i) rd(extent(c.am.a[i], fr, 4 * c.am.a_nstride[i], pl));
        rd(extent(c.am.mask, fr, 4 * c.am.mask_nstride, pl)); rd(extent(c.am.gate, 1, 0, 4ll * c.am.C * c.am.gate_stride));
    } else if (c.kind == L_MEMSET) {
        if (c.ms_gx) wr(GX); else wr(extent(c.ms_ptr, 1, 0, 4ll * (int64_t)c.ms_floats_per_frame * clips * std::max(1, c.T)));
    } else if (c.kind == L_AGEMM || c.kind == L_SOFTMAX) {
        o.barrier = true;
    } else if (c.kind == L_SE_SQUEEZE || c.kind == L_SE_EXCITE || c.kind == L_SE_SCALE) {
        const I2VSeParams& q = c.se;
        const int64_t fr = clips * std::max(1, c.T), pl = 4ll * q.C * q.HW;
        const Range vec = extent(c.se_vec, 1, 0, 4ll * (int64_t)c.se_vec_floats);     // (the node's vectors: read and written by its launches only)
        rd(vec); wr(vec);
        if (c.kind != L_SE_EXCITE) { rd(extent(q.x, fr, 4 * q.x_nstride, pl)); rd(extent(q.g, fr, 4 * q.g_nstride, pl)); }
        if (c.kind == L_SE_SCALE) {
            rd(extent(q.r, fr, 4 * q.r_nstride, pl)); wr(extent(q.dst, fr, 4 * q.dst_nstride, pl));
            wr(extent(q.gate_out, 1, 0, 4ll * q.C * q.gate_out_stride));
        }
    } else {
        const I2VPoolParams& q = c.pool;
        const int64_t fr = clips * std::max(std::max(1, c.T), std::max(q.Ts, q.To)), pin = 4ll * q.C * q.Hs * q.Ws, pout = 4ll * q.C * q.Ho * q.Wo;
        const Range idx = extent(q.idx, 1, 0, fr * (int64_t)q.C * q.Ho * q.Wo);
        const bool fwd = c.kind == L_POOLF || c.kind == L_POOL3F || c.kind == L_AVGF;
        if (fwd) { rd(extent(q.x, fr, 4 * q.x_nstride, pin)); wr(extent(q.y, fr, 4 * q.y_nstride, pout)); wr(idx); }
        else { rd(extent(q.x, fr, 4 * q.x_nstride, pin)); rd(extent(q.y, fr, 4 * q.y_nstride, pout)); rd(extent(q.yact, fr, 4 * q.yact_nstride, pout)); rd(idx);
               wr(extent(q.gx, fr * std::max(1, q.stride_t), 4 * q.gx_nstride, pin)); }
    }
    return o;
}
static std::vector<Access> access_of(const std::vector<Launch>& L, int64_t clips) {
    std::vector<Access> acc; acc.reserve(L.size());
    for (const Launch& l : L) acc.push_back(access_of(l, clips));
    return acc;
}

// Groups that run as ONE kernel and never store what passes between their members: fused pairs, fused fast-pathway blocks, shortcut
// pairs.  A group qualifies only if NOTHING else looks at that memory: no other launch of either list (which also rules out
// I2V_GATES=0, whose backward pass reads fp32 activations, and the in-place ReLU gain of i2v_net_set_relu_gain), no hook, and not
// the network input.  Conservative: any overlap of address ranges counts.  The access sets of both lists are computed once, up here,
// and follow the launches where a pass swaps two (only where conflict() says that neither sees what the other writes).
// Fused pairs (k_conv_fused): launch i a 3x3 convolution, launch i + 1 the pointwise convolution that reads its output -- a
// bottleneck's conv2 -> conv3 in the forward list, the input gradients of conv2 -> conv1 in the backward list.
void mark_fusable(Net& n) {
    const int64_t frames = n.maxN, clips = n.maxN / n.Tin();
    std::vector<Launch>* const lists[2] = {&n.fwd, &n.bwd};
    std::vector<Access> acc[2] = {access_of(n.fwd, clips), access_of(n.bwd, clips)};
    std::vector<Range> hooked;
    for (size_t h = 0; h < n.hooks.size(); ++h) {
        View a = view_of(n, n.hooks[h], false), g = view_of(n, n.hooks[h], true);
        hooked.push_back(extent(a.p, frames, 4 * a.nstride, 4ll * a.C * a.H * a.W));
        hooked.push_back(extent(g.p, frames, 4 * g.nstride, 4ll * g.C * g.H * g.W));
    }
    auto hook_on = [&](const Range& w) { for (const Range& hk : hooked) if (meets(hk, w)) return true; return false; };
    // does a launch of either list, other than launches first .. last of list k, read or write `w`?
    auto others_touch = [&](int k, size_t first, size_t last, const Range& w) {
        for (int m = 0; m < 2; ++m)
            for (size_t j = 0; j < acc[m].size(); ++j)
                if (!(m == k && j >= first && j <= last) && (reads(acc[m][j], w) || writes(acc[m][j], w))) return true;
        return false;
    };
    auto swap_launches = [&](int k, size_t i, size_t j) { std::swap((*lists[k])[i], (*lists[k])[j]); std::swap(acc[k][i], acc[k][j]); };
    // A first bottleneck runs its shortcut convolution between conv2 and conv3 (conv3 adds it): where that launch and the 3x3 are
    // independent of each other, they swap places so that the pair becomes adjacent.
    for (int k = 0; k < 2; ++k)
        for (size_t i = 0; i + 2 < lists[k]->size(); ++i) {
            const Launch& a = (*lists[k])[i]; const Launch& c = (*lists[k])[i + 1]; const Launch& b = (*lists[k])[i + 2];
            if (a.kind != L_CONV || c.kind != L_CONV || b.kind != L_CONV || a.src_is_input || c.src_is_input || !k_conv_fusable(a.conv, b.conv)) continue;
            if (k_conv_fusable(a.conv, c.conv)) continue;
            if (!conflict(acc[k][i], acc[k][i + 1])) swap_launches(k, i, i + 1);
        }
    for (int k = 0; k < 2; ++k)
        for (size_t i = 0; i + 1 < lists[k]->size(); ++i) {
            Launch& a = (*lists[k])[i]; const Launch& b = (*lists[k])[i + 1];
            a.fuse_ok = 0;
            if (a.kind != L_CONV || b.kind != L_CONV || a.src_is_input || b.src_is_input || a.T != b.T) continue;
            const int ok = k_conv_fusable(a.conv, b.conv);
            if (!ok) continue;
            // the intermediate: a writes it and b reads it as its source -- and neither may see it through any other operand
            const Range w = conv_dst(a, clips);
            const bool other = hook_on(w) || others_touch(k, i, i + 1, w) || reads(acc[k][i], w) || reads(acc[k][i + 1], w) > 1 || writes(acc[k][i + 1], w);
            if (!other) a.fuse_ok = ok;
            if (getenv("I2V_FUSE_DEBUG"))
                fprintf(stderr, "[i2v fuse] %s pair %zu: 3x3 Cd=%d K=%d %dx%d -> 1x1 Cd=%d K=%d: eligible=%d other_reader=%d\n", k ? "bwd" : "fwd", i,
                        a.conv.Cd, a.conv.K, a.conv.Hg, a.conv.Wg, b.conv.Cd, b.conv.K, ok, (int)other);
        }
    // ---- fused fast-pathway blocks (k_fastblock): groups of consecutive launches, found from the graph nodes behind them ----
    {
        const bool fb_off = [] { const char* e = getenv("I2V_FASTBLOCK"); return e && e[0] == '0'; }();      // (read per plan)
        auto cd_of = [&](const Launch& l) -> const i2v_conv3d_desc* { return (l.kind == L_CONV && l.node >= 0 && n.nodes[l.node].type == 0 && !n.nodes[l.node].preact()) ? &n.nodes[l.node].cd : nullptr; };
        auto unit = [](const i2v_conv3d_desc& c) { return c.stride == 1 && c.stride_t == 1 && c.dil_t == 1; };
        auto is_pw = [&](const i2v_conv3d_desc& c) { return unit(c) && c.kt == 1 && c.kh == 1 && c.kw == 1 && c.pad == 0 && c.pad_t == 0; };
        auto is_t = [&](const i2v_conv3d_desc& c) { return unit(c) && c.kh == 1 && c.kw == 1 && c.pad == 0 && (c.kt & 1) && 2 * c.pad_t == c.kt - 1; };      // k x 1 x 1, "same"
        auto is_33 = [&](const i2v_conv3d_desc& c) { return unit(c) && c.kt == 1 && c.kh == 3 && c.kw == 3 && c.pad == 1 && c.pad_t == 0; };
        // nothing but the group's own launches may touch an intermediate, and it must not be hooked
        auto private_to = [&](int k, size_t first, size_t last, const Launch& w) {
            const Range r = conv_dst(w, clips);
            return !hook_on(r) && !others_touch(k, first, last, r);
        };
        for (Launch& l : n.fwd) l.fb_ok = 0;
        for (Launch& l : n.bwd) l.fb_ok = 0;
        // backward: [conv3's input gradient, X, conv2's input gradient] with X independent of both (a first block's projection-shortcut
        // gradient sits between them): X moves in front
        for (size_t i = 0; !fb_off && i + 2 < n.bwd.size(); ++i) {
            const Launch& a = n.bwd[i]; const Launch& x = n.bwd[i + 1]; const Launch& b = n.bwd[i + 2];
            const i2v_conv3d_desc* ca = cd_of(a); const i2v_conv3d_desc* cb = cd_of(b);
            if (!ca || !cb || !is_pw(*ca) || !is_33(*cb) || b.conv.src != a.conv.dst || x.kind != L_CONV) continue;
            if (!conflict(acc[1][i + 1], acc[1][i]) && !conflict(acc[1][i + 1], acc[1][i + 2])) swap_launches(1, i, i + 1);
        }
        for (size_t i = 0; !fb_off && i + 1 < n.bwd.size(); ++i) {
            Launch& a = n.bwd[i]; Launch& b = n.bwd[i + 1];
            const i2v_conv3d_desc* ca = cd_of(a); const i2v_conv3d_desc* cb = cd_of(b);
            if (!ca || !cb || !is_pw(*ca) || !is_33(*cb) || a.T != b.T || b.conv.src != a.conv.dst) continue;
            if (i2v_fastblock_rows(a.conv, b.conv, nullptr, nullptr) <= 0) continue;
            if (!private_to(1, i, i + 1, a)) continue;
            a.fb_ok = 2;
        }
        for (size_t i = 0; !fb_off && i + 2 < n.fwd.size(); ++i) {
            Launch& a = n.fwd[i]; Launch& b = n.fwd[i + 1];
            const i2v_conv3d_desc* ca = cd_of(a); const i2v_conv3d_desc* cb = cd_of(b);
            if (!ca || !cb || a.src_is_input || !(is_t(*ca) || is_pw(*ca)) || !is_33(*cb) || !ca->relu || !cb->relu || ca->residual >= 0 || cb->residual >= 0 || cb->src != ca->dst) continue;
            Launch& c3 = n.fwd[i + 2];
            const i2v_conv3d_desc* cc = cd_of(c3);
            if (!cc || !is_pw(*cc)) continue;
            if (cc->src == cb->dst && cc->residual >= 0 && cc->relu && a.T == b.T && a.T == c3.T) {               // identity shortcut
                if (i2v_fastblock_rows(a.conv, b.conv, &c3.conv, nullptr) <= 0) continue;
                if (!private_to(0, i, i + 2, a) || !private_to(0, i, i + 2, b)) continue;
                a.fb_ok = 3;
            } else if (i + 3 < n.fwd.size() && cc->src == ca->src && !cc->relu && cc->residual < 0) {             // projection shortcut, then conv3
                Launch& c4 = n.fwd[i + 3];
                const i2v_conv3d_desc* c4d = cd_of(c4);
                if (!c4d || !is_pw(*c4d) || c4d->src != cb->dst || c4d->residual != cc->dst || !c4d->relu || a.T != b.T || a.T != c3.T || a.T != c4.T) continue;
                if (i2v_fastblock_rows(a.conv, b.conv, &c4.conv, &c3.conv) <= 0) continue;
                if (!private_to(0, i, i + 3, a) || !private_to(0, i, i + 3, b) || !private_to(0, i, i + 3, c3)) continue;
                a.fb_ok = 4;
            }
        }
        // without the autotuner (I2V_AUTOTUNE=0: tests, tools, the host simulation) a group is fused only on request
        const bool fb_force = [] { const char* e = getenv("I2V_FORCE_FASTBLOCK"); return e && e[0] == '1'; }();      // (read per plan: tests compare both)
        for (std::vector<Launch>* L : lists)
            for (Launch& a : *L)
                for (int bk = 0; bk < 4; ++bk) a.fb_b[bk] = (a.fb_ok && fb_force) ? 1 : 0;
        if (getenv("I2V_FUSE_DEBUG"))
            for (std::vector<Launch>* L : lists)
                for (size_t i = 0; i < L->size(); ++i)
                    if ((*L)[i].fb_ok) fprintf(stderr, "[i2v fastblock] %s launch %zu: group of %d (Cs %d -> %d mid channels, %dx%d)\n", L == &n.fwd ? "fwd" : "bwd", i, (*L)[i].fb_ok,
                                               (*L)[i].conv.Cs, (*L)[i].conv.Cd, (*L)[i].conv.Hg, (*L)[i].conv.Wg);
    }
    // ---- shortcut pairs (k_conv_scpair): a 1x1 launch whose output is nothing but the plain addend of a pointwise launch further down ----
    // Forward, a first bottleneck's projection shortcut under its expand convolution; backward, wherever one input gradient is only the
    // next one's addend on the same grid (the stride-1 first bottleneck: the shortcut's input gradient under conv1's).  The pair never
    // stores the intermediate, so nothing -- launch of either list, hook, in-place gain -- may look at that memory while the two launches
    // would have kept a's output in it (spelled out below).  The shortcut need not be adjacent to its consumer: the executor runs it in the consumer's place, which is the same
    // schedule with the shortcut moved down -- admitted only if it does not conflict with any launch it passes (the test of the swaps above).
    {
        const bool sc_off = [] { const char* e = getenv("I2V_SCPAIR"); return e && e[0] == '0'; }();      // (read per plan: tests and A/B runs compare both)
        for (int k = 0; k < 2; ++k) {
            std::vector<Launch>& L = *lists[k];
            const std::vector<Access>& A = acc[k];
            for (Launch& l : L) { l.sc_ok = 0; l.sc_private = false; for (int bk = 0; bk < 4; ++bk) l.sc_b[bk] = 0; }
            for (size_t i = 0; !sc_off && i + 1 < L.size(); ++i) {
                Launch& a = L[i];
                if (a.kind != L_CONV || a.src_is_input || a.conv.add0 || a.conv.relu) continue;
                for (size_t j = i + 1; j < L.size() && j <= i + 3; ++j) {
                    const Launch& b = L[j];
                    if (b.kind != L_CONV || b.conv.add0 != a.conv.dst) continue;
                    if (!sc_pair_ok(a, b)) break;
                    const Range w = conv_dst(a, clips);
                    // The pair differs from the two launches in what `w` holds from a's place in the list on, until something overwrites
                    // it: nothing may look at it there.  Not the launches passed; not b through a second operand; after b, in list order,
                    // no launch may read it before one has overwritten all of it (b itself, where an input gradient adds IN PLACE; the
                    // next user of a scratch view) -- and while it is live no hook and no launch of the other list may touch it at all.
                    bool other = reads(A[j], w) > 1, dead = covers(A[j], w);
                    for (size_t m = i + 1; m < j && !other; ++m) other = reads(A[m], w) || writes(A[m], w);
                    for (size_t m = j + 1; m < L.size() && !other && !dead; ++m) {
                        if (reads(A[m], w)) other = true;
                        else if (covers(A[m], w)) dead = true;
                        else other = writes(A[m], w);
                    }
                    if (!dead) {
                        other = other || hook_on(w);
                        for (const Access& c : acc[1 - k]) other = other || reads(c, w) || writes(c, w);
                    }
                    // ... and the launches it passes are convolutions on planned views that it does not conflict with.  This is conflict()
                    // less ONE term: a passed launch that reads `w` is an other_reader (above) and not a dependent, the split that the
                    // recorded decisions (tests/golden/plan_trace.txt) have always reported; the pair is refused either way.
                    bool dep = false;
                    for (size_t m = i + 1; m < j && !dep; ++m) {
                        dep = (L[m].kind != L_CONV && L[m].kind != L_GCONV && L[m].kind != L_DWCONV) || L[m].src_is_input;
                        for (const Range& x : A[m].w) dep = dep || reads(A[i], x) || writes(A[i], x);
                        for (const Range& x : A[i].w) dep = dep || (x != w && reads(A[m], x));
                    }
                    if (!other && !dep) { a.sc_ok = (int)(j - i); a.sc_private = !dead; for (int bk = 0; bk < 4; ++bk) a.sc_b[bk] = 1; }
                    if (getenv("I2V_FUSE_DEBUG"))
                        fprintf(stderr, "[i2v scpair] %s launches %zu + %zu (K %d + %d -> Cd %d, %dx%d): other_reader=%d dependent=%d\n", k ? "bwd" : "fwd", i, j,
                                a.conv.K, b.conv.K, b.conv.Cd, b.conv.Hg, b.conv.Wg, (int)other, (int)dep);
                    break;
                }
            }
        }
    }
    // without the autotuner (I2V_AUTOTUNE=0: tests, tools) a pair is fused only on request: I2V_FORCE_FUSE = 1 (plain) / 2 (halo where it applies)
    const char* force = getenv("I2V_FORCE_FUSE");
    const int f = force ? atoi(force) : 0;
    for (std::vector<Launch>* L : lists)
        for (Launch& a : *L)
            for (int b = 0; b < 4; ++b) a.fuse_b[b] = (a.fuse_ok && f) ? ((f == 2 && (a.fuse_ok & 2)) ? 2 : 1) : 0;
}

// What the plan leaves UNSTORED, once, for i2v_net_read_tensor: the intermediate of a pair that runs fused in any batch bucket, every
// member's output but the last of a fast-pathway block that does, and the output of a shortcut that runs inside a pair unless its
// consumer adds in place (then the view holds the consumer's result).  In this order: a read-back names the first grouping that applies.
void record_unstored(Net& n) {
    n.unstored.clear();
    const int64_t clips = n.maxN / n.Tin();
    auto any = [](const int b[4]) { return (b[0] | b[1] | b[2] | b[3]) != 0; };
    for (int group = 0; group < 3; ++group)
        for (const std::vector<Launch>* L : {&n.fwd, &n.bwd})
            for (size_t i = 0; i < L->size(); ++i) {
                const Launch& l = (*L)[i];
                if (l.kind != L_CONV) continue;
                if (group == 0 && l.fuse_ok && any(l.fuse_b)) n.unstored.push_back({conv_dst(l, clips), 0, -1});
                if (group == 1 && l.fb_ok && any(l.fb_b))
                    for (int j = 0; j + 1 < l.fb_ok && i + j < L->size(); ++j) n.unstored.push_back({conv_dst((*L)[i + j], clips), 1, -1});
                // a forward shortcut whose view nothing else ever touches can be produced on demand: the launch itself, from its source
                if (group == 2 && l.sc_ok && any(l.sc_b) && (*L)[i + l.sc_ok].conv.dst != l.conv.dst)
                    n.unstored.push_back({conv_dst(l, clips), 2, (L == &n.fwd && l.sc_private) ? (int)i : -1});
            }
}

// Launch overlap (round 6): a single 32-frame clip leaves the 14 x 14 layers with 1.5 tiles per CU, and a launch
// list is a chain -- except where a block has a projection shortcut: forward, the shortcut convolution depends on the block's input
// only (conv3 adds its result); backward, its input gradient depends on the gradient of the block's output only (conv1's input
// gradient adds it).  Such a launch is HOISTED: issued on the net's side stream as soon as the launch it depends on has been issued
// on the main stream, joined (event wait on the main stream) in front of the first launch that touches its operands.  Which launches
// qualify is decided by conflict() on the access sets of a list (access_of above: ranges at the planned frame count, any overlap
// counts, the caller's gradient tensor one opaque range, attention launches barriers).  No launch changes, so every result stays bit-identical; the host simulation, which executes
// launches synchronously in ISSUE order, really runs a hoisted launch early and so tests the analysis (tests/test_planner_hostsim.py).
// MEASURED AND NOT TAKEN (tools/overlap_probe.py, profiles/r6_overlap_probe.txt): one 32-frame clip 610 -> 589 frames/s (-3.4 %), four
// clips 761 -> 755 -- every hoisted launch costs two event records and two cross-queue waits, and a queue that waits on another
// queue's signal resumes tens of microseconds late, more than the idle tail it was meant to fill.  OFF by default; active only for
// calls of at most $I2V_OVERLAP_MAX_FRAMES frames (the tests set it) and never while launches are being timed.
void mark_overlap(Net& n) {
    for (int k = 0; k < 2; ++k) n.ov_at[k].clear();
    for (std::vector<Launch>* L : {&n.fwd, &n.bwd}) for (Launch& l : *L) { l.ov_after = -2; l.ov_join = -1; }
    const char* e = getenv("I2V_OVERLAP_MAX_FRAMES");
    n.ov_max_frames = e ? atoi(e) : 0;
    if (n.ov_max_frames <= 0) return;
    int k = 0;
    for (std::vector<Launch>* L : {&n.fwd, &n.bwd}) {
        const int M = (int)L->size();
        const std::vector<Access> rw = access_of(*L, n.maxN / n.Tin());
        std::vector<char> member(M, 0);          // part of a group that may run as ONE kernel (fused pair, fused fast-pathway block): stays in place
        for (int i = 0; i < M; ++i) {
            const Launch& l = (*L)[i];
            for (int j = 0; j < l.fb_ok && i + j < M; ++j) member[i + j] = 1;
            if (l.fuse_ok) { member[i] = 1; if (i + 1 < M) member[i + 1] = 1; }
        }
        n.ov_at[k].assign(M + 1, {});
        int hoisted = 0;
        for (int i = 1; i < M; ++i) {
            Launch& l = (*L)[i];
            if (l.kind != L_CONV || member[i] || l.src_is_input) continue;
            int dep = -1;
            for (int j = i - 1; j >= 0; --j) if (conflict(rw[i], rw[j])) { dep = j; break; }
            if (dep >= i - 1) continue;                                   // depends on its predecessor: nothing to overlap with
            if (dep >= 0 && (*L)[dep].ov_after != -2) continue;            // depends on a hoisted launch: stays on the main stream (which joins in front of it)
            int join = M;
            for (int j = i + 1; j < M; ++j) if (conflict(rw[j], rw[i])) { join = j; break; }
            l.ov_after = dep; l.ov_join = join;
            n.ov_at[k][dep + 1].push_back(i);
            ++hoisted;
            if (getenv("I2V_FUSE_DEBUG"))
                fprintf(stderr, "[i2v overlap] %s launch %d (Cd %d, K %d, %dx%d): side stream after launch %d, joined before launch %d of %d\n", k ? "bwd" : "fwd", i,
                        l.conv.Cd, l.conv.K, l.conv.Hg, l.conv.Wg, dep, join, M);
        }
        if (!hoisted) n.ov_at[k].clear();
        ++k;
    }
    if (n.ov_at[0].empty() && n.ov_at[1].empty()) return;
    n.side = be_stream_create();
    if (!n.side) { n.ov_at[0].clear(); n.ov_at[1].clear(); }
}

namespace {

// What a tuning pass needs to run and time launches of the net outside a forward / backward call: stand-ins for the caller's x and gx,
// and one event pair.
struct Probe {
    float* scratch = nullptr; void* e0 = nullptr; void* e1 = nullptr;
    const float* x = nullptr; float* gx = nullptr;

    int init(Net& n) {
        const Buffer& ib = n.bufs[n.tens[n.input].buf];
        const size_t img = (size_t)n.maxN * ib.C * ib.H * ib.W;
        scratch = (float*)be_malloc(2 * img * sizeof(float));
        if (!scratch) return fail("autotune scratch allocation failed");
        CHECK_BE(be_memset0(scratch, 2 * img * sizeof(float), nullptr));
        e0 = be_event_create(); e1 = be_event_create();
        x = n.stage_input ? n.arena + n.in_stage_off : scratch;      // quad-row stems need slack around their source
        gx = scratch + img;
        return 0;
    }
    ~Probe() { if (e0) be_event_destroy(e0); if (e1) be_event_destroy(e1); if (scratch) be_free(scratch); }

    // `fn` once as a warm-up (unless the caller has just run it), then `reps` times between the two events.  (Timing short launches
    // until a millisecond had passed -- up to 16 repetitions -- tripled the plan time, 2.0 -> 7.1 s for the bench's three plans, and
    // moved neither the headline nor the single-clip figure beyond box-to-box noise: not kept.)
    template <class F>
    int time(F&& fn, int reps, float* ms_per_run, bool warm_up = true) {
        if (warm_up && fn()) return 1;
        be_event_record(e0, nullptr);
        for (int r = 0; r < reps; ++r) if (fn()) return 1;
        be_event_record(e1, nullptr);
        if (be_stream_sync(nullptr)) return 1;
        float ms = 0.f; be_event_elapsed_ms(e0, e1, &ms);
        *ms_per_run = ms / reps;
        return 0;
    }
};

// One tuning per batch bucket (the planned size, half, a quarter, an eighth of its clips): a configuration that wins at 128
// frames (fewer, larger tiles) loses up to 10 % at 32, where the launch no longer fills the chip -- a caller that plans once for
// its largest group (image_main.py --group_clips, bench.py's single_clip phase) runs every group size on its own choice.
// fn(bucket, grid frames of a launch with Tg grid frames per clip at the bucket's size), bucket 0 -- the planned size -- last; a bucket
// of no clips, or of as many as the next larger one, is skipped.  Stops at the first nonzero answer and returns it.
template <class F>
int for_each_bucket(int max_clips, int Tg, F&& fn) {
    for (int b = 3; b >= 0; --b) {
        const int clips_b = max_clips >> b;
        if (clips_b < 1 || (b > 0 && clips_b == (max_clips >> (b - 1)))) continue;
        if (const int rc = fn(b, clips_b * Tg)) return rc;
    }
    return 0;
}

const char* list_name(const Net& n, const std::vector<Launch>* L) { return L == &n.fwd ? "fwd" : "bwd"; }

// Every convolution launch of both passes with each valid tile configuration on the planned shapes; the fastest is pinned.
int tune_tiles(Net& n, Probe& pr, int max_clips) {
    for (std::vector<Launch>* L : {&n.fwd, &n.bwd})
        for (Launch& l : *L) {
            if (l.kind != L_CONV && l.kind != L_IMGGRAD) continue;
            const int planned_cfg = l.conv.cfg;
            // (the stem gradients -- one to three launches per net, their candidates 5-15 % apart -- are timed over four launches: with two,
            //  alternated runs of one build disagreed about the I3D stem's kernel, an 8 % difference on 18 % of an ILAF step)
            const int reps = l.kind == L_IMGGRAD ? 4 : 2;
            const int rc = for_each_bucket(max_clips, l.conv.Tg, [&](int b, int lf) -> int {
                if (lf * l.conv.Hg * l.conv.Wg == 0) return 0;
                int cand[16]; I2VConvParams probe = l.conv; probe.N = lf;
                probe.temporal = conv_prep(l, pr.x, pr.gx, 0).temporal;      // (the frame-map half of `temporal` is derived at run time: candidates must see what the launch will be)
                const int nc = k_conv_candidates(probe, cand);
                if (nc <= 1) { if (nc == 1) l.cfg_b[b] = cand[0] + 1; return 0; }
                auto time_cfg = [&](int cfg_plus_1, float* per_launch) {
                    l.conv.cfg = cfg_plus_1;
                    return pr.time([&] { return conv_run(l, lf, pr.x, pr.gx, 0, nullptr); }, reps, per_launch);
                };
                float best = 1e30f; int best_c = -1;
                for (int ci = 0; ci < nc; ++ci) {
                    float ms = 0.f;
                    if (time_cfg(cand[ci] + 1, &ms)) return 1;
                    if ((cand[ci] & 2048) && getenv("I2V_FUSE_DEBUG"))
                        fprintf(stderr, "[i2v vfma] %s launch Cd %d K %d (%dx%d) at %d frames: conv_vfma %.1f us, best tile so far %.1f us\n", list_name(n, L),
                                l.conv.Cd, l.conv.K, l.conv.Hg, l.conv.Wg, lf, 1e3f * ms, 1e3f * best);
                    if (ms < best) { best = ms; best_c = cand[ci]; }
                }
                // second stage: the winner with streaming (non-temporal) epilogue stores, bit 7 -- one more timing per launch
                // instead of doubling the candidate list (only the dense vector epilogue has them; elsewhere the bit is inert)
                static const bool no_nt = [] { const char* e = getenv("I2V_NT"); return e && e[0] == '0'; }();
                if (best_c >= 0 && l.kind == L_CONV && !no_nt) {
                    float ms = 0.f;
                    if (time_cfg((best_c | 128) + 1, &ms)) return 1;
                    if (ms < 0.98f * best) { best = ms; best_c |= 128; }
                }
                l.cfg_b[b] = best_c >= 0 ? best_c + 1 : 0;
                return 0;
            });
            l.conv.cfg = l.cfg_b[0] ? l.cfg_b[0] : planned_cfg;      // (bucket 0 came last: conv.cfg ends as the planned size's choice)
            if (rc) return 1;
        }
    return 0;
}

// Fused fast-pathway blocks, per batch bucket: the group's launches on their tuned tiles against the group as one kernel; taken when
// at least 3 % faster (three timed runs each after a warm-up).
int tune_fastblocks(Net& n, Probe& pr, int max_clips) {
    const bool fb_force = [] { const char* e = getenv("I2V_FORCE_FASTBLOCK"); return e && e[0] == '1'; }();      // (read per plan: tests compare both)
    for (std::vector<Launch>* L : {&n.fwd, &n.bwd})
        for (size_t i = 0; i < L->size(); ++i) {
            Launch& a = (*L)[i];
            if (!a.fb_ok || i + a.fb_ok > L->size()) continue;
            for (int bk = 0; bk < 4; ++bk) a.fb_b[bk] = 0;
            const int rc = for_each_bucket(max_clips, a.conv.Tg, [&](int bk, int lf) -> int {
                auto run_sep = [&]() { for (int j = 0; j < a.fb_ok; ++j) { Launch& m = (*L)[i + j]; if (m.cfg_b[bk]) m.conv.cfg = m.cfg_b[bk]; if (conv_run(m, lf, pr.x, pr.gx, 0, nullptr)) return 1; } return 0; };
                auto run_fb = [&]() { return fast_run(*L, i, lf, pr.x, nullptr); };
                float t_sep = 0.f, t_fb = 0.f;
                if (run_fb() != 0) return 0;                       // not eligible at this size (or it failed: the separate launches stay)
                if (pr.time(run_sep, 3, &t_sep) || pr.time(run_fb, 3, &t_fb)) return 1;
                a.fb_b[bk] = (fb_force || t_fb < 0.97f * t_sep) ? 1 : 0;
                if (getenv("I2V_FUSE_DEBUG"))
                    fprintf(stderr, "[i2v fastblock] %s group %zu (%d launches, %d -> %d mid channels) at %d frames: separate %.1f us, fused %.1f us -> %s\n",
                            list_name(n, L), i, a.fb_ok, a.conv.Cs, a.conv.Cd, lf, 1e3f * t_sep, 1e3f * t_fb, a.fb_b[bk] ? "fused" : "separate");
                return 0;
            });
            for (int j = 0; j < a.fb_ok; ++j) { Launch& m = (*L)[i + j]; m.conv.cfg = m.cfg_b[0] ? m.cfg_b[0] : m.conv.cfg; }
            if (rc) return 1;
        }
    return 0;
}

// Fused pairs, per batch bucket: the two launches on their tuned tiles against the pair as one kernel (plain / halo staging), two timed
// runs each.
int tune_pairs(Net& n, Probe& pr, int max_clips) {
    for (std::vector<Launch>* L : {&n.fwd, &n.bwd})
        for (size_t i = 0; i + 1 < L->size(); ++i) {
            Launch& a = (*L)[i]; Launch& b = (*L)[i + 1];
            if (!a.fuse_ok) continue;
            for (int bk = 0; bk < 4; ++bk) a.fuse_b[bk] = 0;
            const int rc = for_each_bucket(max_clips, a.conv.Tg, [&](int bk, int lf) -> int {
                if (!fused_fits(a, b, lf)) return 0;
                const int ca = a.conv.cfg, cb = b.conv.cfg;
                if (a.cfg_b[bk]) a.conv.cfg = a.cfg_b[bk];
                if (b.cfg_b[bk]) b.conv.cfg = b.cfg_b[bk];
                float best = 1e30f; int best_v = 0, rc = 0;
                for (int v = 0; v <= ((a.fuse_ok & 2) ? 2 : 1); ++v) {
                    auto once = [&]() { return v == 0 ? (conv_run(a, lf, pr.x, pr.gx, 0, nullptr) || conv_run(b, lf, pr.x, pr.gx, 0, nullptr))
                                                      : fused_run(a, b, lf, pr.x, v == 2, nullptr); };
                    if (v > 0 && once()) {       // a fused variant that will not launch is simply not a candidate
                        if (getenv("I2V_FUSE_DEBUG")) fprintf(stderr, "[i2v fuse] pair %zu variant %d does not launch: %s\n", i, v, g_err.c_str());
                        g_err.clear(); continue;
                    }
                    float ms = 0.f;
                    if (pr.time(once, 2, &ms, /*warm_up=*/v == 0)) { rc = 1; break; }      // (a fused variant's trial launch was its warm-up)
                    // one launch instead of two also saves whatever a tracing tool adds per dispatch (under `rocprofv3 --pmc` that made the
                    // fused kernel "win" pairs it loses by 10-40 % in a plain run): it has to be 3 % faster to be taken
                    if ((v == 0 ? ms : ms * 1.03f) < best) { best = v == 0 ? ms : ms * 1.03f; best_v = v; }
                    if (getenv("I2V_FUSE_DEBUG"))
                        fprintf(stderr, "[i2v fuse] %s pair %zu (Cd %d -> %d, %dx%d) at %d frames: variant %d = %.1f us\n", list_name(n, L), i,
                                a.conv.Cd, b.conv.Cd, a.conv.Hg, a.conv.Wg, lf, v, 1e3f * ms);
                }
                a.fuse_b[bk] = best_v;
                a.conv.cfg = ca; b.conv.cfg = cb;
                return rc;
            });
            if (rc) return 1;
        }
    return 0;
}

// Shortcut pairs, per batch bucket: the two launches on their tuned tiles against the pair as one kernel, three timed runs each; the
// faster stays.  (No handicap for the single launch as in tune_pairs: the pair removes memory traffic, it is not a wash that only a
// tool's per-dispatch overhead decides.)
int tune_scpairs(Net& n, Probe& pr, int max_clips) {
    for (std::vector<Launch>* L : {&n.fwd, &n.bwd})
        for (size_t i = 0; i < L->size(); ++i) {
            Launch& a = (*L)[i];
            if (!a.sc_ok || i + a.sc_ok >= L->size()) continue;
            Launch& b = (*L)[i + a.sc_ok];
            const int rc = for_each_bucket(max_clips, a.conv.Tg, [&](int bk, int lf) -> int {
                if (lf * a.conv.Hg * a.conv.Wg == 0 || !sc_fits(a, b, lf)) return 0;
                const int ca = a.conv.cfg, cb = b.conv.cfg;
                if (a.cfg_b[bk]) a.conv.cfg = a.cfg_b[bk];
                if (b.cfg_b[bk]) b.conv.cfg = b.cfg_b[bk];
                float t_sep = 0.f, t_pair = 0.f;
                const int rc = pr.time([&] { return conv_run(a, lf, pr.x, pr.gx, 0, nullptr) || conv_run(b, lf, pr.x, pr.gx, 0, nullptr); }, 3, &t_sep) ||
                               pr.time([&] { return sc_run(a, b, lf, nullptr); }, 3, &t_pair);
                a.conv.cfg = ca; b.conv.cfg = cb;
                if (rc) return 1;
                a.sc_b[bk] = t_pair < t_sep ? 1 : 0;
                if (getenv("I2V_FUSE_DEBUG"))
                    fprintf(stderr, "[i2v scpair] %s launches %zu + %zu (K %d + %d -> Cd %d, %dx%d) at %d frames: separate %.1f us, pair %.1f us -> %s\n", list_name(n, L), i,
                            i + a.sc_ok, a.conv.K, b.conv.K, b.conv.Cd, b.conv.Hg, b.conv.Wg, lf, 1e3f * t_sep, 1e3f * t_pair, a.sc_b[bk] ? "pair" : "separate");
                return 0;
            });
            if (rc) return 1;
        }
    return 0;
}

}  // namespace

// Plan-time autotuning ("measure, don't guess"): every convolution launch of both passes is timed with each
// valid tile configuration on the planned shapes (max_frames) and the fastest is pinned.  Tile choice never
// changes results: each output element is the same k-ordered fmaf chain whatever the tile.
int autotune(Net& n) {
    const char* off = getenv("I2V_AUTOTUNE");
    if (off && off[0] == '0') return 0;
    int rc;
    {
        Probe pr;
        if (pr.init(n)) return 1;
        const int max_clips = n.maxN / n.Tin();
        // the fused groups: only where timing means something (the device; the host simulation of the tests has one configuration of everything)
        const bool on_device = strncmp(be_name(), "hip", 3) == 0;
        rc = tune_tiles(n, pr, max_clips);
        if (!rc && on_device) rc = tune_fastblocks(n, pr, max_clips);
        if (!rc && on_device) rc = tune_scpairs(n, pr, max_clips);
        // Pairs are opt-in (I2V_FUSE=1) since round 5: the fused kernel loses 7-35 % on every pair at the headline size and wins 1-2 % on three
        // pairs at 32 frames (profiles/r4_fuse_pairs.txt) -- not worth up to 9 probe launches per pair and bucket in every plan, nor a plan that
        // depends on the process environment (a profiling tool's per-dispatch overhead flatters the single launch).
        static const bool fuse_on = [] { const char* e = getenv("I2V_FUSE"); return e && e[0] == '1'; }();
        if (!rc && fuse_on && on_device) rc = tune_pairs(n, pr, max_clips);
    }
    if (rc) return g_err.empty() ? fail("autotune failed") : 1;
    // the probes scribbled over activations and gradients; start from a clean arena like a fresh plan
    CHECK_BE(be_memset0(n.arena, n.arena_floats * sizeof(float), nullptr));
    return 0;
}

}  // namespace eng
