// Weight packing: every convolution's operands as the kernels read them (see the file header of i2v_engine.cpp).
#include "i2v_net.h"
#include "i2v_conv_aux.h"

#include <stdlib.h>
#include <string.h>

#include <algorithm>

namespace eng {

// Math mode of a plan.  Default: every convolution on fp32-input MFMAs (exact fp32: a k-ordered fmaf chain, the bit-exact rungs of
// the parity ladder).  I2V_MATH=bf16x3 (opt-in, round 5): launches the split-bf16 K loop admits (conv_bf3_ok) run on three-term bf16
// operands -- six bf16 MFMAs per 16 K rows in place of eight fp32 ones at twice the cycles, every product term down to 2^-26 of |w||x|
// kept, fp32 accumulation.  Read when a net is PLANNED (one process may hold plans of both kinds); results of a plan do not depend on
// the autotuner's tile choices in either mode.
bool math_bf16x3() { const char* e = getenv("I2V_MATH"); return e && !strcmp(e, "bf16x3"); }

// w = w1 + w2 + w3 in bf16 (round to nearest even at every level; the residuals are exact in fp32), laid out in the 32x32x16 bf16 MFMA's
// A-fragment order: [Kpad / 16][Cdpad / 32][term][lane][8]: lane l holds row 32 tile + (l & 31), K rows 16 chunk + 8 (l >> 5) + j.
static int upload_split_bf16(Net& n, const std::vector<float>& wp, Packed& P) {
    if (!math_bf16x3() || P.quad || P.Kpad % I2V_KC || P.Cdpad % 32 || P.Kpad == 0) return 0;
    auto bf = [](float x) { uint32_t u; memcpy(&u, &x, 4); u = (u + 0x7fffu + ((u >> 16) & 1u)) & 0xffff0000u; float y; memcpy(&y, &u, 4); return y; };
    const int nch = P.Kpad / I2V_KC, nt = P.Cdpad / 32;
    std::vector<uint16_t> w3((size_t)nch * nt * 3 * 64 * 8);
    for (int c = 0; c < nch; ++c)
        for (int t = 0; t < nt; ++t)
            for (int l = 0; l < 64; ++l)
                for (int j = 0; j < 8; ++j) {
                    float w = wp[(size_t)(16 * c + 8 * (l >> 5) + j) * P.Cdpad + 32 * t + (l & 31)];
                    for (int term = 0; term < 3; ++term) {
                        const float b = bf(w); uint32_t u; memcpy(&u, &b, 4);
                        w3[((((size_t)c * nt + t) * 3 + term) * 64 + l) * 8 + j] = (uint16_t)(u >> 16);
                        w -= b;
                    }
                }
    return upload(n, w3, &P.wp3);
}

// ---------------------------------------------------------------------------------------------
// weight packing
// ---------------------------------------------------------------------------------------------
static int floordiv(int a, int b) { return (a >= 0) ? a / b : -((-a + b - 1) / b); }
static int posmod(int a, int b) { int m = a % b; return m < 0 ? m + b : m; }

int pack_fwd(Net& n, Node& nd) {
    const i2v_conv3d_desc& c = nd.cd;
    const Buffer& sb = n.bufs[n.tens[c.src].buf];
    int K = c.kt * c.kh * c.kw * c.cin;
    Packed& P = nd.fwd;
    P.K = K; P.Kpad = (int)align_up(K, I2V_KC); P.Cd = c.cout; P.Cdpad = (int)align_up(c.cout, 128);
    P.tap_uniform = (c.cin % I2V_KC == 0) ? 1 : 0;
    if (P.tap_uniform && c.kt == 1 && c.kh == 3 && c.kw == 3 && c.stride == 1 && c.stride_t == 1 && c.pad == 1 && !nd.preact()) P.halo = 9;
    // "Quad rows" for narrow stems (few input channels AND few output channels: SlowFast's fast pathway, 3 -> 8): such a launch
    // spends its time ISSUING the 4-byte im2col DMA of the per-row path (one instruction per K row and 64 pixels; 17 TFLOP/s),
    // not in the matrix pipe.  K rows ordered (channel, frame tap, row tap, column-tap quad x 4) put four ADJACENT source pixels
    // in consecutive rows, which the kernel (MODE 4) stages with ONE 16-byte DMA per pixel: 1.6x on that launch
    // (tools/conv_microbench.cpp "fast stem").  Wide stems (64 output channels) are bound elsewhere and measured no gain.
    static const bool no_quad = [] { const char* e = getenv("I2V_QUAD"); return e && e[0] == '0'; }();
    if (!no_quad && c.cin < I2V_KC && c.cout <= 32 && c.kw >= 2 && c.kw <= 8 && !nd.preact()) {
        const int kwq = (c.kw + 3) / 4;
        // Frame PAIRS (round 3): with <= 8 output channels (SlowFast's fast stem) half of even a 16-row fragment is empty.  Two
        // consecutive output frames share most of their source frames when the kernel spans time (5 taps at stride = dilation 2:
        // six distinct source frames for the pair instead of ten), so one grid frame computes BOTH -- rows (frame class, channel), K
        // rows over the UNION of the pair's frame taps, zero weights where a class has no tap there -- with 0.6x the matrix work
        // and im2col traffic of two half-empty launches.  A zero weight adds an exact +0 to the k-ordered chain and the real taps
        // keep their order: same bits as the unpaired packing.  The epilogue is the class-packed one of the image gradient
        // (I2VConvParams::blkt = 2: row -> channel, frame 2 tau + class).
        static const bool no_tpair = [] { const char* e = getenv("I2V_TPAIR"); return e && e[0] == '0'; }();
        const Buffer& dbuf = n.bufs[n.tens[c.dst].buf];
        std::vector<int> taps;                       // frame offsets relative to the grid frame's base source frame
        const int classes = (!no_tpair && c.kt > 1 && 2 * c.cout <= 16 && dbuf.T >= 2) ? 2 : 1;
        for (int ct = 0; ct < classes; ++ct)
            for (int q = 0; q < c.kt; ++q) {
                const int u = ct * c.stride_t + q * c.dil_t - c.pad_t;
                if (std::find(taps.begin(), taps.end(), u) == taps.end()) taps.push_back(u);
            }
        std::sort(taps.begin(), taps.end());
        const int NU = (int)taps.size();
        if (classes == 2) { P.tpair = 2; P.Cd = 2 * c.cout; P.Cdpad = (int)align_up(P.Cd, 128); }
        P.K = c.cin * NU * c.kh * kwq * 4; P.Kpad = (int)align_up(P.K, I2V_KC); P.tap_uniform = 0;
        P.quad = kwq; P.quad_kw = c.kw; P.quad_dw0 = -c.pad;
        if (c.kh == 7 && c.kw == 7 && c.pad == 3) P.halo = 77;      // seven row taps from -3: what conv_stem_halo's window (37 rows from 2 y0 - 3, 56 K rows per plane) is built for
        std::vector<float> wq((size_t)P.Kpad * P.Cdpad, 0.f);
        std::vector<I2VKEntry> kq(P.Kpad, I2VKEntry{0, 0, 0, 0});
        for (int ci = 0; ci < c.cin; ++ci)
            for (int ui = 0; ui < NU; ++ui)
                for (int r = 0; r < c.kh; ++r)
                    for (int s4 = 0; s4 < kwq * 4; ++s4) {
                        const int k = (((ci * NU + ui) * c.kh + r) * kwq) * 4 + s4;
                        kq[k] = I2VKEntry{ci * sb.H * sb.W, r - c.pad, s4 - c.pad, (s4 < c.kw ? 1 : 0) + 2 * taps[ui]};
                        if (s4 >= c.kw) continue;
                        for (int ct = 0; ct < classes; ++ct) {
                            const int num = taps[ui] - ct * c.stride_t + c.pad_t;       // = q * dil_t for this class's tap q
                            if (num < 0 || num % c.dil_t || num / c.dil_t >= c.kt) continue;
                            const int q = num / c.dil_t;
                            for (int co = 0; co < c.cout; ++co)
                                wq[(size_t)k * P.Cdpad + ct * c.cout + co] = nd.w[((((size_t)co * c.cin + ci) * c.kt + q) * c.kh + r) * c.kw + s4];
                        }
                    }
        for (const I2VKEntry& e : kq) if (e.valid >> 1) P.has_dt = 1;
        if (upload(n, wq, &P.wp)) return 1;
        return upload(n, kq, &P.ktab);
    }
    // the 7x7 / stride-2 / pad-3 stem over 3 channels in (tap, channel) order: conv_stem64_halo may walk it without the k-table
    if (!P.tap_uniform && c.cin == 3 && c.kt == 1 && c.kh == 7 && c.kw == 7 && c.stride == 2 && c.pad == 3 && c.dil_t == 1 && c.pad_t == 0 && !nd.preact()) P.halo = 49;
    if (c.kh == 1 && c.kw == 1 && c.pad == 0 && c.stride == 1 && !nd.preact()) P.halo = 1;      // every tap at (0, 0): k x 1 x 1 (conv_vfma_kernel's mark)
    std::vector<float> wp((size_t)P.Kpad * P.Cdpad, 0.f);
    std::vector<I2VKEntry> kt(P.Kpad, I2VKEntry{0, 0, 0, 0});
    // K order: (16-channel chunk, tap, channel in chunk) when the channel count allows -- each 16-row chunk keeps a
    // single tap (MODE 2) and consecutive chunks re-read the same 16 channels at the next tap, a few KB apart in
    // the cache instead of a full channel sweep apart -- else (tap, channel).
    const int NT = c.kt * c.kh * c.kw;
    for (int q = 0; q < c.kt; ++q)
        for (int r = 0; r < c.kh; ++r)
            for (int s = 0; s < c.kw; ++s)
                for (int ci = 0; ci < c.cin; ++ci) {
                    const int tap = (q * c.kh + r) * c.kw + s;
                    int k = P.tap_uniform ? ((ci / I2V_KC) * NT + tap) * I2V_KC + ci % I2V_KC : tap * c.cin + ci;
                    kt[k] = I2VKEntry{ci * sb.H * sb.W, r - c.pad, s - c.pad, 1 + 2 * (q * c.dil_t - c.pad_t)};
                    for (int co = 0; co < c.cout; ++co)
                        wp[(size_t)k * P.Cdpad + co] = nd.w[((((size_t)co * c.cin + ci) * c.kt + q) * c.kh + r) * c.kw + s];
                }
    for (const I2VKEntry& e : kt) if (e.valid >> 1) P.has_dt = 1;
    if (upload(n, wp, &P.wp) || upload_split_bf16(n, wp, P)) return 1;
    return upload(n, kt, &P.ktab);
}

// Input-gradient operands, one per stride-parity class (pt, ph, pw): the source positions congruent to the
// class modulo the stride receive exactly the taps with (class + pad - tap) % stride == 0.
int pack_bwd(Net& n, Node& nd) {
    const i2v_conv3d_desc& c = nd.cd;
    const Buffer& sb = n.bufs[n.tens[c.src].buf];
    const Buffer& db = n.bufs[n.tens[c.dst].buf];
    int st = c.stride, stt = c.stride_t;
    for (int pt = 0; pt < stt; ++pt)
    for (int ph = 0; ph < st; ++ph)
        for (int pw = 0; pw < st; ++pw) {
            Packed P;
            P.pt = pt; P.ph = ph; P.pw = pw;
            P.Tg = (sb.T - pt + stt - 1) / stt;
            P.Hg = (sb.H - ph + st - 1) / st; P.Wg = (sb.W - pw + st - 1) / st;
            std::vector<int> tq, tr, ts;
            for (int q = 0; q < c.kt; ++q) if (posmod(pt + c.pad_t - q * c.dil_t, stt) == 0) tq.push_back(q);
            for (int r = 0; r < c.kh; ++r) if (posmod(ph + c.pad - r, st) == 0) tr.push_back(r);
            for (int s = 0; s < c.kw; ++s) if (posmod(pw + c.pad - s, st) == 0) ts.push_back(s);
            int K = (int)(tq.size() * tr.size() * ts.size()) * c.cout;
            P.K = K; P.Kpad = (int)align_up(K, I2V_KC); P.Cd = c.cin; P.Cdpad = (int)align_up(c.cin, 128);
            P.tap_uniform = (c.cout % I2V_KC == 0) ? 1 : 0;
            if (P.tap_uniform && st == 1 && stt == 1 && c.kt == 1 && c.kh == 3 && c.kw == 3 && c.pad == 1 && !nd.preact()) P.halo = 9;
            if (c.kh == 1 && c.kw == 1 && c.pad == 0 && st == 1 && !nd.preact()) P.halo = 1;      // every tap at (0, 0)
            std::vector<float> wp((size_t)P.Kpad * P.Cdpad, 0.f);
            std::vector<I2VKEntry> kt(P.Kpad ? P.Kpad : 1, I2VKEntry{0, 0, 0, 0});
            int t = 0;
            const int NTc = (int)(tq.size() * tr.size() * ts.size());
            for (int q : tq)
            for (int r : tr)
                for (int s : ts) {
                    int dt = floordiv(pt + c.pad_t - q * c.dil_t, stt);
                    int dh = floordiv(ph + c.pad - r, st), dw = floordiv(pw + c.pad - s, st);
                    for (int co = 0; co < c.cout; ++co) {
                        int k = P.tap_uniform ? ((co / I2V_KC) * NTc + t) * I2V_KC + co % I2V_KC : t * c.cout + co;
                        kt[k] = I2VKEntry{co * db.H * db.W, dh, dw, 1 + 2 * dt};
                        for (int ci = 0; ci < c.cin; ++ci)
                            wp[(size_t)k * P.Cdpad + ci] =
                                nd.w[((((size_t)co * c.cin + ci) * c.kt + q) * c.kh + r) * c.kw + s] * (nd.preact() ? nd.pre_scale[ci] : 1.f);
                    }
                    ++t;
                }
            for (const I2VKEntry& e : kt) if (e.valid >> 1) P.has_dt = 1;
            if (upload(n, wp, &P.wp) || upload_split_bf16(n, wp, P)) return 1;
            if (upload(n, kt, &P.ktab)) return 1;
            nd.bwd.push_back(P);
        }
    return 0;
}

// Grouped nodes run on k_gconv where the library has it (the product build defines I2V_HAVE_GCONV; the host simulation's one-file
// build does not) unless I2V_GCONV=0 asks for the dense route: the block-diagonal weight through the packings above.  Read per plan.
bool gconv_enabled() {
#ifdef I2V_HAVE_GCONV
    const char* e = getenv("I2V_GCONV");
    return !(e && e[0] == '0');
#else
    return false;
#endif
}

// k_gconv's operands (I2VGConvParams::w).  Forward: [group][ci][tap 3 r + s][co].  Input gradient: per stride-parity class (ph, pw) --
// the classes of pack_bwd, in its order -- [group][co][slot 3 a + b][ci] with a - 1 = (ph + 1 - r) / stride for the row taps r the class
// owns (b alike), zeros in the slots it does not; gw_tapmask has a bit per owned slot.
int pack_gconv(Net& n, Node& nd) {
    const i2v_conv3d_desc& c = nd.cd;
    const int G = nd.groups, gw = c.cin / G, st = c.stride;
    std::vector<float> wf(conv_aux::gconv_fwd_floats(G, gw));
    conv_aux::gconv_pack_fwd(nd.wg.data(), G, gw, wf.data());
    if (upload(n, wf, &nd.gw_fwd)) return 1;
    std::vector<float> wb(conv_aux::gconv_bwd_floats(G, gw, st));
    conv_aux::gconv_pack_bwd(nd.wg.data(), G, gw, st, wb.data(), nd.gw_tapmask);
    return upload(n, wb, &nd.gw_bwd);
}

// Depthwise nodes run on k_dwconv where the library has it (-DI2V_HAVE_DWCONV: the product build) unless I2V_DWCONV=0 asks for the
// dense route.  Read per plan.
bool dwconv_enabled() {
#ifdef I2V_HAVE_DWCONV
    const char* e = getenv("I2V_DWCONV");
    return !(e && e[0] == '0');
#else
    return false;
#endif
}

// k_dwconv's operands (I2VDwConvParams::w).  Forward: the filter as it is, [C][k r + s].  Input gradient: per stride-parity class (ph,
// pw) -- the classes of pack_bwd, in its order -- [C][slot k a + b] with a - pad = (ph + pad - r) / stride for the row taps r the class
// owns (b alike): the mirrored filter, zeros in the slots the class does not own; gw_tapmask has a bit per owned slot.
int pack_dwconv(Net& n, Node& nd) {
    const i2v_conv3d_desc& c = nd.cd;
    if (upload(n, nd.wg, &nd.gw_fwd)) return 1;
    std::vector<float> wb(conv_aux::dwconv_bwd_floats(c.cin, c.kh, c.stride));
    conv_aux::dwconv_pack_bwd(nd.wg.data(), c.cin, c.kh, c.stride, wb.data(), nd.gw_tapmask);
    return upload(n, wb, &nd.gw_bwd);
}

// Gradient of the FIRST convolution w.r.t. the image.  GEMM-N would be Cin = 3; instead the output is
// cut into B x B position blocks (B = stride, or 2 for stride 1) and the B*B*Cin (class, channel)
// pairs form the Cd axis: out[(ph,pw),ci][i][j] = sum_{co,dh,dw} w'[(co,dh,dw)][(ph,pw),ci] *
// dz[co][i*m + dh][j*m + dw], m = B/stride, with zero weights where a class has no such tap.
// The packings that suit the 16-row halo-tile kernel (conv_imggrad_halo) are chosen when it is among the autotuner's candidates
// (I2V_IGHALO not 0) and not switched off (I2V_IMG_SPLIT=0: the round-3 packings; read per plan so that tests can compare the two)
static bool img_prefer_16_rows() {
    static const bool no_igh = [] { const char* e = getenv("I2V_IGHALO"); return e && e[0] == '0'; }();
    const char* const es = getenv("I2V_IMG_SPLIT");
    return !no_igh && !(es && es[0] == '0');
}
// `only_ct` >= 0: pack that temporal class ALONE -- grid = its own frames, its own frame taps --, as the frame-skipping case below does
// for the one class that has taps (pack_img decides when a dense temporal stride is split into one launch per class).
static int pack_img_one(Net& n, Node& nd, Node::ImgGrad& ig, const int only_ct) {
    const i2v_conv3d_desc& c = nd.cd;
    const Buffer& sb = n.bufs[n.tens[c.src].buf];
    const Buffer& db = n.bufs[n.tens[c.dst].buf];
    const int st = c.stride, B = st == 1 ? 2 : st, m = B / st;
    const int stt = c.stride_t;
    // temporal classes: one per stride residue (1 for images).  A stem that samples every stt-th frame with a
    // kernel that reaches no other residue (SlowFast's slow pathway: kt = 1) has taps in ONE class only: then
    // only that class is packed (grid = the sampled frames, output stride stt) and the frames in between are
    // zero-filled by a memset instead of being computed as stt - 1 classes of zero weights.
    int with_taps = 0, only = 0;
    for (int ct = 0; ct < stt; ++ct) {
        bool any = false;
        for (int q = 0; q < c.kt; ++q) if (posmod(ct + c.pad_t - q * c.dil_t, stt) == 0) any = true;
        if (any) { with_taps++; only = ct; }
    }
    const bool forced = only_ct >= 0;
    if (forced) only = only_ct;
    const bool sparse = forced || (stt > 1 && with_taps == 1);
    int Bt = sparse ? 1 : stt; const int ct0 = sparse ? only : 0;
    static const bool no_tpair = [] { const char* e = getenv("I2V_TPAIR"); return e && e[0] == '0'; }();
    // (Tried and dropped for the DENSE temporal stride of I3D's stem: two stride periods per grid frame -- 48 of 64 rows over 4 dz frames
    //  instead of 2 x (24 of 32 over 3) -- runs the 64-row tiles and was 23 % SLOWER, 1343 -> 1657 us per launch.)
    int dt_lo = 1 << 30, dt_hi = -(1 << 30), dh_lo = 1 << 30, dh_hi = -(1 << 30), dw_lo = 1 << 30, dw_hi = -(1 << 30);
    for (int ct = ct0; ct < ct0 + Bt; ++ct)
        for (int q = 0; q < c.kt; ++q)
            if (posmod(ct + c.pad_t - q * c.dil_t, stt) == 0) { int d = floordiv(ct + c.pad_t - q * c.dil_t, stt); dt_lo = d < dt_lo ? d : dt_lo; dt_hi = d > dt_hi ? d : dt_hi; }
    for (int ph = 0; ph < B; ++ph)
        for (int r = 0; r < c.kh; ++r)
            if (posmod(ph + c.pad - r, st) == 0) { int d = floordiv(ph + c.pad - r, st); dh_lo = d < dh_lo ? d : dh_lo; dh_hi = d > dh_hi ? d : dh_hi; }
    for (int pw = 0; pw < B; ++pw)
        for (int s = 0; s < c.kw; ++s)
            if (posmod(pw + c.pad - s, st) == 0) { int d = floordiv(pw + c.pad - s, st); dw_lo = d < dw_lo ? d : dw_lo; dw_hi = d > dw_hi ? d : dw_hi; }
    const int TH = dh_hi - dh_lo + 1, TW = dw_hi - dw_lo + 1;
    // Pairs of SAMPLED frames (round 3; the gradient-side twin of pack_fwd's frame pairs): a frame-skipping stem whose kernel spans
    // time (SlowFast's fast stem: every 2nd frame, 5 taps) gives each sampled frame 5 dz frames, two neighbouring sampled frames 6
    // between them -- both as temporal classes of ONE grid frame: 24 of 32 rows over 6 frame taps instead of two launches' worth
    // of 12 of 16 rows over 5.  The classes lie stt frames apart (I2VConvParams::oct).  Zero weights where a class has no tap: same bits.
    // ... unless the 16-row halo-tile kernel can take the UNPAIRED quad-row packing (round 5: a 4 x 4 tap window, the frame-tap planes of
    // 1, 2 or 4 channels -- a whole number of four-chunk groups -- within its 20 planes): 12 of 16 rows over the sampled frame's own 5
    // taps is 17 % less matrix work than 24 of 32 over 6, and that kernel stages a plane once whatever the row count.
    const int TTu = dt_hi - dt_lo + 1, cps_u = TTu % 4 == 0 ? 1 : TTu % 2 == 0 ? 2 : 4;
    const bool unpaired_halo = img_prefer_16_rows() && c.cout % I2V_KC != 0 && TH == 4 && TW >= 2 && TW <= 4 && c.cout % cps_u == 0 && cps_u * TTu <= 20 &&
                               B * B * c.cin <= 16 && m == 1;
    const bool pairs = sparse && !forced && !no_tpair && !unpaired_halo && dt_hi > dt_lo && 2 * B * B * c.cin <= 32 && (sb.T - ct0 + stt - 1) / stt >= 2;
    if (pairs) { Bt = 2; dt_hi += 1; }
    const int TT = dt_hi - dt_lo + 1;
    Packed& P = ig.P;
    // few output channels (SlowFast's fast stem: 8) cannot use the tap-uniform path; instead of the per-row path they take the
    // "quad rows" order (channel, frame tap, row tap, column-tap quad x 4): see pack_fwd
    static const bool no_quad = [] { const char* e = getenv("I2V_QUAD"); return e && e[0] == '0'; }();
    // Round 5, measured and NOT taken (opt-in I2V_IMG_QUAD=1): quad rows for the stride-2 7x7 stems with 64 output channels (ResNet, I3D, SlowFast's
    // slow pathway) too.  Their class-packed gradient has exactly FOUR column taps per row run (TW = 4: one quad, no padding) and issues 16
    // four-byte im2col DMA pieces per wave and chunk beside 16 MFMAs of 32 cycles (PMC: matrix pipe 0.59 busy); as quad rows the same chunk is four
    // 16-byte pieces per wave.  Slower all the same: image gradient 52.0 -> 44.6 TFLOP/s on the I2V stem, 60.7 -> 53.6 on I3D's, 43.7 -> 40.0 on
    // SlowFast's (gpurun_out r5p, same box, alternated): the channel-major K order sweeps one channel's 4 x 4 window per chunk, and the masked
    // fragment reads of MODE 4 cost more than the DMA instructions they save.  Same products either way (the host simulation follows the k-table).
    static const bool img_quad = [] { const char* e = getenv("I2V_IMG_QUAD"); return e && e[0] == '1'; }();
    const bool quad = !no_quad && (c.cout % I2V_KC != 0 || (img_quad && TW == 4)) && TW >= 2 && TW <= 8;
    const int TWq = quad ? (TW + 3) / 4 * 4 : TW;               // column taps per run, padded to whole quads
    P.K = TT * TH * TWq * c.cout; P.Kpad = (int)align_up(P.K, I2V_KC);
    P.Cd = Bt * B * B * c.cin; P.Cdpad = (int)align_up(P.Cd, 128);
    P.tap_uniform = (!quad && c.cout % I2V_KC == 0) ? 1 : 0;
    if (quad) { P.quad = TWq / 4; P.quad_kw = TW; P.quad_dw0 = dw_lo; }
    if (P.tap_uniform) { P.ig_tt = TT; P.ig_th = TH; P.ig_tw = TW; }
    else if (quad && TWq == 4 && TH == 4) { P.ig_tt = TT; P.ig_th = TH; P.ig_tw = TWq; }      // (conv_imggrad_halo, QUAD: one 4 x 4 plane per chunk)
    P.Tg = sparse ? (sb.T - ct0 + stt - 1) / stt : (sb.T + Bt - 1) / Bt; P.Hg = (sb.H + B - 1) / B; P.Wg = (sb.W + B - 1) / B;
    ig.blk = B; ig.sh = m; ig.blkt = Bt; ig.ost = sparse ? stt : Bt; ig.ot0 = ct0; ig.skips = sparse && !forced;
    if (pairs) { P.Tg = (P.Tg + 1) / 2; ig.ost = 2 * stt; ig.st = 2; ig.oct = stt; }
    {   // this launch's part of the node's algorithmic flops: its classes' frame taps over all of them
        int mine = 0, all = 0;
        for (int ct = 0; ct < stt; ++ct)
            for (int q = 0; q < c.kt; ++q)
                if (posmod(ct + c.pad_t - q * c.dil_t, stt) == 0) { ++all; if (!forced || ct == only_ct) ++mine; }
        ig.flop_share = all > 0 ? (double)mine / all : 1.0;
    }
    std::vector<float> wp((size_t)P.Kpad * P.Cdpad, 0.f);
    std::vector<I2VKEntry> kt(P.Kpad, I2VKEntry{0, 0, 0, 0});
    // K order = (16-channel chunk, tap, channel in chunk) when the channel count allows: every 16-row K chunk
    // still has ONE tap (MODE 2), and a block sweeps all taps of 16 channels before moving on, so the taps'
    // overlapping reads of `dz` are a few KB apart instead of a full 64-channel sweep apart (the co-resident
    // blocks' halos then fit the L2).  Otherwise (tap, channel) -- or the quad-row order.
    const int NT = TT * TH * TW;
    auto krow = [&](int tt, int th, int tw, int co) {
        if (quad) return (((co * TT + tt) * TH + th) * TWq) + tw;
        const int tap = (tt * TH + th) * TW + tw;
        return P.tap_uniform ? ((co / I2V_KC) * NT + tap) * I2V_KC + co % I2V_KC : tap * c.cout + co;
    };
    for (int tt = 0; tt < TT; ++tt)
    for (int th = 0; th < TH; ++th)
        for (int tw = 0; tw < TWq; ++tw)
            for (int co = 0; co < c.cout; ++co)
                kt[krow(tt, th, tw, co)] = I2VKEntry{co * db.H * db.W, th + dh_lo, tw + dw_lo, (tw < TW ? 1 : 0) + 2 * (tt + dt_lo)};
    for (int cc = 0; cc < Bt; ++cc)
    for (int q = 0; q < c.kt; ++q) {
        const int ct = pairs ? ct0 : ct0 + cc;          // (pairs: both classes are the ONE residue with taps, a sampled frame apart)
        if (posmod(ct + c.pad_t - q * c.dil_t, stt)) continue;
        const int tt = floordiv(ct + c.pad_t - q * c.dil_t, stt) - dt_lo + (pairs ? cc : 0);
        for (int ph = 0; ph < B; ++ph)
            for (int pw = 0; pw < B; ++pw)
                for (int r = 0; r < c.kh; ++r) {
                    if (posmod(ph + c.pad - r, st)) continue;
                    const int th = floordiv(ph + c.pad - r, st) - dh_lo;
                    for (int s = 0; s < c.kw; ++s) {
                        if (posmod(pw + c.pad - s, st)) continue;
                        const int tw = floordiv(pw + c.pad - s, st) - dw_lo;
                        for (int co = 0; co < c.cout; ++co)
                            for (int ci = 0; ci < c.cin; ++ci)
                                wp[(size_t)krow(tt, th, tw, co) * P.Cdpad + ((cc * B + ph) * B + pw) * c.cin + ci] =
                                    nd.w[((((size_t)co * c.cin + ci) * c.kt + q) * c.kh + r) * c.kw + s];
                    }
                }
    }
    for (const I2VKEntry& e : kt) if (e.valid >> 1) P.has_dt = 1;
    // conv_igvfma_kernel skips the class-row pairs a tap cannot feed under the stride-2 7 x 7 geometry (row class ph owns row tap th iff
    // ph == 1 || th < 3, column class alike): claimed only when EVERY weight outside that pattern is an exact zero in this packing
    if (quad && TWq == 4 && TH == 4 && Bt == 1 && B == 2 && c.cin == 3 && P.Cd == 12) {
        bool ok = true;
        for (int k = 0; k < P.K && ok; ++k) {
            const int tw = k % 4, th = (k / 4) % 4;
            for (int cd = 0; cd < 12 && ok; ++cd) {
                const int cls = cd / 3, ph = cls / 2, pw = cls % 2;
                const bool owned = (ph == 1 || th < 3) && (pw == 1 || tw < 3);
                if (!owned && wp[(size_t)k * P.Cdpad + cd] != 0.f) ok = false;
            }
        }
        P.ig_p77 = ok ? 1 : 0;
        std::vector<float> wc((size_t)P.Kpad * 16, 0.f);             // rows of 16 floats for the vector-FMA kernel's scalar loads
        for (int k = 0; k < P.K; ++k) for (int cd = 0; cd < 12; ++cd) wc[(size_t)k * 16 + cd] = wp[(size_t)k * P.Cdpad + cd];
        if (upload(n, wc, &P.wpc)) return 1;
    }
    if (upload(n, wp, &P.wp)) return 1;
    return upload(n, kt, &P.ktab);
}

// The input gradient of a stem as one class-packed launch -- or, for a DENSE temporal stride (I3D: 5x7x7 / (2,2,2): two temporal classes
// with 3 and 2 frame taps), one launch per temporal class: packed together the classes share the union of their frame taps (3) and a
// 32-row fragment (24 of 32 rows), alone each runs its own taps on 12 of 16 rows -- 5 x 16 instead of 3 x 32 row-taps per pair of
// frames, and the 16-row conv_imggrad_halo keeps six blocks per CU where the 32-row one keeps four.  Only when that kernel is among the
// candidates (tap-uniform packing of a stride-2 stem, I2V_IGHALO not 0): conv_tile prefers the packed form.  A zero weight adds an exact
// +0 to the k-ordered chain and the real taps keep their order: same bits either way.
int pack_img(Net& n, Node& nd) {
    const i2v_conv3d_desc& c = nd.cd;
    const int stt = c.stride_t, B = c.stride == 1 ? 2 : c.stride;
    int classes_with_taps = 0;
    for (int ct = 0; ct < stt; ++ct) {
        bool any = false;
        for (int q = 0; q < c.kt; ++q) if (posmod(ct + c.pad_t - q * c.dil_t, stt) == 0) any = true;
        classes_with_taps += any ? 1 : 0;
    }
    const bool split = img_prefer_16_rows() && stt > 1 && classes_with_taps == stt && c.cout % I2V_KC == 0 && c.stride == 2 && B * B * c.cin <= 16 &&
                       c.kh <= 8 && c.kw <= 8 && (((c.kh + 1) / 2) * ((c.kw + 1) / 2)) % 4 == 0 && n.bufs[n.tens[c.src].buf].T >= stt;
    nd.imgs.clear();
    if (!split) { nd.imgs.emplace_back(); return pack_img_one(n, nd, nd.imgs.back(), -1); }
    nd.imgs.resize(stt);
    for (int ct = 0; ct < stt; ++ct) if (pack_img_one(n, nd, nd.imgs[ct], ct)) return 1;
    return 0;
}

}  // namespace eng
