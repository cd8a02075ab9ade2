// Planner and executor of the XCiT surrogates (include/i2v_xcit.h) on the transformer stack: one arena per (net, max frames), the forward
// as a fixed launch sequence up to the deepest hooked block, and the input-gradient pass -- no weight gradients.  An XCiT block has three
// sub-layers where the shared block of i2v_xf.h has two, so it is composed here from the shared launches (linear / linear_bwd with their
// bias, GELU, GELU' and residual epilogues, the LayerNorm pair) and the XCiT ones (i2v_xcit.hip; without -DI2V_HAVE_XCIT the scalar
// restatement i2v_xcit_host.h), as i2v_convnext.cpp composes its own:
//   forward   t1 = LN1 x | qkv = qkv(t1) | t1 = XCA(qkv) | y1 = x + proj'(t1)
//             t1 = LN3 y1 | u = dw1(t1) + b1 | y2 = y1 + dw2'(a gelu(u) + s) + b2'
//             t1 = LN2 y2 | h = fc1(t1), t2 = gelu(h) | x' = y2 + fc2'(t2)                       (proj', dw2', b2', fc2': gamma-folded; 12 launches)
//   backward  t2 = (g fc2') gelu'(h) | t1 = t2 fc1 | G = LN2'(t1; y2) + g
//             t1 = dw2'^T(G) a gelu'(u) | dqkv = dw1^T(t1) | G = LN3'(dqkv; y1) + G
//             t1 = G proj' | dqkv = XCA'(t1) | t1 = dqkv qkv | G = LN1'(t1; x) + G (+ the hook at that stream)         (12 launches)
// saved per block: x, qkv, the normalised Gram with the norms, the probabilities, y1, u, y2, h and six LayerNorm statistics per token.
// The stem's four 3 x 3 / 2 convolutions run as a gather launch and the shared linear launch each (bias and GELU in its epilogue, which
// keeps the pre-activation), backward as linear_bwd and a gather-form scatter that multiplies by gelu' of the saved pre-activation.
#include <math.h>

#include <algorithm>

#include "../../include/i2v_xcit.h"
#include "i2v_xf.h"
#ifdef I2V_HAVE_XCIT
#include "i2v_xcit_kernels.h"
#else
#include "i2v_xcit_host.h"      // (the host simulation's one-file build: the launches as scalar code)
#endif
#ifdef I2V_HAVE_CAIT
#include "i2v_cait_kernels.h"   // cait_add_pos: the plain `+ pos` launch of a stem without a prefix token
#else
#include "i2v_cait_host.h"
#endif

namespace {

struct XcBlock : Block {
    const float *temp = nullptr, *n3w = nullptr, *n3b = nullptr, *w1 = nullptr, *b1 = nullptr, *bna = nullptr, *bns = nullptr, *w2 = nullptr,
                *b2 = nullptr;
    const float *w1m = nullptr, *w2m = nullptr;      // the two (9, dim) filters with their rows in reverse order: the input gradient's
    float *gram = nullptr, *u = nullptr, *y2 = nullptr;      // (Block::y is y1, Block::P the probabilities)
};

}  // namespace

struct i2v_xcit : XfNet {
    i2v_xcit_config cfg{};
    int T = 0, gsz = 0, nb = 0;
    int cs[5] = {0, 0, 0, 0, 0}, side[5] = {0, 0, 0, 0, 0};      // the stem's widths (input, dim / 8, dim / 4, dim / 2, dim) and plane sides
    const float *sw[4] = {nullptr, nullptr, nullptr, nullptr}, *sb[4] = {nullptr, nullptr, nullptr, nullptr}, *pos = nullptr;
    float *pre[3] = {nullptr, nullptr, nullptr}, *act[3] = {nullptr, nullptr, nullptr};      // stem stages 1 .. 3: pre-activation, gelu of it
    float *rows = nullptr, *x_top = nullptr;
    std::vector<XcBlock> blocks;

    float* stream_after(int b) { return b + 1 < nb ? blocks[b + 1].x : x_top; }
    float* hook_stream(int b) { return stream_after(b); }
    int64_t hook_floats(int) const { return (int64_t)T * cfg.dim; }
    XcitAttn attn(const XcBlock& B, int frames) const {
        XcitAttn a{};
        a.qkv = B.qkv; a.F = frames; a.T = T; a.H = cfg.heads; a.dh = cfg.dim / cfg.heads; a.temperature = B.temp; a.gram = B.gram; a.probs = B.P;
        return a;
    }
    XcitDw3 dw(const float* x, const float* w, float* y, int frames) const {
        XcitDw3 d{};
        d.x = x; d.w = w; d.y = y; d.N = frames; d.H = gsz; d.W = gsz; d.C = cfg.dim;
        return d;
    }
};

namespace {

// a device copy of the (9, D) filter `host` with its rows in reverse order
int mirrored(Arena& A, const float* host, int64_t D, const float** out) {
    std::vector<float> mir((size_t)9 * D);
    for (int t = 0; t < 9; ++t)
        for (int64_t c = 0; c < D; ++c) mir[(size_t)t * D + c] = host[(size_t)(8 - t) * D + c];
    float* dm = A.alloc(9 * D);
    if (!dm) return A.oom("a mirrored filter");
    HCHK(hipMemcpy(dm, mir.data(), mir.size() * 4, hipMemcpyHostToDevice));
    *out = dm;
    return 0;
}

int xcit_plan(i2v_xcit* n, const float* const* w, int nw, const int32_t* hooks, int n_hooks) {
    const i2v_xcit_config& c = n->cfg;
    Arena& A = n->arena;
    if (c.img <= 0 || c.img % 16 != 0 || c.in_chans <= 0 || c.dim <= 0 || c.dim % 8 != 0 || c.heads <= 0 || c.dim % c.heads != 0 ||
        (c.dim / c.heads) % 4 != 0 || c.mlp <= 0 || c.mlp % 4 != 0 || c.blocks <= 0)
        return fail("i2v_xcit_create: unsupported configuration (img %d dim %d heads %d mlp %d blocks %d)", c.img, c.dim, c.heads, c.mlp, c.blocks);
    if (c.dim / c.heads > XCIT_MAX_DH)
        return fail("i2v_xcit_create: heads of width %d: the dh x dh matrices of one head fit one workgroup up to width %d", c.dim / c.heads,
                    (int)XCIT_MAX_DH);
    n->gsz = c.img / 16;
    n->T = n->gsz * n->gsz;
    n->cs[0] = c.in_chans; n->cs[1] = c.dim / 8; n->cs[2] = c.dim / 4; n->cs[3] = c.dim / 2; n->cs[4] = c.dim;
    for (int k = 0; k < 5; ++k) n->side[k] = c.img >> k;
    const int deepest = Hooks::deepest(hooks, n_hooks, c.blocks, A);
    if (deepest < 0) return 1;
    n->nb = A.depth = deepest + 1;
    const int want = 9 + 21 * n->nb;
    if (nw != want) return fail("i2v_xcit_create: %d weight arrays given, %d expected for %d blocks", nw, want, n->nb);
    const int64_t D = c.dim, T = n->T, F = n->max_frames, H = c.heads, Hm = c.mlp, dh = D / H, FT = F * T;
    std::vector<int64_t> sizes;
    for (int k = 0; k < 4; ++k) { sizes.push_back((int64_t)n->cs[k + 1] * 9 * n->cs[k]); sizes.push_back(n->cs[k + 1]); }
    sizes.push_back(T * D);
    for (int b = 0; b < n->nb; ++b)
        for (int64_t v : {D, D, 3 * D * D, 3 * D, H, D * D, D, D, D, Hm * D, Hm, D * Hm, D, D, D, 9 * D, D, D, D, 9 * D, D}) sizes.push_back(v);
    // the whole plan in floats, in 64 bits, before the first allocation: weights, the stem's saves and scratch, per-block saves, shared
    // scratch, hook gradients
    int64_t rows = 0, stem = 0;
    for (int k = 0; k < 4; ++k) {
        const int64_t P = (int64_t)n->side[k + 1] * n->side[k + 1];
        rows = std::max(rows, F * P * 9 * n->cs[k]);
        if (k < 3) stem += 2 * F * P * n->cs[k + 1];
    }
    int64_t total = rows + stem;
    total += n->nb * (18 * D + FT * (11 * D + 6) + F * H * dh * (2 * dh + 2));
    total += FT * D + FT * D + FT * Hm + FT * 3 * D + FT * D;
    total += n_hooks * FT * D;
    for (int64_t v : sizes) total += v;
    VCHK(A.plan(total, F * n->side[1] * n->side[1]));
    if (rows >= (1ll << 31) || FT * Hm >= (1ll << 31) || F > 65535)
        return fail("i2v_xcit_create: %lld bytes needed: too many frames for one net", (long long)A.planned);
    std::vector<const float*> dev;
    VCHK(A.upload(sizes, w, dev));
    for (int k = 0; k < 4; ++k) { n->sw[k] = dev[2 * k]; n->sb[k] = dev[2 * k + 1]; }
    n->pos = dev[8];
    if (!(n->rows = A.alloc(rows))) return A.oom("the stem's rows");
    for (int k = 0; k < 3; ++k) {
        const int64_t sz = F * n->side[k + 1] * n->side[k + 1] * n->cs[k + 1];
        if (!(n->pre[k] = A.alloc(sz)) || !(n->act[k] = A.alloc(sz))) return A.oom("the stem's saved planes");
    }
    n->blocks.resize(n->nb);
    for (int b = 0; b < n->nb; ++b) {
        XcBlock& B = n->blocks[b];
        const float* const* q = &dev[9 + 21 * b];
        B.weights(q, q + 5);
        B.temp = q[4]; B.n3w = q[13]; B.n3b = q[14]; B.w1 = q[15]; B.b1 = q[16]; B.bna = q[17]; B.bns = q[18]; B.w2 = q[19]; B.b2 = q[20];
        VCHK(mirrored(A, w[9 + 21 * b + 15], D, &B.w1m));
        VCHK(mirrored(A, w[9 + 21 * b + 19], D, &B.w2m));
        if (!(B.x = A.alloc(FT * D)) || !(B.qkv = A.alloc(FT * 3 * D)) || !(B.gram = A.alloc(F * H * (dh + 2) * dh)) ||
            !(B.P = A.alloc(F * H * dh * dh)) || !(B.y = A.alloc(FT * D)) || !(B.u = A.alloc(FT * D)) || !(B.y2 = A.alloc(FT * D)) ||
            !(B.h = A.alloc(FT * Hm)) || !(B.stats = A.alloc(6 * FT)))
            return A.oom("saved activations of a block");
    }
    if (!(n->x_top = A.alloc(FT * D)) || !(n->t1 = A.alloc(FT * D)) || !(n->t2 = A.alloc(FT * Hm)) || !(n->dqkv = A.alloc(FT * 3 * D)) ||
        !(n->G = A.alloc(FT * D)))
        return A.oom("scratch");
    for (int i = 0; i < n_hooks; ++i) VCHK(n->hooks.add(A, hooks[i], FT * D));
    return 0;
}

int xcit_forward(i2v_xcit* n, const float* x, int frames, hipStream_t s) {
    const i2v_xcit_config& c = n->cfg;
    const int D = c.dim, M = frames * n->T;
    const int64_t FT = (int64_t)frames * n->T, sp = (int64_t)n->max_frames * n->T;
    const float* src = x;
    for (int k = 0; k < 4; ++k) {                                        // the stem: gather, Linear with the folded BN (+ GELU)
        const int P = n->side[k + 1], rowsM = frames * P * P, K = 9 * n->cs[k];
        VCHK(xcit_stem_gather(src, n->rows, frames, n->side[k], n->side[k], n->cs[k], k == 0, s));
        if (k < 3) VCHK(linear(n->rows, rowsM, K, n->sw[k], n->sb[k], n->cs[k + 1], nullptr, n->pre[k], n->act[k], s));
        else VCHK(linear(n->rows, rowsM, K, n->sw[k], n->sb[k], D, nullptr, n->blocks[0].x, nullptr, s));
        src = k < 3 ? n->act[k] : nullptr;
    }
    VCHK(cait_add_pos(n->blocks[0].x, n->pos, frames, n->T, D, s));
    for (int b = 0; b < n->nb; ++b) {
        const XcBlock& B = n->blocks[b];
        float* st = B.stats;                                              // [mean1 | rstd1 | mean3 | rstd3 | mean2 | rstd2] at max_frames spacing
        VCHK(vit_layernorm(B.x, FT, D, B.n1w, B.n1b, c.ln_eps, n->t1, st, st + sp, s));
        VCHK(linear(n->t1, M, D, B.qkvw, B.qkvb, 3 * D, nullptr, B.qkv, nullptr, s));
        XcitAttn a = n->attn(B, frames);
        a.out = n->t1;
        VCHK(xcit_attention(a, s));
        VCHK(linear(n->t1, M, D, B.projw, B.projb, D, B.x, B.y, nullptr, s));                    // y1 = x + gamma1 proj(XCA)
        VCHK(vit_layernorm(B.y, FT, D, B.n3w, B.n3b, c.ln_eps, n->t1, st + 2 * sp, st + 3 * sp, s));
        XcitDw3 d1 = n->dw(n->t1, B.w1, B.u, frames);
        d1.b = B.b1;
        VCHK(xcit_dw3(d1, s));                                                                   // u = dw1(LN3 y1) + b1
        XcitDw3 d2 = n->dw(B.u, B.w2, B.y2, frames);
        d2.b = B.b2; d2.ta = B.bna; d2.ts = B.bns; d2.add = B.y;
        VCHK(xcit_dw3(d2, s));                                                                   // y2 = y1 + gamma3 (dw2(bn(gelu(u))) + b2)
        VCHK(vit_layernorm(B.y2, FT, D, B.n2w, B.n2b, c.ln_eps, n->t1, st + 4 * sp, st + 5 * sp, s));
        VCHK(linear(n->t1, M, D, B.fc1w, B.fc1b, c.mlp, nullptr, B.h, n->t2, s));                // h = fc1(LN2 y2), t2 = gelu(h)
        VCHK(linear(n->t2, M, c.mlp, B.fc2w, B.fc2b, D, B.y2, n->stream_after(b), nullptr, s));  // x' = y2 + gamma2 fc2(gelu(h))
    }
    return 0;
}

int xcit_backward(i2v_xcit* n, float* gx, int accumulate, hipStream_t s) {
    const i2v_xcit_config& c = n->cfg;
    const int frames = n->frames, D = c.dim, M = frames * n->T;
    const int64_t FT = (int64_t)frames * n->T, sp = (int64_t)n->max_frames * n->T;
    for (int b = n->nb - 1; b >= 0; --b) {
        // gradient of the stream after block b: the top hook's view for the deepest block, the running gradient G below it (where the LN1
        // backward of block b + 1 has already added the hook at that stream)
        const float* gin = n->grad_in(b, n->nb);
        const XcBlock& B = n->blocks[b];
        const float* st = B.stats;
        VCHK(linear_bwd(gin, M, D, B.fc2w, c.mlp, B.h, n->t2, s));                               // dh = (g fc2') * gelu'(h)
        VCHK(linear_bwd(n->t2, M, c.mlp, B.fc1w, D, nullptr, n->t1, s));                         // d LN2 out
        VCHK(vit_layernorm_bwd(n->t1, B.y2, st + 4 * sp, st + 5 * sp, B.n2w, FT, D, gin, nullptr, n->G, s));      // G = d y2
        XcitDw3 d2 = n->dw(n->G, B.w2m, n->t1, frames);
        d2.ma = B.bna; d2.mu = B.u;
        VCHK(xcit_dw3(d2, s));                                                                   // du = dw2'^T(G) * a gelu'(u)
        VCHK(xcit_dw3(n->dw(n->t1, B.w1m, n->dqkv, frames), s));                                 // d LN3 out
        VCHK(vit_layernorm_bwd(n->dqkv, B.y, st + 2 * sp, st + 3 * sp, B.n3w, FT, D, n->G, nullptr, n->G, s));    // G = d y1
        VCHK(linear_bwd(n->G, M, D, B.projw, D, nullptr, n->t1, s));                             // d attention out
        XcitAttn a = n->attn(B, frames);
        a.dout = n->t1; a.dqkv = n->dqkv;
        VCHK(xcit_attention_bwd(a, s));
        VCHK(linear_bwd(n->dqkv, M, 3 * D, B.qkvw, D, nullptr, n->t1, s));                       // d LN1 out
        VCHK(vit_layernorm_bwd(n->t1, B.x, st, st + sp, B.n1w, FT, D, n->G, n->grad_below(b), n->G, s));   // G = dx (+ hook)
    }
    // the position table is an addend: the stem's output gradient is the stream's
    const float* g = n->G;
    for (int k = 3; k >= 0; --k) {
        const int P = n->side[k + 1], rowsM = frames * P * P, K = 9 * n->cs[k];
        VCHK(linear_bwd(g, rowsM, n->cs[k + 1], n->sw[k], K, nullptr, n->rows, s));
        if (k > 0) {                                                      // d pre-activation of stage k, over its gelu output
            VCHK(xcit_stem_scatter(n->rows, n->pre[k - 1], n->act[k - 1], frames, n->side[k], n->side[k], n->cs[k], 0, 0, s));
            g = n->act[k - 1];
        } else {
            VCHK(xcit_stem_scatter(n->rows, nullptr, gx, frames, n->side[0], n->side[0], n->cs[0], 1, accumulate, s));
        }
    }
    return 0;
}

}  // namespace

extern "C" int i2v_xcit_create(int device, const i2v_xcit_config* cfg, const float* const* weights, int n_weights, const int32_t* hook_blocks,
                               int n_hooks, int max_frames, i2v_xcit_handle* out) {
    return xf_create("i2v_xcit_create", "block", device, cfg, weights, hook_blocks, max_frames, out, [&](i2v_xcit* n) {
        n->cfg = *cfg;
        return xcit_plan(n, weights, n_weights, hook_blocks, n_hooks);
    });
}

extern "C" int i2v_xcit_destroy(i2v_xcit_handle net) { return xf_destroy(net); }

extern "C" int64_t i2v_xcit_workspace_bytes(i2v_xcit_handle net) { return xf_workspace_bytes(net); }

extern "C" int i2v_xcit_forward(i2v_xcit_handle n, const float* x, int frames, void* stream) {
    return xf_forward("i2v_xcit_forward", n, x, frames, stream, xcit_forward);
}

extern "C" int i2v_xcit_backward(i2v_xcit_handle n, float* gx, int accumulate, void* stream) {
    return xf_backward("i2v_xcit_backward", n, gx, accumulate, stream, xcit_backward);
}

extern "C" int i2v_xcit_hook_info(i2v_xcit_handle n, int hook, float** act, int64_t* act_stride, float** grad, int64_t* grad_stride, int64_t* D) {
    return xf_hook_info("i2v_xcit_hook_info", n, hook, act, act_stride, grad, grad_stride, D);
}

extern "C" int i2v_xcit_read_hook(i2v_xcit_handle n, int hook, int which, float* out, int frames, void* stream) {
    return xf_read_hook("i2v_xcit_read_hook", n, hook, which, out, frames, stream);
}

// ---- the kernels on their own ----
extern "C" int i2v_xcit_attention_f32(const float* qkv, int frames, int T, int heads, int dh, const float* temperature, float* gram, float* probs,
                                      float* out, void* stream) {
    XcitAttn a{};
    a.qkv = qkv; a.F = frames; a.T = T; a.H = heads; a.dh = dh; a.temperature = temperature; a.gram = gram; a.probs = probs; a.out = out;
    return xcit_attention(a, (hipStream_t)stream);
}

extern "C" int i2v_xcit_attention_bwd_f32(const float* qkv, const float* gram, const float* probs, const float* dout, int frames, int T, int heads,
                                          int dh, const float* temperature, float* dqkv, void* stream) {
    XcitAttn a{};
    a.qkv = qkv; a.F = frames; a.T = T; a.H = heads; a.dh = dh; a.temperature = temperature;
    a.gram = const_cast<float*>(gram); a.probs = const_cast<float*>(probs); a.dout = dout; a.dqkv = dqkv;
    return xcit_attention_bwd(a, (hipStream_t)stream);
}

extern "C" int i2v_xcit_dw3_f32(const float* x, int n, int H, int W, int C, const float* w, const float* bias, const float* ta, const float* ts,
                                const float* add, const float* ma, const float* mu, float* y, void* stream) {
    XcitDw3 d{};
    d.x = x; d.w = w; d.b = bias; d.ta = ta; d.ts = ts; d.add = add; d.ma = ma; d.mu = mu; d.y = y; d.N = n; d.H = H; d.W = W; d.C = C;
    return xcit_dw3(d, (hipStream_t)stream);
}

extern "C" int i2v_xcit_stem_gather_f32(const float* src, float* rows, int frames, int H, int W, int C, int nchw, void* stream) {
    return xcit_stem_gather(src, rows, frames, H, W, C, nchw, (hipStream_t)stream);
}

extern "C" int i2v_xcit_stem_scatter_f32(const float* drows, const float* pre, float* dst, int frames, int H, int W, int C, int nchw, int accumulate,
                                         void* stream) {
    return xcit_stem_scatter(drows, pre, dst, frames, H, W, C, nchw, accumulate, (hipStream_t)stream);
}
