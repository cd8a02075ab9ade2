// Planner and executor of the ConvNeXt surrogates (include/i2v_convnext.h) on the transformer stack: one arena per (net, max frames),
// the forward as a fixed launch sequence up to the deepest hooked stage, and the input-gradient pass -- no weight gradients.  In
// token-major layout everything of a block behind its depthwise convolution is the LayerNorm + MLP half of a transformer block, so the
// arena, the hook list, the two linear launches (with their bias, GELU and residual epilogues) and the LayerNorm pair are the shared ones
// of i2v_xf.h, the stem is its LayerNorm stem (the one Swin runs) and the downsample's 2 x 2 gather is the Swin patch-merging permutation; this file
// brings the block's launch order, the downsample and the ConvNeXt sizes.  The depthwise kernel is in i2v_convnext.hip.
//
// A block runs in place on its stage's stream x (F, plane^2, w):
//   forward   u = dw(x) + b | t1 = LN(u) | h = fc1(t1), t2 = gelu(h) | x = x + fc2'(t2)            (fc2' = gamma-folded fc2; 4 launches)
//   backward  t2 = (g fc2') * gelu'(h) | t1 = t2 fc1 | t3 = LN'(t1; u) | G = dw^T(t3) + g          (g: the gradient of the block's output)
// saved per block: u, h and the LayerNorm's two statistics per position.
#include "../../include/i2v_convnext.h"
#include "i2v_swin_kernels.h"
#include "i2v_xf.h"
#ifndef I2V_HAVE_CONVNEXT
#include "i2v_convnext_host.h"     // (the host simulation's one-file build: the depthwise launch as scalar code)
#endif

namespace {

struct CnBlock {
    const float *dww, *dwm, *dwb, *nw, *nb, *fc1w, *fc1b, *fc2w, *fc2b;   // dww: the (49, w) filter; dwm: the same mirrored (row 48 - t)
    float *u, *h, *stats;                                                  // saved: dw output, fc1 pre-activation, LN mean | rstd
    I2VCnDwParams fwd, bwd;
};

struct CnStage {
    int grid = 0, width = 0;
    std::vector<CnBlock> blocks;
    float* x = nullptr;                      // the stage's stream: its input, every block's output in turn, at the end the hooked feature
    // the downsample in front of the stage (i >= 1): LN over the previous stage's width, gather, Linear
    const float *dnw = nullptr, *dnb = nullptr, *dlw = nullptr, *dlb = nullptr;
    float* dstats = nullptr;                 // the LN's statistics over the PREVIOUS stage's positions
    int64_t T() const { return (int64_t)grid * grid; }
};

}  // namespace

struct i2v_convnext : XfNet {
    i2v_convnext_config cfg{};
    int ns = 0, gsz = 0;
    const float *pe_w = nullptr, *pe_b = nullptr, *pe_nw = nullptr, *pe_nb = nullptr;
    std::vector<CnStage> stages;
    float *patches = nullptr, *emb = nullptr, *estats = nullptr;

    float* hook_stream(int i) { return stages[i].x; }
    int64_t hook_floats(int i) const { return stages[i].T() * stages[i].width; }
};

namespace {

int dw_plan(I2VCnDwParams* p, const float* x, const float* w, const float* b, const float* add, float* y, int g, int C) {
    *p = I2VCnDwParams{};
    p->x = x; p->w = w; p->b = b; p->add = add; p->y = y; p->H = g; p->W = g; p->C = C;
#ifdef I2V_HAVE_CONVNEXT
    const int bad = k_convnext_dw_plan(p);
#else
    const int bad = eng::convnext_host::plan(p);
#endif
    if (bad) return fail("i2v_convnext_create: a %d x %d plane of %d channels does not fit the depthwise launch", g, g, C);
    return 0;
}

int dw_run(I2VCnDwParams p, int frames, hipStream_t s) {
    p.N = frames;
#ifdef I2V_HAVE_CONVNEXT
    if (k_convnext_dw(p, (i2v_stream_t)s) != 0) {
        const char* e = be_error();
        return fail("%s", e ? e : "k_convnext_dw failed");
    }
#else
    (void)s;
    if (eng::convnext_host::dw(p) != 0) return fail("convnext_host::dw: launch not planned");
#endif
    return 0;
}

int convnext_plan(i2v_convnext* n, const float* const* w, int nw, const int32_t* hooks, int n_hooks) {
    const i2v_convnext_config& c = n->cfg;
    Arena& A = n->arena;
    if (c.img <= 0 || c.patch <= 0 || c.patch % 4 != 0 || c.img % c.patch != 0 || c.in_chans <= 0 || c.dim <= 0 || c.dim % 4 != 0 ||
        c.stages <= 0 || c.stages > I2V_CONVNEXT_MAX_STAGES)
        return fail("i2v_convnext_create: unsupported configuration (img %d patch %d dim %d stages %d)", c.img, c.patch, c.dim, c.stages);
    n->gsz = c.img / c.patch;
    for (int i = 0; i < c.stages; ++i) {
        if (c.depths[i] <= 0) return fail("i2v_convnext_create: stage %d has %d blocks", i, c.depths[i]);
        if (n->gsz % (1 << i) != 0) return fail("i2v_convnext_create: the %d x %d plane of the stem does not halve %d times", n->gsz, n->gsz, i);
    }
    const int deepest = Hooks::deepest(hooks, n_hooks, c.stages, A);
    if (deepest < 0) return 1;
    n->ns = A.depth = deepest + 1;
    const int64_t F = n->max_frames, KP = (int64_t)c.in_chans * c.patch * c.patch;
    const int64_t T0 = (int64_t)n->gsz * n->gsz, D0 = c.dim, FT0 = F * T0;
    // every size of the plan in floats, in 64 bits, before the first allocation
    std::vector<int64_t> sizes = {D0 * KP, D0, D0, D0};
    int64_t acts = FT0 * KP + FT0 * D0 + 2 * FT0;                              // patches, emb, stem LN stats
    for (int i = 0; i < n->ns; ++i) {
        const int64_t D = D0 << i, FT = F * (T0 >> (2 * i));
        if (i > 0) {
            for (int64_t v : {D / 2, D / 2, 2 * D * D, D}) sizes.push_back(v);
            acts += 2 * 4 * FT;                                                 // the downsample's LN stats over the previous stage
        }
        for (int b = 0; b < c.depths[i]; ++b) {
            for (int64_t v : {49 * D, D, D, D, 4 * D * D, 4 * D, 4 * D * D, D}) sizes.push_back(v);
            acts += 49 * D + FT * D + 4 * FT * D + 2 * FT;                      // mirrored filter; u, h, stats
        }
        acts += FT * D;                                                         // the stage's stream
    }
    acts += FT0 * D0 + 4 * FT0 * D0 + FT0 * D0 + FT0 * D0;                      // shared scratch: t1, t2, t3, G (stage 0 is the largest)
    for (int i = 0; i < n_hooks; ++i) acts += F * (T0 >> (2 * hooks[i])) * (D0 << hooks[i]);
    if ((int)sizes.size() != nw) return fail("i2v_convnext_create: %d weight arrays given, %zu expected for %d stages", nw, sizes.size(), n->ns);
    int64_t total = acts;
    for (int64_t v : sizes) total += v;
    VCHK(A.plan(total, FT0));
    if (FT0 * 4 * D0 >= (1ll << 31)) return fail("i2v_convnext_create: %lld bytes needed: too many frames for one net", (long long)A.planned);
    std::vector<const float*> dev;
    VCHK(A.upload(sizes, w, dev));
    n->pe_w = dev[0]; n->pe_b = dev[1]; n->pe_nw = dev[2]; n->pe_nb = dev[3];
    if (!(n->patches = A.alloc(FT0 * KP)) || !(n->emb = A.alloc(FT0 * D0)) || !(n->estats = A.alloc(2 * FT0))) return A.oom("stem");
    if (!(n->t1 = A.alloc(FT0 * D0)) || !(n->t2 = A.alloc(4 * FT0 * D0)) || !(n->dqkv = A.alloc(FT0 * D0)) || !(n->G = A.alloc(FT0 * D0)))
        return A.oom("scratch");
    size_t wi = 4;
    n->stages.resize(n->ns);
    for (int i = 0; i < n->ns; ++i) {
        CnStage& S = n->stages[i];
        S.grid = n->gsz >> i; S.width = c.dim << i;
        const int64_t D = S.width, FT = F * S.T();
        if (i > 0) {
            S.dnw = dev[wi]; S.dnb = dev[wi + 1]; S.dlw = dev[wi + 2]; S.dlb = dev[wi + 3];
            wi += 4;
            if (!(S.dstats = A.alloc(2 * 4 * FT))) return A.oom("downsample");
        }
        if (!(S.x = A.alloc(FT * D))) return A.oom("a stage's stream");
        S.blocks.resize(c.depths[i]);
        for (int b = 0; b < c.depths[i]; ++b) {
            CnBlock& B = S.blocks[b];
            const float* const* q = &dev[wi];
            B.dww = q[0]; B.dwb = q[1]; B.nw = q[2]; B.nb = q[3]; B.fc1w = q[4]; B.fc1b = q[5]; B.fc2w = q[6]; B.fc2b = q[7];
            // the input gradient's filter: the rows of the (49, w) filter in reverse order
            std::vector<float> mir((size_t)49 * D);
            const float* hw = w[wi];
            for (int t = 0; t < 49; ++t)
                for (int64_t ch = 0; ch < D; ++ch) mir[(size_t)t * D + ch] = hw[(size_t)(48 - t) * D + ch];
            float* dm = A.alloc(49 * D);
            if (!dm) return A.oom("a mirrored filter");
            HCHK(hipMemcpy(dm, mir.data(), mir.size() * 4, hipMemcpyHostToDevice));
            B.dwm = dm;
            wi += 8;
            if (!(B.u = A.alloc(FT * D)) || !(B.h = A.alloc(4 * FT * D)) || !(B.stats = A.alloc(2 * FT)))
                return A.oom("saved activations of a block");
            VCHK(dw_plan(&B.fwd, S.x, B.dww, B.dwb, nullptr, B.u, S.grid, S.width));
        }
    }
    for (int i = 0; i < n_hooks; ++i) {
        const CnStage& S = n->stages[hooks[i]];
        VCHK(n->hooks.add(A, hooks[i], F * S.T() * S.width));
    }
    // the backward launches: dw^T(t3) + g into G, g being G itself or, for the last block of the deepest stage, its hook's gradient view
    for (int i = 0; i < n->ns; ++i) {
        CnStage& S = n->stages[i];
        for (size_t b = 0; b < S.blocks.size(); ++b) {
            const bool last = i == n->ns - 1 && b + 1 == S.blocks.size();
            const float* g = last ? n->hooks.grad_at(i) : n->G;
            VCHK(dw_plan(&S.blocks[b].bwd, n->dqkv, S.blocks[b].dwm, nullptr, g, n->G, S.grid, S.width));
        }
    }
    return 0;
}

int convnext_forward(i2v_convnext* n, const float* x, int frames, hipStream_t s) {
    const i2v_convnext_config& c = n->cfg;
    const int64_t esp = (int64_t)n->max_frames * n->gsz * n->gsz;
    VCHK(ln_stem(x, frames, c.in_chans, n->gsz, c.patch, n->pe_w, n->pe_b, n->pe_nw, n->pe_nb, c.ln_eps, c.dim, n->patches, n->emb,
                            n->estats, n->estats + esp, n->stages[0].x, s));
    for (int i = 0; i < n->ns; ++i) {
        CnStage& S = n->stages[i];
        const int D = S.width;
        const int64_t FT = frames * S.T(), sp = n->max_frames * S.T();
        if (i > 0) {        // downsample: LayerNorm per position of the previous stage, 2 x 2 gather to 4 x its width, Linear to this width
            const CnStage& P = n->stages[i - 1];
            VCHK(vit_layernorm(P.x, 4 * FT, P.width, S.dnw, S.dnb, c.ln_eps, n->t1, S.dstats, S.dstats + 4 * sp, s));
            VCHK(swin_merge_gather(n->t1, frames, P.grid, P.grid, P.width, n->t2, s));
            VCHK(linear(n->t2, (int)FT, 4 * P.width, S.dlw, S.dlb, D, nullptr, S.x, nullptr, s));
        }
        for (CnBlock& B : S.blocks) {
            VCHK(dw_run(B.fwd, frames, s));                                                   // u = dw(x) + b
            VCHK(vit_layernorm(B.u, FT, D, B.nw, B.nb, c.ln_eps, n->t1, B.stats, B.stats + sp, s));
            VCHK(linear(n->t1, (int)FT, D, B.fc1w, B.fc1b, 4 * D, nullptr, B.h, n->t2, s));   // h = fc1(LN u), t2 = gelu(h)
            VCHK(linear(n->t2, (int)FT, 4 * D, B.fc2w, B.fc2b, D, S.x, S.x, nullptr, s));     // x = x + gamma fc2(gelu(h))
        }
    }
    return 0;
}

int convnext_backward(i2v_convnext* n, float* gx, int accumulate, hipStream_t s) {
    const i2v_convnext_config& c = n->cfg;
    const int frames = n->frames;
    for (int i = n->ns - 1; i >= 0; --i) {
        CnStage& S = n->stages[i];
        const int D = S.width;
        const int64_t FT = frames * S.T(), sp = n->max_frames * S.T();
        for (int b = (int)S.blocks.size() - 1; b >= 0; --b) {
            CnBlock& B = S.blocks[b];
            // gradient of the block's output: the deepest stage's hook view for the very last block, the running gradient G otherwise
            const float* gin = (i == n->ns - 1 && b == (int)S.blocks.size() - 1) ? n->hooks.grad_at(i) : n->G;
            VCHK(linear_bwd(gin, (int)FT, D, B.fc2w, 4 * D, B.h, n->t2, s));                  // dh = (g fc2') * gelu'(h)
            VCHK(linear_bwd(n->t2, (int)FT, 4 * D, B.fc1w, D, nullptr, n->t1, s));            // d LN out
            VCHK(vit_layernorm_bwd(n->t1, B.u, B.stats, B.stats + sp, B.nw, FT, D, nullptr, nullptr, n->dqkv, s));     // du
            VCHK(dw_run(B.bwd, frames, s));                                                   // G = dw^T(du) + g
        }
        if (i > 0) {
            // G holds the gradient of this stage's input (FT rows of this width): back through the Linear, the gather and the LayerNorm,
            // plus the previous stage's own hook gradient when it has one
            const CnStage& P = n->stages[i - 1];
            VCHK(linear_bwd(n->G, (int)FT, D, S.dlw, 4 * P.width, nullptr, n->t1, s));
            VCHK(swin_merge_scatter(n->t1, frames, P.grid, P.grid, P.width, nullptr, n->dqkv, s));
            VCHK(vit_layernorm_bwd(n->dqkv, P.x, S.dstats, S.dstats + 4 * sp, S.dnw, 4 * FT, P.width, n->hooks.grad_at(i - 1), nullptr, n->G, s));
        }
    }
    const int64_t esp = (int64_t)n->max_frames * n->gsz * n->gsz;
    return ln_stem_bwd(n->G, frames, c.in_chans, n->gsz, c.patch, n->pe_w, n->pe_nw, c.dim, n->emb, n->estats, n->estats + esp,
                                  n->t1, n->patches, gx, accumulate, s);
}

}  // namespace

extern "C" int i2v_convnext_create(int device, const i2v_convnext_config* cfg, const float* const* weights, int n_weights,
                                   const int32_t* hook_stages, int n_hooks, int max_frames, i2v_convnext_handle* out) {
    return xf_create("i2v_convnext_create", "stage", device, cfg, weights, hook_stages, max_frames, out, [&](i2v_convnext* n) {
        n->cfg = *cfg;
        return convnext_plan(n, weights, n_weights, hook_stages, n_hooks);
    });
}

extern "C" int i2v_convnext_destroy(i2v_convnext_handle net) { return xf_destroy(net); }

extern "C" int64_t i2v_convnext_workspace_bytes(i2v_convnext_handle net) { return xf_workspace_bytes(net); }

extern "C" int i2v_convnext_forward(i2v_convnext_handle n, const float* x, int frames, void* stream) {
    return xf_forward("i2v_convnext_forward", n, x, frames, stream, convnext_forward);
}

extern "C" int i2v_convnext_backward(i2v_convnext_handle n, float* gx, int accumulate, void* stream) {
    return xf_backward("i2v_convnext_backward", n, gx, accumulate, stream, convnext_backward);
}

extern "C" int i2v_convnext_hook_info(i2v_convnext_handle n, int hook, float** act, int64_t* act_stride, float** grad, int64_t* grad_stride,
                                      int64_t* D) {
    return xf_hook_info("i2v_convnext_hook_info", n, hook, act, act_stride, grad, grad_stride, D);
}

extern "C" int i2v_convnext_read_hook(i2v_convnext_handle n, int hook, int which, float* out, int frames, void* stream) {
    return xf_read_hook("i2v_convnext_read_hook", n, hook, which, out, frames, stream);
}
