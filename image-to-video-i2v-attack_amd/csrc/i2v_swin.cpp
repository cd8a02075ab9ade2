// Planner and executor of the Swin surrogates (include/i2v_swin.h): one arena per (net, max frames), the forward as a fixed launch
// sequence up to the deepest hooked stage, and the input-gradient pass -- no weight gradients, as the CNN and ViT paths.  The arena, the
// hook list, the seven entries' guards, the LayerNorm stem and the pre-norm block are those of i2v_xf.h; this file brings the stages with
// their window attention step and patch merging, and the Swin sizes.  The window attention and patch-merging kernels are in
// i2v_swin.hip; the linear layers, LayerNorms and patch rows are the ViT kernels.
#include "../../include/i2v_swin.h"
#include "i2v_swin_kernels.h"
#include "i2v_xf.h"

namespace {

struct Stage {
    int grid = 0, width = 0, heads = 0, ws = 0;
    std::vector<Block> blocks;
    float* out = nullptr;                    // stream after the last block: the hooked feature
    // the patch merging behind the stage (when a deeper stage runs)
    const float *mnw = nullptr, *mnb = nullptr, *mred = nullptr;
    float *mg = nullptr, *mstats = nullptr;  // saved: the gathered rows (F, grid^2 / 4, 4 width), their LN stats
    int64_t T() const { return (int64_t)grid * grid; }
    float* stream_after(size_t b) { return b + 1 < blocks.size() ? blocks[b + 1].x : out; }
};

}  // namespace

struct i2v_swin : XfNet {
    i2v_swin_config cfg{};
    int ns = 0, gsz = 0;
    const float *pe_w = nullptr, *pe_b = nullptr, *pe_nw = nullptr, *pe_nb = nullptr;
    std::vector<Stage> stages;
    float *patches = nullptr, *emb = nullptr, *estats = nullptr;

    float* hook_stream(int i) { return stages[i].out; }
    int64_t hook_floats(int i) const { return stages[i].T() * stages[i].width; }
    BlockRun run(const Stage& S, int frames, hipStream_t s) const {
        return {frames, (int)S.T(), S.width, 4 * S.width, max_frames * S.T(), cfg.ln_eps, t1, t2, dqkv, G, s};
    }
};

namespace {

int swin_plan(i2v_swin* n, const float* const* w, int nw, const int32_t* hooks, int n_hooks) {
    const i2v_swin_config& c = n->cfg;
    Arena& A = n->arena;
    if (c.img <= 0 || c.patch <= 0 || c.patch % 4 != 0 || c.img % c.patch != 0 || c.in_chans <= 0 || c.dim <= 0 || c.dim % 4 != 0 ||
        c.stages <= 0 || c.stages > I2V_SWIN_MAX_STAGES || !(c.window == 7 || c.window == 4))
        return fail("i2v_swin_create: unsupported configuration (img %d patch %d dim %d window %d stages %d)", c.img, c.patch, c.dim, c.window,
                    c.stages);
    const int dh = c.window == 7 ? 32 : 16;
    n->gsz = c.img / c.patch;
    for (int i = 0; i < c.stages; ++i) {
        const int width = c.dim << i;
        if (c.depths[i] <= 0 || c.heads[i] <= 0 || c.heads[i] * dh != width)
            return fail("i2v_swin_create: stage %d has %d blocks and %d heads at width %d (head width %d with window %d)", i, c.depths[i],
                        c.heads[i], width, dh, c.window);
        if (n->gsz % (1 << i) != 0 || (n->gsz >> i) % c.window != 0)
            return fail("i2v_swin_create: the %d x %d grid of stage %d is not a whole number of %d x %d windows", n->gsz >> i, n->gsz >> i, i,
                        c.window, c.window);
    }
    const int deepest = Hooks::deepest(hooks, n_hooks, c.stages, A);
    if (deepest < 0) return 1;
    n->ns = A.depth = deepest + 1;
    const int64_t F = n->max_frames, KP = (int64_t)c.in_chans * c.patch * c.patch, NI = (int64_t)(2 * c.window - 1) * (2 * c.window - 1);
    const int64_t T0 = (int64_t)n->gsz * n->gsz, D0 = c.dim;
    // every size of the plan in floats, in 64 bits, before the first allocation
    std::vector<int64_t> sizes = {D0 * KP, D0, D0, D0};
    int64_t acts = F * T0 * KP + F * T0 * D0 + 2 * F * T0;                     // patches, emb, embedding LN stats
    for (int i = 0; i < n->ns; ++i) {
        const int64_t D = D0 << i, FT = F * (T0 >> (2 * i));
        for (int b = 0; b < c.depths[i]; ++b) {
            for (int64_t v : {D, D, 3 * D * D, 3 * D, NI * c.heads[i], D * D, D, D, D, 4 * D * D, 4 * D, 4 * D * D, D}) sizes.push_back(v);
            acts += FT * D + 3 * FT * D + FT * D + 4 * FT * D + 4 * FT;         // x, qkv, y, h, stats
        }
        acts += FT * D;                                                         // the stage's output stream
        if (i + 1 < n->ns) {
            for (int64_t v : {4 * D, 4 * D, 8 * D * D}) sizes.push_back(v);
            acts += FT * D + 2 * (FT / 4);                                      // gathered rows, their LN stats
        }
    }
    const int64_t FT0 = F * T0;
    acts += FT0 * D0 + 4 * FT0 * D0 + 3 * FT0 * D0 + FT0 * D0;                  // shared scratch: t1, t2, dqkv, G (stage 0 is the largest)
    for (int i = 0; i < n_hooks; ++i) acts += F * (T0 >> (2 * hooks[i])) * (D0 << hooks[i]);
    if ((int)sizes.size() != nw) return fail("i2v_swin_create: %d weight arrays given, %zu expected for %d stages", nw, sizes.size(), n->ns);
    int64_t total = acts;
    for (int64_t v : sizes) total += v;
    VCHK(A.plan(total, FT0));
    std::vector<const float*> dev;
    VCHK(A.upload(sizes, w, dev));
    n->pe_w = dev[0]; n->pe_b = dev[1]; n->pe_nw = dev[2]; n->pe_nb = dev[3];
    if (!(n->patches = A.alloc(F * T0 * KP)) || !(n->emb = A.alloc(F * T0 * D0)) || !(n->estats = A.alloc(2 * F * T0)))
        return A.oom("embedding");
    size_t wi = 4;
    n->stages.resize(n->ns);
    for (int i = 0; i < n->ns; ++i) {
        Stage& S = n->stages[i];
        S.grid = n->gsz >> i; S.width = c.dim << i; S.heads = c.heads[i];
        S.ws = c.window;
        const int64_t D = S.width, FT = F * S.T();
        S.blocks.resize(c.depths[i]);
        for (int b = 0; b < c.depths[i]; ++b) {
            Block& B = S.blocks[b];
            const float* const* q = &dev[wi];
            B.weights(q, q + 5);                                   // the bias table sits behind qkv's bias
            B.table = q[4];
            wi += 13;
            B.shift = (b % 2 == 1 && S.grid > S.ws) ? S.ws / 2 : 0;
            if (!(B.x = A.alloc(FT * D)) || !(B.qkv = A.alloc(3 * FT * D)) || !(B.y = A.alloc(FT * D)) || !(B.h = A.alloc(4 * FT * D)) ||
                !(B.stats = A.alloc(4 * FT)))
                return A.oom("saved activations of a block");
        }
        if (!(S.out = A.alloc(FT * D))) return A.oom("a stage's output");
        if (i + 1 < n->ns) {
            S.mnw = dev[wi]; S.mnb = dev[wi + 1]; S.mred = dev[wi + 2];
            wi += 3;
            if (!(S.mg = A.alloc(FT * D)) || !(S.mstats = A.alloc(2 * (FT / 4)))) return A.oom("patch merging");
        }
    }
    if (!(n->t1 = A.alloc(FT0 * D0)) || !(n->t2 = A.alloc(4 * FT0 * D0)) || !(n->dqkv = A.alloc(3 * FT0 * D0)) || !(n->G = A.alloc(FT0 * D0)))
        return A.oom("scratch");
    for (int i = 0; i < n_hooks; ++i) {
        const Stage& S = n->stages[hooks[i]];
        VCHK(n->hooks.add(A, hooks[i], F * S.T() * S.width));
    }
    return 0;
}

int swin_forward(i2v_swin* n, const float* x, int frames, hipStream_t s) {
    const i2v_swin_config& c = n->cfg;
    const int64_t esp = (int64_t)n->max_frames * n->gsz * n->gsz;
    VCHK(ln_stem(x, frames, c.in_chans, n->gsz, c.patch, n->pe_w, n->pe_b, n->pe_nw, n->pe_nb, c.ln_eps, c.dim, n->patches, n->emb, n->estats,
               n->estats + esp, n->stages[0].blocks[0].x, s));
    for (int i = 0; i < n->ns; ++i) {
        Stage& S = n->stages[i];
        const int D = S.width, g = S.grid, dh = D / S.heads;
        const BlockRun r = n->run(S, frames, s);
        for (size_t b = 0; b < S.blocks.size(); ++b)
            VCHK(block_forward(S.blocks[b], r, S.stream_after(b), [&](const Block& B, float* o) {
                return swin_window_attention(B.qkv, frames, g, g, S.ws, B.shift, S.heads, dh, B.table, o, s);
            }));
        if (i + 1 < n->ns) {                                       // patch merging: gather, LayerNorm over 4 width, reduce to 2 width
            const int64_t FT = frames * S.T();
            VCHK(swin_merge_gather(S.out, frames, g, g, D, S.mg, s));
            VCHK(vit_layernorm(S.mg, FT / 4, 4 * D, S.mnw, S.mnb, c.ln_eps, n->t1, S.mstats, S.mstats + r.sp / 4, s));
            VCHK(linear(n->t1, (int)FT / 4, 4 * D, S.mred, nullptr, 2 * D, nullptr, n->stages[i + 1].blocks[0].x, nullptr, s));
        }
    }
    return 0;
}

int swin_backward(i2v_swin* n, float* gx, int accumulate, hipStream_t s) {
    const i2v_swin_config& c = n->cfg;
    const int frames = n->frames;
    for (int i = n->ns - 1; i >= 0; --i) {
        Stage& S = n->stages[i];
        const int D = S.width, g = S.grid, dh = D / S.heads;
        const BlockRun r = n->run(S, frames, s);
        if (i + 1 < n->ns) {
            // G holds the gradient of the next stage's input (FT / 4 rows of 2 width): back through the reduction, the LayerNorm and the
            // gather, plus this stage's own hook gradient when it has one
            const int64_t FT = frames * S.T();
            VCHK(linear_bwd(n->G, (int)FT / 4, 2 * D, S.mred, 4 * D, nullptr, n->t1, s));
            VCHK(vit_layernorm_bwd(n->t1, S.mg, S.mstats, S.mstats + r.sp / 4, S.mnw, FT / 4, 4 * D, nullptr, nullptr, n->dqkv, s));
            VCHK(swin_merge_scatter(n->dqkv, frames, g, g, D, n->hooks.grad_at(i), n->G, s));
        }
        for (int b = (int)S.blocks.size() - 1; b >= 0; --b) {
            // gradient of the stream after block b: the deepest stage's hook view for the very last block, the running gradient G otherwise
            const float* gin = (i == n->ns - 1 && b == (int)S.blocks.size() - 1) ? n->hooks.grad_at(i) : n->G;
            VCHK(block_backward(S.blocks[b], r, gin, nullptr, [&](const Block& B, const float* dout) {
                return swin_window_attention_bwd(B.qkv, dout, frames, g, g, S.ws, B.shift, S.heads, dh, B.table, n->dqkv, s);
            }));
        }
    }
    const int64_t esp = (int64_t)n->max_frames * n->gsz * n->gsz;
    return ln_stem_bwd(n->G, frames, c.in_chans, n->gsz, c.patch, n->pe_w, n->pe_nw, c.dim, n->emb, n->estats, n->estats + esp, n->t1, n->patches,
                     gx, accumulate, s);
}

}  // namespace

extern "C" int i2v_swin_create(int device, const i2v_swin_config* cfg, const float* const* weights, int n_weights, const int32_t* hook_stages,
                               int n_hooks, int max_frames, i2v_swin_handle* out) {
    return xf_create("i2v_swin_create", "stage", device, cfg, weights, hook_stages, max_frames, out, [&](i2v_swin* n) {
        n->cfg = *cfg;
        return swin_plan(n, weights, n_weights, hook_stages, n_hooks);
    });
}

extern "C" int i2v_swin_destroy(i2v_swin_handle net) { return xf_destroy(net); }

extern "C" int64_t i2v_swin_workspace_bytes(i2v_swin_handle net) { return xf_workspace_bytes(net); }

extern "C" int i2v_swin_forward(i2v_swin_handle n, const float* x, int frames, void* stream) {
    return xf_forward("i2v_swin_forward", n, x, frames, stream, swin_forward);
}

extern "C" int i2v_swin_backward(i2v_swin_handle n, float* gx, int accumulate, void* stream) {
    return xf_backward("i2v_swin_backward", n, gx, accumulate, stream, swin_backward);
}

extern "C" int i2v_swin_hook_info(i2v_swin_handle n, int hook, float** act, int64_t* act_stride, float** grad, int64_t* grad_stride, int64_t* D) {
    return xf_hook_info("i2v_swin_hook_info", n, hook, act, act_stride, grad, grad_stride, D);
}

extern "C" int i2v_swin_read_hook(i2v_swin_handle n, int hook, int which, float* out, int frames, void* stream) {
    return xf_read_hook("i2v_swin_read_hook", n, hook, which, out, frames, stream);
}

// ---- the kernels on their own ----
extern "C" int i2v_swin_window_attention_f32(const float* qkv, int frames, int H, int W, int window, int shift, int heads, int dh,
                                             const float* table, float* out, void* stream) {
    return swin_window_attention(qkv, frames, H, W, window, shift, heads, dh, table, out, (hipStream_t)stream);
}
extern "C" int i2v_swin_window_attention_bwd_f32(const float* qkv, const float* dout, int frames, int H, int W, int window, int shift,
                                                 int heads, int dh, const float* table, float* dqkv, void* stream) {
    return swin_window_attention_bwd(qkv, dout, frames, H, W, window, shift, heads, dh, table, dqkv, (hipStream_t)stream);
}
extern "C" int i2v_swin_merge_f32(const float* x, int frames, int H, int W, int C, float* out, void* stream) {
    return swin_merge_gather(x, frames, H, W, C, out, (hipStream_t)stream);
}
extern "C" int i2v_swin_merge_bwd_f32(const float* dout, int frames, int H, int W, int C, float* dx, int accumulate, void* stream) {
    return swin_merge_scatter(dout, frames, H, W, C, accumulate ? dx : nullptr, dx, (hipStream_t)stream);
}
extern "C" int i2v_swin_embed_f32(const float* img, int frames, int in_chans, int g, int patch, const float* W, const float* b,
                                  const float* norm_w, const float* norm_b, float eps, int dim, float* patches, float* emb, float* mean,
                                  float* rstd, float* tokens, void* stream) {
    return ln_stem(img, frames, in_chans, g, patch, W, b, norm_w, norm_b, eps, dim, patches, emb, mean, rstd, tokens, (hipStream_t)stream);
}
extern "C" int i2v_swin_embed_bwd_f32(const float* dtokens, int frames, int in_chans, int g, int patch, const float* W, const float* norm_w,
                                      int dim, const float* emb, const float* mean, const float* rstd, float* demb, float* patches,
                                      float* gimg, int accumulate, void* stream) {
    return ln_stem_bwd(dtokens, frames, in_chans, g, patch, W, norm_w, dim, emb, mean, rstd, demb, patches, gimg, accumulate, (hipStream_t)stream);
}
