// Planner and executor of the CoaT-Lite surrogates (include/i2v_coat.h) on the transformer stack: one arena per (net, max frames), the
// forward as a fixed launch sequence up to the deepest hooked stage, and the input-gradient pass -- no weight gradients.  A serial
// block is the shared pre-norm block of i2v_xf.h (block_forward / block_backward as they are) behind the stage's cpe; this file brings
// the patch embeddings behind a class row, the sizes, and the attention step: coat_dwmix (crpe) and coat_attention (i2v_coat.hip;
// without -DI2V_HAVE_COAT the scalar restatement i2v_coat_host.h).
//   stage 0     ln_stem (4 x 4 patches, Linear, LayerNorm) | U = [cls; tokens]                                  (vit_assemble, a table of zeros)
//   stage k     rows = the 2 x 2 cells of the grid rows behind the class row (coat_cell_gather) | Linear | LayerNorm | U = [cls; tokens]
//   block       B.x = cpe(U) (coat_dwmix, residual) | the shared block, its attention step:
//               E = crpe(v) read in place out of qkv (coat_dwmix) | out = FA(qkv, E) with G and the column statistics kept |
//               the block writes U again, the last one of a stage the stage's output
//   backward    the same in reverse: per block the shared backward leaves d B.x in G, cpe's transpose writes G2, the next block below
//               reads G2; the attention step: coat_attention_bwd, then crpe's transpose of dE ACCUMULATED onto dv; at a stage's foot
//               the class row is stripped (coat_cell_gather, s = 1), LayerNorm and Linear backward, and the cells are scattered into
//               G2 -- onto a copy of the hook's gradient when the stage below is hooked
// saved per block: x, qkv, y, h, four LayerNorm statistics per token, E (F, T, D), G (F, H, dh, dh) and the column statistics
// (F, H, 2, dh): no token-by-anything matrix.  Per stage: the embedding before its LayerNorm with two statistics per grid token, and the
// stream behind its last block.
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>

#include "../../include/i2v_coat.h"
#include "i2v_xf.h"
#ifdef I2V_HAVE_COAT
#include "i2v_coat_kernels.h"
#else
#include "i2v_coat_host.h"      // (the host simulation's one-file build: the launches as scalar code)
#endif

namespace {

struct CoatBlock : Block {
    int stage = 0;
    float *E = nullptr, *gram = nullptr, *kstat = nullptr;
};

struct CoatStage {
    int grid = 0, width = 0, dh = 0, T = 0, mlp = 0, first = 0, count = 0, kp = 0;      // kp: columns of a patch row
    const float *pw = nullptr, *pb = nullptr, *nw = nullptr, *nb = nullptr, *cls = nullptr, *zeros = nullptr;
    const float *cpw = nullptr, *cpb = nullptr, *w3 = nullptr, *w5 = nullptr, *w7 = nullptr, *cb = nullptr;
    float *emb = nullptr, *mean = nullptr, *rstd = nullptr, *out = nullptr;
};

}  // namespace

struct i2v_coat : XfNet {
    i2v_coat_config cfg{};
    int ns = 0, nb = 0;
    std::vector<CoatStage> stages;
    std::vector<CoatBlock> blocks;
    float *G2 = nullptr, *U = nullptr, *dE = nullptr, *patches = nullptr, *dgram = nullptr;

    float* hook_stream(int k) { return stages[k].out; }
    int64_t hook_floats(int k) const { return (int64_t)stages[k].T * stages[k].width; }
    BlockRun run(const CoatStage& S, int frames, hipStream_t s) const {
        return {frames, S.T, S.width, S.mlp, (int64_t)max_frames * S.T, cfg.ln_eps, t1, t2, dqkv, G, s};
    }
    CoatDw cpe(const CoatStage& S, int frames, const float* x, float* y) const {
        CoatDw d{};
        d.x = x; d.y = y; d.w3 = S.cpw; d.b = S.cpb; d.F = frames; d.g = S.grid; d.C = S.width; d.n3 = S.width; d.prefix = 1; d.residual = 1;
        d.xrs = d.yrs = S.width;
        return d;
    }
    CoatDw crpe(const CoatStage& S, int frames) const {
        CoatDw d{};
        d.w3 = S.w3; d.w5 = S.w5; d.w7 = S.w7; d.b = S.cb; d.F = frames; d.g = S.grid; d.C = S.width;
        d.n3 = cfg.win3 * S.dh; d.n5 = cfg.win5 * S.dh; d.prefix = 1;
        return d;
    }
    CoatAttn attn(const CoatBlock& B, int frames) const {
        const CoatStage& S = stages[B.stage];
        CoatAttn a{};
        a.qkv = B.qkv; a.E = B.E; a.F = frames; a.T = S.T; a.H = cfg.heads; a.dh = S.dh; a.scale = 1.f / sqrtf((float)S.dh);
        a.gram = B.gram; a.kstat = B.kstat;
        return a;
    }
};

namespace {

int coat_plan(i2v_coat* n, const float* const* w, int nw, const int32_t* hooks, int n_hooks) {
    const i2v_coat_config& c = n->cfg;
    Arena& A = n->arena;
    if (c.img <= 0 || c.img % 32 != 0 || c.in_chans <= 0 || (c.in_chans * 16) % 4 != 0)
        return fail("i2v_coat_create: unsupported configuration (img %d: a multiple of 32; %d input channels)", c.img, c.in_chans);
    if (c.heads <= 0 || c.win3 <= 0 || c.win5 <= 0 || c.win7 <= 0 || c.win3 + c.win5 + c.win7 != c.heads)
        return fail("i2v_coat_create: window head counts %d / %d / %d are positive and sum to the %d heads", c.win3, c.win5, c.win7, c.heads);
    for (int k = 0; k < I2V_COAT_STAGES; ++k) {
        const int D = c.dims[k];
        if (D <= 0 || D % c.heads != 0 || (D / c.heads) % 4 != 0 || c.depths[k] <= 0 || c.mlp_ratios[k] <= 0)
            return fail("i2v_coat_create: stage %d has width %d, %d heads, %d blocks and MLP ratio %d", k, D, c.heads, c.depths[k], c.mlp_ratios[k]);
        if (D / c.heads > COAT_MAX_DH) return fail("i2v_coat_create: heads of width %d in stage %d: up to %d", D / c.heads, k, (int)COAT_MAX_DH);
    }
    const int deepest = Hooks::deepest(hooks, n_hooks, I2V_COAT_STAGES, A);
    if (deepest < 0) return 1;
    n->ns = A.depth = deepest + 1;
    const int64_t F = n->max_frames;
    // the stages that run, and every size of the plan in floats, in 64 bits, before the first allocation
    n->stages.clear();
    n->nb = 0;
    for (int k = 0, g = c.img / 4; k < n->ns; ++k, g /= 2) {
        CoatStage S;
        S.grid = g; S.width = c.dims[k]; S.dh = S.width / c.heads; S.T = 1 + g * g; S.mlp = c.mlp_ratios[k] * S.width;
        S.first = n->nb; S.count = c.depths[k]; S.kp = k ? 4 * c.dims[k - 1] : c.in_chans * 16;
        n->stages.push_back(S);
        n->nb += S.count;
    }
    std::vector<int64_t> sizes;
    int64_t acts = 0, mFTD = 0, mMlp = 0, mRows = 0, mGram = 0;
    for (int k = 0; k < n->ns; ++k) {
        const CoatStage& S = n->stages[k];
        const int64_t D = S.width, FT = F * S.T, np = (int64_t)S.grid * S.grid, dh = S.dh, M = S.mlp;
        for (int64_t v : {D * S.kp, D, D, D, D, S.T * D, 9 * D, D, 9 * c.win3 * dh, 25 * c.win5 * dh, 49 * c.win7 * dh, D}) sizes.push_back(v);
        for (int b = 0; b < S.count; ++b) {
            for (int64_t v : {D, D, 3 * D * D, 3 * D, D * D, D, D, D, M * D, M, D * M, D}) sizes.push_back(v);
            acts += FT * D + 3 * FT * D + FT * D + FT * M + 4 * FT + FT * D + F * D * dh + 2 * F * D;      // x, qkv, y, h, statistics, E, G, kstat
        }
        acts += F * np * D + 2 * F * np + FT * D;                            // the embedding, its statistics, the stream behind the stage
        mFTD = std::max(mFTD, FT * D); mMlp = std::max(mMlp, FT * M); mRows = std::max(mRows, F * np * S.kp); mGram = std::max(mGram, F * D * dh);
    }
    acts += 5 * mFTD + mMlp + 3 * mFTD + mRows + mGram;                      // t1, G, G2, U, dE; t2; dqkv; the patch rows; dG
    for (int i = 0; i < n_hooks; ++i) acts += F * n->stages[hooks[i]].T * n->stages[hooks[i]].width;
    if ((int)sizes.size() != nw) return fail("i2v_coat_create: %d weight arrays given, %zu expected for %d stages", nw, sizes.size(), n->ns);
    int64_t total = acts;
    for (int64_t v : sizes) total += v;
    VCHK(A.plan(total, F * n->stages[0].T));
    if (3 * mFTD >= (1ll << 31) || mMlp >= (1ll << 31) || mRows >= (1ll << 31) || F > 65535)
        return fail("i2v_coat_create: %lld bytes needed: too many frames for one net", (long long)A.planned);
    std::vector<const float*> dev;
    VCHK(A.upload(sizes, w, dev));
    size_t wi = 0;
    n->blocks.resize(n->nb);
    for (int k = 0; k < n->ns; ++k) {
        CoatStage& S = n->stages[k];
        const int64_t D = S.width, FT = F * S.T, np = (int64_t)S.grid * S.grid;
        S.pw = dev[wi]; S.pb = dev[wi + 1]; S.nw = dev[wi + 2]; S.nb = dev[wi + 3]; S.cls = dev[wi + 4]; S.zeros = dev[wi + 5];
        S.cpw = dev[wi + 6]; S.cpb = dev[wi + 7]; S.w3 = dev[wi + 8]; S.w5 = dev[wi + 9]; S.w7 = dev[wi + 10]; S.cb = dev[wi + 11];
        wi += 12;
        for (int b = 0; b < S.count; ++b) {
            CoatBlock& B = n->blocks[S.first + b];
            B.stage = k;
            B.weights(&dev[wi], &dev[wi + 4]);
            wi += 12;
            VCHK(B.alloc_saves(A, FT, D, S.mlp, 0));
            if (!(B.E = A.alloc(FT * D)) || !(B.gram = A.alloc(F * D * S.dh)) || !(B.kstat = A.alloc(2 * F * D))) return A.oom("saved attention of a block");
        }
        if (!(S.emb = A.alloc(F * np * D)) || !(S.mean = A.alloc(F * np)) || !(S.rstd = A.alloc(F * np)) || !(S.out = A.alloc(FT * D)))
            return A.oom("a stage's embedding and output");
    }
    if (!(n->t1 = A.alloc(mFTD)) || !(n->G = A.alloc(mFTD)) || !(n->G2 = A.alloc(mFTD)) || !(n->U = A.alloc(mFTD)) || !(n->dE = A.alloc(mFTD)) ||
        !(n->t2 = A.alloc(mMlp)) || !(n->dqkv = A.alloc(3 * mFTD)) || !(n->patches = A.alloc(mRows)) || !(n->dgram = A.alloc(mGram)))
        return A.oom("scratch");
    for (int i = 0; i < n_hooks; ++i) VCHK(n->hooks.add(A, hooks[i], F * n->hook_floats(hooks[i])));
    return 0;
}

int coat_forward(i2v_coat* n, const float* x, int frames, hipStream_t s) {
    const i2v_coat_config& c = n->cfg;
    for (int k = 0; k < n->ns; ++k) {
        const CoatStage& S = n->stages[k];
        const int np = S.grid * S.grid;
        if (k == 0) {
            VCHK(ln_stem(x, frames, c.in_chans, S.grid, 4, S.pw, S.pb, S.nw, S.nb, c.ln_eps, S.width, n->patches, S.emb, S.mean, S.rstd, n->t1, s));
        } else {
            const CoatStage& P = n->stages[k - 1];
            CoatCells q{P.out, n->patches, frames, P.grid, P.width, 2, 1, 0};
            VCHK(coat_cell_gather(q, s));
            VCHK(linear(n->patches, frames * np, S.kp, S.pw, S.pb, S.width, nullptr, S.emb, nullptr, s));
            VCHK(vit_layernorm(S.emb, (int64_t)frames * np, S.width, S.nw, S.nb, c.ln_eps, n->t1, S.mean, S.rstd, s));
        }
        VCHK(vit_assemble(n->t1, S.cls, 1, S.zeros, n->U, frames, S.T, S.width, s));
        const BlockRun r = n->run(S, frames, s);
        for (int b = 0; b < S.count; ++b) {
            const CoatBlock& B = n->blocks[S.first + b];
            VCHK(coat_dwmix(n->cpe(S, frames, n->U, B.x), s));
            VCHK(block_forward(B, r, b + 1 < S.count ? n->U : S.out, [&](const Block&, float* o) {
                CoatDw e = n->crpe(S, frames);                                // E = crpe(v), v read in place out of qkv; the class row 0
                e.x = B.qkv + 2 * S.width; e.xrs = 3 * S.width; e.y = B.E; e.yrs = S.width;
                VCHK(coat_dwmix(e, s));
                CoatAttn a = n->attn(B, frames);
                a.out = o;
                return coat_attention(a, s);
            }));
        }
    }
    return 0;
}

int coat_backward(i2v_coat* n, float* gx, int accumulate, hipStream_t s) {
    const i2v_coat_config& c = n->cfg;
    const int frames = n->frames;
    for (int k = n->ns - 1; k >= 0; --k) {
        const CoatStage& S = n->stages[k];
        const BlockRun r = n->run(S, frames, s);
        const int np = S.grid * S.grid;
        for (int b = S.count - 1; b >= 0; --b) {
            const CoatBlock& B = n->blocks[S.first + b];
            // gradient of the stream behind the block: the deepest stage's hook view at the top; below it G2, which cpe's transpose of
            // the block above or the patch embedding's backward of the stage above (the hook there added) has left
            const float* gin = k == n->ns - 1 && b == S.count - 1 ? n->hooks.grad_at(k) : n->G2;
            VCHK(block_backward(B, r, gin, nullptr, [&](const Block&, const float* dout) {
                CoatAttn a = n->attn(B, frames);
                a.dout = dout; a.dgram = n->dgram; a.dqkv = n->dqkv; a.dE = n->dE;
                VCHK(coat_attention_bwd(a, s));
                CoatDw e = n->crpe(S, frames);                                // dv += crpe^T dE
                e.x = n->dE; e.xrs = S.width; e.y = n->dqkv + 2 * S.width; e.yrs = 3 * S.width; e.accumulate = 1;
                return coat_dwmix_bwd(e, s);
            }));
            VCHK(coat_dwmix_bwd(n->cpe(S, frames, n->G, n->G2), s));
        }
        // G2: gradient of [cls; tokens].  The class row is a parameter's; the grid rows go back through the LayerNorm and the Linear
        CoatCells strip{n->G2, n->t1, frames, S.grid, S.width, 1, 1, 0};
        VCHK(coat_cell_gather(strip, s));
        if (k == 0)
            return ln_stem_bwd(n->t1, frames, c.in_chans, S.grid, 4, S.pw, S.nw, S.width, S.emb, S.mean, S.rstd, n->t2, n->patches, gx, accumulate, s);
        const CoatStage& P = n->stages[k - 1];
        VCHK(vit_layernorm_bwd(n->t1, S.emb, S.mean, S.rstd, S.nw, (int64_t)frames * np, S.width, nullptr, nullptr, n->t2, s));
        VCHK(linear_bwd(n->t2, frames * np, S.width, S.pw, S.kp, nullptr, n->patches, s));
        const float* hook = n->hooks.grad_at(k - 1);
        if (hook) HCHK(hipMemcpyAsync(n->G2, hook, (size_t)frames * P.T * P.width * 4, hipMemcpyDeviceToDevice, s));
        CoatCells q{n->patches, n->G2, frames, P.grid, P.width, 2, 1, hook != nullptr};
        VCHK(coat_cell_scatter(q, s));
    }
    return 0;
}

}  // namespace

extern "C" int i2v_coat_create(int device, const i2v_coat_config* cfg, const float* const* weights, int n_weights, const int32_t* hook_stages,
                               int n_hooks, int max_frames, i2v_coat_handle* out) {
    return xf_create("i2v_coat_create", "stage", device, cfg, weights, hook_stages, max_frames, out, [&](i2v_coat* n) {
        n->cfg = *cfg;
        return coat_plan(n, weights, n_weights, hook_stages, n_hooks);
    });
}

extern "C" int i2v_coat_destroy(i2v_coat_handle net) { return xf_destroy(net); }

extern "C" int64_t i2v_coat_workspace_bytes(i2v_coat_handle net) { return xf_workspace_bytes(net); }

extern "C" int i2v_coat_forward(i2v_coat_handle n, const float* x, int frames, void* stream) {
    return xf_forward("i2v_coat_forward", n, x, frames, stream, coat_forward);
}

extern "C" int i2v_coat_backward(i2v_coat_handle n, float* gx, int accumulate, void* stream) {
    return xf_backward("i2v_coat_backward", n, gx, accumulate, stream, coat_backward);
}

extern "C" int i2v_coat_hook_info(i2v_coat_handle n, int hook, float** act, int64_t* act_stride, float** grad, int64_t* grad_stride, int64_t* D) {
    return xf_hook_info("i2v_coat_hook_info", n, hook, act, act_stride, grad, grad_stride, D);
}

extern "C" int i2v_coat_read_hook(i2v_coat_handle n, int hook, int which, float* out, int frames, void* stream) {
    return xf_read_hook("i2v_coat_read_hook", n, hook, which, out, frames, stream);
}

// ---- the kernels on their own ----
extern "C" int i2v_coat_factor_attention_f32(const float* qkv, const float* E, int frames, int T, int heads, int dh, float scale, float* gram,
                                             float* kstat, float* out, void* stream) {
    CoatAttn a{};
    a.qkv = qkv; a.E = E; a.F = frames; a.T = T; a.H = heads; a.dh = dh; a.scale = scale; a.gram = gram; a.kstat = kstat; a.out = out;
    return coat_attention(a, (hipStream_t)stream);
}

extern "C" int i2v_coat_factor_attention_bwd_f32(const float* qkv, const float* E, const float* gram, const float* kstat, const float* dout,
                                                 int frames, int T, int heads, int dh, float scale, float* dgram, float* dqkv, float* dE,
                                                 void* stream) {
    CoatAttn a{};
    a.qkv = qkv; a.E = E; a.F = frames; a.T = T; a.H = heads; a.dh = dh; a.scale = scale;
    a.gram = const_cast<float*>(gram); a.kstat = const_cast<float*>(kstat);      // (read only by the backward)
    a.dout = dout; a.dgram = dgram; a.dqkv = dqkv; a.dE = dE;
    return coat_attention_bwd(a, (hipStream_t)stream);
}

extern "C" int i2v_coat_dwmix_f32(const float* x, int64_t x_rs, const float* w3, const float* w5, const float* w7, const float* bias, int frames,
                                  int g, int C, int n3, int n5, int prefix, int residual, float* y, int64_t y_rs, void* stream) {
    CoatDw d{};
    d.x = x; d.w3 = w3; d.w5 = w5; d.w7 = w7; d.b = bias; d.y = y; d.F = frames; d.g = g; d.C = C; d.n3 = n3; d.n5 = n5; d.prefix = prefix;
    d.residual = residual != 0; d.xrs = x_rs; d.yrs = y_rs;
    return coat_dwmix(d, (hipStream_t)stream);
}

extern "C" int i2v_coat_dwmix_bwd_f32(const float* dy, int64_t dy_rs, const float* w3, const float* w5, const float* w7, int frames, int g, int C,
                                      int n3, int n5, int prefix, int residual, int accumulate, float* dx, int64_t dx_rs, void* stream) {
    CoatDw d{};
    d.x = dy; d.w3 = w3; d.w5 = w5; d.w7 = w7; d.y = dx; d.F = frames; d.g = g; d.C = C; d.n3 = n3; d.n5 = n5; d.prefix = prefix;
    d.residual = residual != 0; d.accumulate = accumulate != 0; d.xrs = dy_rs; d.yrs = dx_rs;
    return coat_dwmix_bwd(d, (hipStream_t)stream);
}

extern "C" int i2v_coat_cell_gather_f32(const float* x, int frames, int g, int C, int s, int prefix, float* rows, void* stream) {
    CoatCells q{x, rows, frames, g, C, s, prefix, 0};
    return coat_cell_gather(q, (hipStream_t)stream);
}

extern "C" int i2v_coat_cell_scatter_f32(const float* rows, int frames, int g, int C, int s, int prefix, int accumulate, float* dx, void* stream) {
    CoatCells q{rows, dx, frames, g, C, s, prefix, accumulate != 0};
    return coat_cell_scatter(q, (hipStream_t)stream);
}
