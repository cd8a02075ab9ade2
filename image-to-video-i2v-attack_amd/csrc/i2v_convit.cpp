// Planner and executor of the ConViT surrogates (include/i2v_convit.h) on the transformer stack: one arena per (net, max frames), the
// forward as a fixed launch sequence up to the deepest hooked block, and the input-gradient pass -- no weight gradients.  A ConViT block
// is the shared pre-norm block of i2v_xf.h with the gated positional attention launch as its attention step (i2v_convit.hip; without
// -DI2V_HAVE_CONVIT the scalar restatement i2v_convit_host.h).  The first `local_blocks` blocks run on the T patch tokens with one
// (heads, T, ld) table and one (heads) vector each; then the class token joins the stream, and the remaining blocks run on T + 1 tokens
// with plain softmax attention -- the same launch without a table.  Two BlockRuns, one per token count, as Swin runs its stages.
//
// Saved per block as for ViT: x, qkv, Ppatch, y, h and four LayerNorm statistics per token.  The backward pass shares one scratch array
// of the probabilities' size between all blocks: the gradient of the scores.
#include <math.h>

#include "../../include/i2v_convit.h"
#include "i2v_xf.h"
#ifdef I2V_HAVE_CONVIT
#include "i2v_convit_kernels.h"
#else
#include "i2v_convit_host.h"    // (the host simulation's one-file build: the launches as scalar code)
#endif
#ifdef I2V_HAVE_CAIT
#include "i2v_cait_kernels.h"   // cait_add_pos: the plain `+ pos_embed` launch of a stem without a prefix token
#else
#include "i2v_cait_host.h"
#endif

namespace {

struct ConvitBlock : Block {
    const float *c = nullptr, *tab = nullptr;    // 1 - sigma(gating_param) (heads); sigma(gating_param) * Ppos (heads, T, ld); null: plain attention
    int T = 0;                                   // tokens this block runs on
};

}  // namespace

struct i2v_convit : XfNet {
    i2v_convit_config cfg{};
    int T = 0, gsz = 0, nb = 0, nl = 0;          // patch tokens; grid side; blocks run; of these, on T tokens (the rest on T + 1)
    float scale = 0.f;
    const float *pe_w = nullptr, *pe_b = nullptr, *pos = nullptr, *cls = nullptr;
    std::vector<ConvitBlock> blocks;
    float* x_top = nullptr;                      // stream after the last block run
    float *x_join = nullptr, *g_join = nullptr;  // stream after block nl - 1 (T tokens) and its gradient, where blocks follow the join
    float *dS = nullptr, *patches = nullptr;

    bool joined() const { return nb > nl; }
    int tokens_at(int b) const { return b < nl ? T : T + 1; }
    float* stream_after(int b) { return b + 1 == nl && joined() ? x_join : b + 1 < nb ? blocks[b + 1].x : x_top; }
    float* hook_stream(int b) { return stream_after(b); }
    int64_t hook_floats(int b) const { return (int64_t)tokens_at(b) * cfg.dim; }
    BlockRun run(int frames, int tokens, hipStream_t s) const {
        return {frames, tokens, cfg.dim, cfg.mlp, (int64_t)max_frames * tokens, cfg.ln_eps, t1, t2, dqkv, G, s};
    }
    ConvitAttn attn(const ConvitBlock& B, int frames) const {
        ConvitAttn a{};
        a.qkv = B.qkv; a.F = frames; a.T = B.T; a.H = cfg.heads; a.dh = cfg.dim / cfg.heads; a.scale = scale;
        a.c = B.c; a.table = B.tab; a.P = B.P;
        return a;
    }
};

namespace {

int convit_plan(i2v_convit* n, const float* const* w, int nw, const int32_t* hooks, int n_hooks) {
    const i2v_convit_config& c = n->cfg;
    Arena& A = n->arena;
    if (!vit_shape_ok(c) || (c.dim / c.heads) % 4 != 0 || c.local_blocks < 1 || c.local_blocks > c.blocks)
        return fail("i2v_convit_create: unsupported configuration (img %d patch %d dim %d heads %d mlp %d blocks %d local_blocks %d)", c.img,
                    c.patch, c.dim, c.heads, c.mlp, c.blocks, c.local_blocks);
    n->gsz = c.img / c.patch;
    n->T = n->gsz * n->gsz;
    n->scale = 1.f / sqrtf((float)(c.dim / c.heads));
    if (convit_lds_bytes(n->T + 1) > CONVIT_LDS_MAX)
        return fail("i2v_convit_create: %d keys need %lld bytes of LDS per workgroup, over the budget of %d", n->T + 1,
                    (long long)convit_lds_bytes(n->T + 1), (int)CONVIT_LDS_MAX);
    const int deepest = Hooks::deepest(hooks, n_hooks, c.blocks, A);
    if (deepest < 0) return 1;
    n->nb = A.depth = deepest + 1;
    n->nl = n->nb < c.local_blocks ? n->nb : c.local_blocks;
    const int want = 4 + 14 * n->nl + 12 * (n->nb - n->nl);
    if (nw != want) return fail("i2v_convit_create: %d weight arrays given, %d expected for %d blocks", nw, want, n->nb);
    const int64_t D = c.dim, T = n->T, F = n->max_frames, KP = (int64_t)c.in_chans * c.patch * c.patch, H = c.heads, Hm = c.mlp;
    const int64_t ld0 = convit_probs_ld(n->T);
    std::vector<int64_t> sizes = {D * KP, D, T * D, D};
    for (int b = 0; b < n->nb; ++b) {
        for (int64_t v : {D, D, 3 * D * D, 3 * D}) sizes.push_back(v);
        if (b < n->nl) { sizes.push_back(H); sizes.push_back(H * T * ld0); }
        for (int64_t v : {D * D, D, D, D, Hm * D, Hm, D * Hm, D}) sizes.push_back(v);
    }
    // the whole plan in floats, in 64 bits, before the first allocation: weights, per-block saves, shared scratch, hook gradients
    const int64_t Tm = n->tokens_at(n->nb - 1), FT = F * T, FTm = F * Tm, probs_m = F * H * Tm * convit_probs_ld((int)Tm);
    int64_t total = 0;
    for (int b = 0; b < n->nb; ++b) {
        const int64_t Tb = n->tokens_at(b), FTb = F * Tb;
        total += FTb * D + FTb * 3 * D + F * H * Tb * convit_probs_ld((int)Tb) + FTb * D + FTb * Hm + 4 * FTb;
    }
    total += FTm * D + FTm * D + FTm * Hm + probs_m + FTm * 3 * D + FTm * D + FT * KP + (n->joined() ? 2 * FT * D : 0);
    for (int i = 0; i < n_hooks; ++i) total += F * n->tokens_at(hooks[i]) * D;
    for (int64_t v : sizes) total += v;
    VCHK(A.plan(total, FTm));
    if (probs_m >= (1ll << 31) || FTm * Hm >= (1ll << 31) || FT * KP >= (1ll << 31) || F > 65535)
        return fail("i2v_convit_create: %lld bytes needed: too many frames for one net", (long long)A.planned);
    std::vector<const float*> dev;
    VCHK(A.upload(sizes, w, dev));
    n->pe_w = dev[0]; n->pe_b = dev[1]; n->pos = dev[2]; n->cls = dev[3];
    n->blocks.resize(n->nb);
    const float* const* q = &dev[4];
    for (int b = 0; b < n->nb; ++b) {
        ConvitBlock& B = n->blocks[b];
        const bool local = b < n->nl;
        B.weights(q, q + (local ? 6 : 4));
        if (local) { B.c = q[4]; B.tab = q[5]; }
        q += local ? 14 : 12;
        B.T = n->tokens_at(b);
        VCHK(B.alloc_saves(A, F * B.T, D, Hm, F * H * B.T * convit_probs_ld(B.T)));
    }
    if (!(n->x_top = A.alloc(FTm * D)) || !(n->t1 = A.alloc(FTm * D)) || !(n->t2 = A.alloc(FTm * Hm)) || !(n->dS = A.alloc(probs_m)) ||
        !(n->dqkv = A.alloc(FTm * 3 * D)) || !(n->G = A.alloc(FTm * D)) || !(n->patches = A.alloc(FT * KP)))
        return A.oom("scratch");
    if (n->joined() && (!(n->x_join = A.alloc(FT * D)) || !(n->g_join = A.alloc(FT * D)))) return A.oom("scratch at the join");
    for (int i = 0; i < n_hooks; ++i) VCHK(n->hooks.add(A, hooks[i], F * n->tokens_at(hooks[i]) * D));
    return 0;
}

int convit_forward(i2v_convit* n, const float* x, int frames, hipStream_t s) {
    const i2v_convit_config& c = n->cfg;
    float* x0 = n->blocks[0].x;
    VCHK(patch_rows(x, frames, c.in_chans, n->gsz, c.patch, n->pe_w, n->pe_b, c.dim, n->patches, x0, s));
    VCHK(cait_add_pos(x0, n->pos, frames, n->T, c.dim, s));
    for (int b = 0; b < n->nb; ++b) {
        const ConvitBlock& CB = n->blocks[b];
        if (b == n->nl) VCHK(convit_join_cls(n->x_join, n->cls, CB.x, frames, n->T, c.dim, s));      // [cls; x] before the first plain block
        VCHK(block_forward(CB, n->run(frames, CB.T, s), n->stream_after(b), [&](const Block&, float* o) {
            ConvitAttn a = n->attn(CB, frames);
            a.out = o;
            return convit_attention(a, s);
        }));
    }
    return 0;
}

int convit_backward(i2v_convit* n, float* gx, int accumulate, hipStream_t s) {
    const i2v_convit_config& c = n->cfg;
    const int frames = n->frames;
    for (int b = n->nb - 1; b >= 0; --b) {
        // gradient of the stream after block b: the top hook's view for the deepest block, the running gradient G below it (where the
        // LN1 backward of block b + 1 has already added the hook at that stream) -- except across the join, where the stream after
        // block nl - 1 has T tokens and the gradient of block nl's input T + 1: rows 1 .. T of G plus that hook go to g_join
        const bool below_join = n->joined() && b == n->nl - 1, at_join = n->joined() && b == n->nl;
        const float* gin = below_join ? n->g_join : n->grad_in(b, n->nb);
        const ConvitBlock& CB = n->blocks[b];
        VCHK(block_backward(CB, n->run(frames, CB.T, s), gin, at_join ? nullptr : n->grad_below(b),
                            [&](const Block&, const float* dout) {
                                ConvitAttn a = n->attn(CB, frames);
                                a.dout = dout; a.dS = n->dS; a.dqkv = n->dqkv;
                                return convit_attention_bwd(a, s);
                            }));
        if (at_join) VCHK(convit_join_cls_bwd(n->G, n->hooks.grad_at(b - 1), n->g_join, frames, n->T, c.dim, s));
    }
    // pos_embed is an addend: the patch rows' gradient is the stream's, times the patch weight
    return patch_rows_bwd(n->G, frames, c.in_chans, n->gsz, c.patch, n->pe_w, c.dim, n->patches, gx, accumulate, s);
}

}  // namespace

extern "C" int i2v_convit_create(int device, const i2v_convit_config* cfg, const float* const* weights, int n_weights, const int32_t* hook_blocks,
                                 int n_hooks, int max_frames, i2v_convit_handle* out) {
    return xf_create("i2v_convit_create", "block", device, cfg, weights, hook_blocks, max_frames, out, [&](i2v_convit* n) {
        n->cfg = *cfg;
        return convit_plan(n, weights, n_weights, hook_blocks, n_hooks);
    });
}

extern "C" int i2v_convit_destroy(i2v_convit_handle net) { return xf_destroy(net); }

extern "C" int64_t i2v_convit_workspace_bytes(i2v_convit_handle net) { return xf_workspace_bytes(net); }

extern "C" int i2v_convit_forward(i2v_convit_handle n, const float* x, int frames, void* stream) {
    return xf_forward("i2v_convit_forward", n, x, frames, stream, convit_forward);
}

extern "C" int i2v_convit_backward(i2v_convit_handle n, float* gx, int accumulate, void* stream) {
    return xf_backward("i2v_convit_backward", n, gx, accumulate, stream, convit_backward);
}

extern "C" int i2v_convit_hook_info(i2v_convit_handle n, int hook, float** act, int64_t* act_stride, float** grad, int64_t* grad_stride,
                                    int64_t* D) {
    return xf_hook_info("i2v_convit_hook_info", n, hook, act, act_stride, grad, grad_stride, D);
}

extern "C" int i2v_convit_read_hook(i2v_convit_handle n, int hook, int which, float* out, int frames, void* stream) {
    return xf_read_hook("i2v_convit_read_hook", n, hook, which, out, frames, stream);
}

// ---- the kernel on its own ----
extern "C" int i2v_convit_attention_f32(const float* qkv, int frames, int T, int heads, int dh, float scale, const float* c, const float* table,
                                        float* probs, float* out, void* stream) {
    ConvitAttn a{};
    a.qkv = qkv; a.F = frames; a.T = T; a.H = heads; a.dh = dh; a.scale = scale; a.c = c; a.table = table; a.P = probs; a.out = out;
    return convit_attention(a, (hipStream_t)stream);
}

extern "C" int i2v_convit_attention_bwd_f32(const float* qkv, const float* probs, const float* dout, int frames, int T, int heads, int dh,
                                            float scale, const float* c, const float* table, float* ds_scratch, float* dqkv, void* stream) {
    ConvitAttn a{};
    a.qkv = qkv; a.F = frames; a.T = T; a.H = heads; a.dh = dh; a.scale = scale; a.c = c; a.table = table;
    a.P = const_cast<float*>(probs); a.dout = dout; a.dS = ds_scratch; a.dqkv = dqkv;
    return convit_attention_bwd(a, (hipStream_t)stream);
}

extern "C" int i2v_convit_join_cls_f32(const float* x, const float* cls, float* out, int frames, int T, int C, void* stream) {
    return convit_join_cls(x, cls, out, frames, T, C, (hipStream_t)stream);
}

extern "C" int i2v_convit_join_cls_bwd_f32(const float* dout, const float* add, float* dx, int frames, int T, int C, void* stream) {
    return convit_join_cls_bwd(dout, add, dx, frames, T, C, (hipStream_t)stream);
}
