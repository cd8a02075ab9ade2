// Planner and executor of the ViT surrogate (include/i2v_vit.h): one arena per (net, max frames), the forward as a fixed launch sequence
// up to the deepest hook, and the input-gradient pass -- no weight gradients, as the CNN path.  The arena, the hook list and the pre-norm
// block are shared with the Swin planner (i2v_xf.h); this file brings the embedding with its prefix rows, the attention over all tokens
// with saved probabilities, and the ViT sizes.  The kernels are in i2v_vit.hip.
#include <math.h>

#include "../../include/i2v_vit.h"
#include "i2v_xf.h"

namespace {

int probs_ld(int T) { return (T + 3) / 4 * 4; }

// batch b = frame * heads + head.  qkv (F, T, 3C): q of head h at column h*dh, k at C + h*dh, v at 2C + h*dh; probs (F, heads, T, ld)
int attention(const float* qkv, int F, int T, int heads, int dh, float scale, float* P, float* out, hipStream_t s) {
    const int C = heads * dh, ld = probs_ld(T);
    const int64_t qs = 3LL * C * T, ps = (int64_t)T * ld;
    VitGemm g{};                                           // S = scale q k^T
    g.A = qkv; g.a_bo = qs; g.a_bi = dh; g.a_sm = 3 * C; g.a_sk = 1;
    g.B = qkv + C; g.b_bo = qs; g.b_bi = dh; g.b_sk = 1; g.b_sn = 3 * C;
    g.C = P; g.c_bo = heads * ps; g.c_bi = ps; g.c_sm = ld;
    g.M = T; g.N = T; g.K = dh; g.batch = F * heads; g.nb_in = heads; g.alpha = scale;
    VCHK(vit_gemm(g, s));
    VCHK(vit_softmax(P, (int64_t)F * heads * T, T, ld, s));
    VitGemm o{};                                           // out = P v
    o.A = P; o.a_bo = heads * ps; o.a_bi = ps; o.a_sm = ld; o.a_sk = 1;
    o.B = qkv + 2 * C; o.b_bo = qs; o.b_bi = dh; o.b_sk = 3 * C; o.b_sn = 1;
    o.C = out; o.c_bo = (int64_t)T * C; o.c_bi = dh; o.c_sm = C;
    o.M = T; o.N = dh; o.K = T; o.batch = F * heads; o.nb_in = heads; o.alpha = 1.f;
    return vit_gemm(o, s);
}

int attention_bwd(const float* qkv, const float* P, const float* dout, int F, int T, int heads, int dh, float scale, float* dP, float* dqkv,
                  hipStream_t s) {
    const int C = heads * dh, ld = probs_ld(T);
    const int64_t qs = 3LL * C * T, ps = (int64_t)T * ld, os = (int64_t)T * C;
    VitGemm g{};                                           // dP = dout v^T
    g.A = dout; g.a_bo = os; g.a_bi = dh; g.a_sm = C; g.a_sk = 1;
    g.B = qkv + 2 * C; g.b_bo = qs; g.b_bi = dh; g.b_sk = 1; g.b_sn = 3 * C;
    g.C = dP; g.c_bo = heads * ps; g.c_bi = ps; g.c_sm = ld;
    g.M = T; g.N = T; g.K = dh; g.batch = F * heads; g.nb_in = heads; g.alpha = 1.f;
    VCHK(vit_gemm(g, s));
    VCHK(vit_softmax_bwd(dP, P, (int64_t)F * heads * T, T, ld, scale, s));    // dS = scale * P (dP - rowsum(dP P))
    VitGemm q{};                                           // dq = dS k
    q.A = dP; q.a_bo = heads * ps; q.a_bi = ps; q.a_sm = ld; q.a_sk = 1;
    q.B = qkv + C; q.b_bo = qs; q.b_bi = dh; q.b_sk = 3 * C; q.b_sn = 1;
    q.C = dqkv; q.c_bo = qs; q.c_bi = dh; q.c_sm = 3 * C;
    q.M = T; q.N = dh; q.K = T; q.batch = F * heads; q.nb_in = heads; q.alpha = 1.f;
    VCHK(vit_gemm(q, s));
    VitGemm k = q;                                         // dk = dS^T q
    k.A = dP; k.a_sm = 1; k.a_sk = ld;
    k.B = qkv;
    k.C = dqkv + C;
    VCHK(vit_gemm(k, s));
    VitGemm v = k;                                         // dv = P^T dout
    v.A = P;
    v.B = dout; v.b_bo = os; v.b_bi = dh; v.b_sk = C; v.b_sn = 1;
    v.C = dqkv + 2 * C;
    return vit_gemm(v, s);
}

// `prefix`: (npre, dim), the rows ahead of the patch rows (cls_token; then dist_token of a distilled DeiT)
int embed(const float* img, int F, int Cin, int gsz, int P, const float* W, const float* b, const float* prefix, int npre, const float* pos,
          int dim, float* patches, float* emb, float* tokens, hipStream_t s) {
    if (npre < 1) return fail("i2v_vit_embed: %d prefix tokens (at least 1)", npre);
    const int np = gsz * gsz, KP = Cin * P * P;
    VCHK(vit_patchify(img, patches, F, Cin, gsz, gsz, P, nullptr, 0, s));
    VCHK(linear(patches, F * np, KP, W, b, dim, nullptr, emb, nullptr, s));
    return vit_assemble(emb, prefix, npre, pos, tokens, F, np + npre, dim, s);
}

// the patch rows' gradient is the token gradient without the prefix rows (a slice from row npre of each frame, read in place by the
// GEMM), times W
int embed_bwd(const float* dtok, int F, int Cin, int gsz, int P, const float* W, int dim, int npre, float* patches, float* gimg,
              int accumulate, hipStream_t s) {
    if (npre < 1) return fail("i2v_vit_embed_bwd: %d prefix tokens (at least 1)", npre);
    const int np = gsz * gsz, KP = Cin * P * P;
    VitGemm g{};
    g.A = dtok + (int64_t)npre * dim; g.a_bo = (int64_t)(np + npre) * dim; g.a_sm = dim; g.a_sk = 1;
    g.B = W; g.b_sk = KP; g.b_sn = 1;
    g.C = patches; g.c_bo = (int64_t)np * KP; g.c_sm = KP;
    g.M = np; g.N = KP; g.K = dim; g.batch = F; g.nb_in = 1; g.alpha = 1.f;
    VCHK(vit_gemm(g, s));
    return vit_patchify(nullptr, patches, F, Cin, gsz, gsz, P, gimg, accumulate, s);
}

}  // namespace

struct i2v_vit : XfNet {
    i2v_vit_config cfg{};
    int T = 0, gsz = 0, nb = 0, ld = 0, npre = 1;
    float scale = 0.f;
    const float *pe_w = nullptr, *pe_b = nullptr, *prefix = nullptr, *pos = nullptr;
    std::vector<Block> blocks;
    float* x_top = nullptr;                      // stream after the last block run
    float *dP = nullptr, *patches = nullptr, *emb = nullptr;

    float* stream_after(int b) { return b + 1 < nb ? blocks[b + 1].x : x_top; }
    BlockRun run(int frames, hipStream_t s) const {
        return {frames, T, cfg.dim, cfg.mlp, (int64_t)max_frames * T, cfg.ln_eps, t1, t2, dqkv, G, s};
    }
};

namespace {

int vit_plan(i2v_vit* n, const float* const* w, int nw, const int32_t* hooks, int n_hooks) {
    const i2v_vit_config& c = n->cfg;
    Arena& A = n->arena;
    if (c.img <= 0 || c.patch <= 0 || c.img % c.patch != 0 || c.patch % 4 != 0 || c.in_chans <= 0 || c.dim <= 0 || c.heads <= 0 ||
        c.dim % c.heads != 0 || c.dim % 4 != 0 || (c.dim / c.heads) % 4 != 0 || c.mlp <= 0 || c.mlp % 4 != 0 || c.blocks <= 0)
        return fail("i2v_vit_create: unsupported configuration (img %d patch %d dim %d heads %d mlp %d blocks %d)", c.img, c.patch, c.dim, c.heads,
                    c.mlp, c.blocks);
    if (n->npre < 1 || n->npre > 2) return fail("i2v_vit_create: %d prefix tokens (1: cls_token, or 2: cls_token and dist_token)", n->npre);
    const int deepest = Hooks::deepest(hooks, n_hooks, c.blocks, A);
    if (deepest < 0) return 1;
    n->nb = A.depth = deepest + 1;
    if (nw != 4 + 12 * n->nb) return fail("i2v_vit_create: %d weight arrays given, %d expected for %d blocks", nw, 4 + 12 * n->nb, n->nb);
    n->gsz = c.img / c.patch;
    n->T = n->npre + n->gsz * n->gsz;
    n->ld = probs_ld(n->T);
    n->scale = 1.f / sqrtf((float)(c.dim / c.heads));     // dh^-0.5 (exactly 0.125 for dh = 64)
    const int64_t D = c.dim, T = n->T, F = n->max_frames, KP = (int64_t)c.in_chans * c.patch * c.patch;
    // weights
    std::vector<int64_t> sizes = {D * KP, D, n->npre * D, T * D};
    for (int b = 0; b < n->nb; ++b)
        for (int64_t v : {D, D, 3 * D * D, 3 * D, D * D, D, D, D, (int64_t)c.mlp * D, (int64_t)c.mlp, D * c.mlp, D}) sizes.push_back(v);
    // the whole plan in floats, in 64 bits, before the first allocation: weights, per-block saves, shared scratch, hook gradients
    const int64_t FT = F * T, Hm = c.mlp, NPt = T - n->npre, probs = F * c.heads * T * n->ld;
    const int64_t per_block = FT * D + FT * 3 * D + probs + FT * D + FT * Hm + 4 * FT;
    const int64_t shared = FT * D + FT * D + FT * Hm + probs + FT * 3 * D + FT * D + F * NPt * KP + F * NPt * D;
    int64_t total = n->nb * per_block + shared + (int64_t)n_hooks * FT * D;
    for (int64_t v : sizes) total += v;
    VCHK(A.plan(total, FT));
    std::vector<const float*> dev;
    VCHK(A.upload(sizes, w, dev));
    n->pe_w = dev[0]; n->pe_b = dev[1]; n->prefix = dev[2]; n->pos = dev[3];
    n->blocks.resize(n->nb);
    for (int b = 0; b < n->nb; ++b) {
        Block& B = n->blocks[b];
        B.weights(&dev[4 + 12 * b], &dev[8 + 12 * b]);
        if (!(B.x = A.alloc(FT * D)) || !(B.qkv = A.alloc(FT * 3 * D)) || !(B.P = A.alloc(probs)) ||
            !(B.y = A.alloc(FT * D)) || !(B.h = A.alloc(FT * Hm)) || !(B.stats = A.alloc(4 * FT)))
            return A.oom("saved activations of a block");
    }
    if (!(n->x_top = A.alloc(FT * D)) || !(n->t1 = A.alloc(FT * D)) || !(n->t2 = A.alloc(FT * Hm)) ||
        !(n->dP = A.alloc(probs)) || !(n->dqkv = A.alloc(FT * 3 * D)) || !(n->G = A.alloc(FT * D)) ||
        !(n->patches = A.alloc(F * NPt * KP)) || !(n->emb = A.alloc(F * NPt * D)))
        return A.oom("scratch");
    for (int i = 0; i < n_hooks; ++i) VCHK(n->hooks.add(A, hooks[i], FT * D));
    return 0;
}

}  // namespace

extern "C" int i2v_vit_create(int device, const i2v_vit_config* cfg, const float* const* weights, int n_weights, const int32_t* hook_blocks,
                              int n_hooks, int max_frames, i2v_vit_handle* out) {
    return i2v_vit_create_ex(device, cfg, 1, weights, n_weights, hook_blocks, n_hooks, max_frames, out);
}

extern "C" int i2v_vit_create_ex(int device, const i2v_vit_config* cfg, int n_prefix, const float* const* weights, int n_weights,
                                 const int32_t* hook_blocks, int n_hooks, int max_frames, i2v_vit_handle* out) {
    if (!cfg || !weights || !hook_blocks || !out) return fail("i2v_vit_create: null argument");
    return create_net("i2v_vit_create", "block", device, max_frames, out, [&](i2v_vit* n) {
        n->cfg = *cfg;
        n->npre = n_prefix;
        return vit_plan(n, weights, n_weights, hook_blocks, n_hooks);
    });
}

extern "C" int i2v_vit_destroy(i2v_vit_handle net) {
    delete net;
    return 0;
}

extern "C" int64_t i2v_vit_workspace_bytes(i2v_vit_handle net) { return net ? net->arena.bytes : -1; }

extern "C" int i2v_vit_forward(i2v_vit_handle n, const float* x, int frames, void* stream) {
    if (!n || !x) return fail("i2v_vit_forward: null argument");
    if (frames <= 0 || frames > n->max_frames) return fail("i2v_vit_forward: %d frames, the net is planned for 1..%d", frames, n->max_frames);
    hipStream_t s = (hipStream_t)stream;
    const i2v_vit_config& c = n->cfg;
    const int heads = c.heads, dh = c.dim / heads;
    const BlockRun r = n->run(frames, s);
    n->frames = frames;
    VCHK(embed(x, frames, c.in_chans, n->gsz, c.patch, n->pe_w, n->pe_b, n->prefix, n->npre, n->pos, c.dim, n->patches, n->emb, n->blocks[0].x, s));
    for (int b = 0; b < n->nb; ++b)
        VCHK(block_forward(n->blocks[b], r, n->stream_after(b), [&](const Block& B, float* o) {
            return attention(B.qkv, frames, n->T, heads, dh, n->scale, B.P, o, s);
        }));
    return 0;
}

extern "C" int i2v_vit_backward(i2v_vit_handle n, float* gx, int accumulate, void* stream) {
    if (!n || !gx) return fail("i2v_vit_backward: null argument");
    if (n->frames <= 0) return fail("i2v_vit_backward: no forward pass to differentiate");
    hipStream_t s = (hipStream_t)stream;
    const i2v_vit_config& c = n->cfg;
    const int frames = n->frames, heads = c.heads, dh = c.dim / heads;
    const BlockRun r = n->run(frames, s);
    for (int b = n->nb - 1; b >= 0; --b) {
        // gradient of the stream after block b: the top hook's view for the deepest block, the running gradient G below it (where
        // the LN1 backward of block b + 1 has already added the hook at that stream)
        const float* gin = b == n->nb - 1 ? n->hooks.grad_at(b) : n->G;
        VCHK(block_backward(n->blocks[b], r, gin, b > 0 ? n->hooks.grad_at(b - 1) : nullptr, [&](const Block& B, const float* dout) {
            return attention_bwd(B.qkv, B.P, dout, frames, n->T, heads, dh, n->scale, n->dP, n->dqkv, s);
        }));
    }
    return embed_bwd(n->G, frames, c.in_chans, n->gsz, c.patch, n->pe_w, c.dim, n->npre, n->patches, gx, accumulate, s);
}

extern "C" int i2v_vit_hook_info(i2v_vit_handle n, int hook, float** act, int64_t* act_stride, float** grad, int64_t* grad_stride, int64_t* D) {
    if (!n || !n->hooks.has(hook)) return fail("i2v_vit_hook_info: no hook %d", hook);
    return hook_info(n->stream_after(n->hooks.at[hook]), n->hooks.grad[hook], (int64_t)n->T * n->cfg.dim, act, act_stride, grad, grad_stride, D);
}

extern "C" int i2v_vit_read_hook(i2v_vit_handle n, int hook, int which, float* out, int frames, void* stream) {
    if (!n || !out || !n->hooks.has(hook)) return fail("i2v_vit_read_hook: no hook %d", hook);
    return read_hook("i2v_vit_read_hook", which ? n->hooks.grad[hook] : n->stream_after(n->hooks.at[hook]), (int64_t)n->T * n->cfg.dim, out,
                     frames, n->max_frames, stream);
}

// ---- the kernels on their own ----
extern "C" int i2v_vit_linear_f32(const float* x, int M, int K, const float* W, const float* bias, int N, const float* residual, float* y,
                                  float* gelu_out, void* stream) {
    return linear(x, M, K, W, bias, N, residual, y, gelu_out, (hipStream_t)stream);
}
extern "C" int i2v_vit_linear_bwd_f32(const float* dy, int M, int N, const float* W, int K, const float* pre, float* dx, void* stream) {
    return linear_bwd(dy, M, N, W, K, pre, dx, (hipStream_t)stream);
}
extern "C" int i2v_vit_layernorm_f32(const float* x, int64_t rows, int C, const float* gamma, const float* beta, float eps, float* out,
                                     float* mean, float* rstd, void* stream) {
    return vit_layernorm(x, rows, C, gamma, beta, eps, out, mean, rstd, (hipStream_t)stream);
}
extern "C" int i2v_vit_layernorm_bwd_f32(const float* dy, const float* x, const float* mean, const float* rstd, const float* gamma,
                                         int64_t rows, int C, const float* add0, const float* add1, float* dx, void* stream) {
    return vit_layernorm_bwd(dy, x, mean, rstd, gamma, rows, C, add0, add1, dx, (hipStream_t)stream);
}
extern "C" int i2v_vit_probs_ld(int T) { return probs_ld(T); }
extern "C" int i2v_vit_attention_f32(const float* qkv, int frames, int T, int heads, int dh, float scale, float* probs, float* out,
                                     void* stream) {
    return attention(qkv, frames, T, heads, dh, scale, probs, out, (hipStream_t)stream);
}
extern "C" int i2v_vit_attention_bwd_f32(const float* qkv, const float* probs, const float* dout, int frames, int T, int heads, int dh,
                                         float scale, float* dprobs, float* dqkv, void* stream) {
    return attention_bwd(qkv, probs, dout, frames, T, heads, dh, scale, dprobs, dqkv, (hipStream_t)stream);
}
extern "C" int i2v_vit_embed_f32(const float* img, int frames, int in_chans, int g, int patch, const float* W, const float* b,
                                 const float* cls, const float* pos, int dim, float* patches, float* emb, float* tokens, void* stream) {
    return embed(img, frames, in_chans, g, patch, W, b, cls, 1, pos, dim, patches, emb, tokens, (hipStream_t)stream);
}
extern "C" int i2v_vit_embed_ex_f32(const float* img, int frames, int in_chans, int g, int patch, const float* W, const float* b,
                                    const float* prefix, int n_prefix, const float* pos, int dim, float* patches, float* emb, float* tokens,
                                    void* stream) {
    return embed(img, frames, in_chans, g, patch, W, b, prefix, n_prefix, pos, dim, patches, emb, tokens, (hipStream_t)stream);
}
extern "C" int i2v_vit_embed_bwd_f32(const float* dtokens, int frames, int in_chans, int g, int patch, const float* W, int dim,
                                     float* patches, float* gimg, int accumulate, void* stream) {
    return embed_bwd(dtokens, frames, in_chans, g, patch, W, dim, 1, patches, gimg, accumulate, (hipStream_t)stream);
}
extern "C" int i2v_vit_embed_bwd_ex_f32(const float* dtokens, int frames, int in_chans, int g, int patch, const float* W, int dim,
                                        int n_prefix, float* patches, float* gimg, int accumulate, void* stream) {
    return embed_bwd(dtokens, frames, in_chans, g, patch, W, dim, n_prefix, patches, gimg, accumulate, (hipStream_t)stream);
}
