// Planner and executor of the ViT surrogate (include/i2v_vit.h): one arena per (net, max frames), the forward as a fixed launch sequence
// up to the deepest hook, and the input-gradient pass -- no weight gradients, as the CNN path.  The arena, the hook list, the seven entries'
// guards, the block stack and the attention composed from the shared launches are those of i2v_xf.h; this file brings the embedding with
// its prefix rows, the ViT sizes, and the kernels on their own.  The kernels are in i2v_vit.hip.
#include <math.h>

#include "../../include/i2v_vit.h"
#include "i2v_xf.h"

namespace {

// batch b = frame * heads + head.  qkv (F, T, 3C): q of head h at column h*dh, k at C + h*dh, v at 2C + h*dh; probs (F, heads, T, ld)
int attention(const float* qkv, int F, int T, int heads, int dh, float scale, float* P, float* out, hipStream_t s) {
    return xf_attention(xf_attn_qkv(qkv, F, T, heads, dh, scale), P, out, s);
}

int attention_bwd(const float* qkv, const float* P, const float* dout, int F, int T, int heads, int dh, float scale, float* dP, float* dqkv,
                  hipStream_t s) {
    const int C = heads * dh;
    return xf_attention_bwd(xf_attn_qkv(qkv, F, T, heads, dh, scale), P, dout, dP, dqkv, dqkv + C, dqkv + 2 * C, s);
}

// `prefix`: (npre, dim), the rows ahead of the patch rows (cls_token; then dist_token of a distilled DeiT)
int embed(const float* img, int F, int Cin, int gsz, int P, const float* W, const float* b, const float* prefix, int npre, const float* pos,
          int dim, float* patches, float* emb, float* tokens, hipStream_t s) {
    if (npre < 1) return fail("i2v_vit_embed: %d prefix tokens (at least 1)", npre);
    VCHK(patch_rows(img, F, Cin, gsz, P, W, b, dim, patches, emb, s));
    return vit_assemble(emb, prefix, npre, pos, tokens, F, gsz * gsz + npre, dim, s);
}

int embed_bwd(const float* dtok, int F, int Cin, int gsz, int P, const float* W, int dim, int npre, float* patches, float* gimg,
              int accumulate, hipStream_t s) {
    if (npre < 1) return fail("i2v_vit_embed_bwd: %d prefix tokens (at least 1)", npre);
    return patch_rows_bwd_prefix(dtok, F, Cin, gsz, P, W, dim, npre, patches, gimg, accumulate, s);
}

}  // namespace

struct i2v_vit : XfStack<i2v_vit_config> {
    int ld = 0, npre = 1;
    const float *pe_w = nullptr, *pe_b = nullptr, *prefix = nullptr, *pos = nullptr;
    float *dP = nullptr, *patches = nullptr, *emb = nullptr;
};

namespace {

int vit_plan(i2v_vit* n, const float* const* w, int nw, const int32_t* hooks, int n_hooks) {
    const i2v_vit_config& c = n->cfg;
    Arena& A = n->arena;
    if (!vit_shape_ok(c) || (c.dim / c.heads) % 4 != 0)
        return fail("i2v_vit_create: unsupported configuration (img %d patch %d dim %d heads %d mlp %d blocks %d)", c.img, c.patch, c.dim, c.heads,
                    c.mlp, c.blocks);
    if (n->npre < 1 || n->npre > 2) return fail("i2v_vit_create: %d prefix tokens (1: cls_token, or 2: cls_token and dist_token)", n->npre);
    const int deepest = Hooks::deepest(hooks, n_hooks, c.blocks, A);
    if (deepest < 0) return 1;
    n->nb = A.depth = deepest + 1;
    if (nw != 4 + 12 * n->nb) return fail("i2v_vit_create: %d weight arrays given, %d expected for %d blocks", nw, 4 + 12 * n->nb, n->nb);
    n->gsz = c.img / c.patch;
    n->T = n->npre + n->gsz * n->gsz;
    n->ld = xf_probs_ld(n->T);
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
        VCHK(B.alloc_saves(A, FT, D, Hm, probs));
    }
    if (!(n->x_top = A.alloc(FT * D)) || !(n->t1 = A.alloc(FT * D)) || !(n->t2 = A.alloc(FT * Hm)) ||
        !(n->dP = A.alloc(probs)) || !(n->dqkv = A.alloc(FT * 3 * D)) || !(n->G = A.alloc(FT * D)) ||
        !(n->patches = A.alloc(F * NPt * KP)) || !(n->emb = A.alloc(F * NPt * D)))
        return A.oom("scratch");
    for (int i = 0; i < n_hooks; ++i) VCHK(n->hooks.add(A, hooks[i], FT * D));
    return 0;
}

int vit_forward(i2v_vit* n, const float* x, int frames, hipStream_t s) {
    const i2v_vit_config& c = n->cfg;
    VCHK(embed(x, frames, c.in_chans, n->gsz, c.patch, n->pe_w, n->pe_b, n->prefix, n->npre, n->pos, c.dim, n->patches, n->emb, n->blocks[0].x, s));
    return n->forward_blocks(frames, s, [&](int b, float* o) {
        return attention(n->blocks[b].qkv, frames, n->T, c.heads, c.dim / c.heads, n->scale, n->blocks[b].P, o, s);
    });
}

int vit_backward(i2v_vit* n, float* gx, int accumulate, hipStream_t s) {
    const i2v_vit_config& c = n->cfg;
    const int frames = n->frames;
    VCHK(n->backward_blocks(frames, s, [&](int b, const float* dout) {
        return attention_bwd(n->blocks[b].qkv, n->blocks[b].P, dout, frames, n->T, c.heads, c.dim / c.heads, n->scale, n->dP, n->dqkv, s);
    }));
    return embed_bwd(n->G, frames, c.in_chans, n->gsz, c.patch, n->pe_w, c.dim, n->npre, n->patches, gx, accumulate, s);
}

}  // namespace

extern "C" int i2v_vit_create(int device, const i2v_vit_config* cfg, const float* const* weights, int n_weights, const int32_t* hook_blocks,
                              int n_hooks, int max_frames, i2v_vit_handle* out) {
    return i2v_vit_create_ex(device, cfg, 1, weights, n_weights, hook_blocks, n_hooks, max_frames, out);
}

extern "C" int i2v_vit_create_ex(int device, const i2v_vit_config* cfg, int n_prefix, const float* const* weights, int n_weights,
                                 const int32_t* hook_blocks, int n_hooks, int max_frames, i2v_vit_handle* out) {
    return xf_create("i2v_vit_create", "block", device, cfg, weights, hook_blocks, max_frames, out, [&](i2v_vit* n) {
        n->cfg = *cfg;
        n->npre = n_prefix;
        return vit_plan(n, weights, n_weights, hook_blocks, n_hooks);
    });
}

extern "C" int i2v_vit_destroy(i2v_vit_handle net) { return xf_destroy(net); }

extern "C" int64_t i2v_vit_workspace_bytes(i2v_vit_handle net) { return xf_workspace_bytes(net); }

extern "C" int i2v_vit_forward(i2v_vit_handle n, const float* x, int frames, void* stream) {
    return xf_forward("i2v_vit_forward", n, x, frames, stream, vit_forward);
}

extern "C" int i2v_vit_backward(i2v_vit_handle n, float* gx, int accumulate, void* stream) {
    return xf_backward("i2v_vit_backward", n, gx, accumulate, stream, vit_backward);
}

extern "C" int i2v_vit_hook_info(i2v_vit_handle n, int hook, float** act, int64_t* act_stride, float** grad, int64_t* grad_stride, int64_t* D) {
    return xf_hook_info("i2v_vit_hook_info", n, hook, act, act_stride, grad, grad_stride, D);
}

extern "C" int i2v_vit_read_hook(i2v_vit_handle n, int hook, int which, float* out, int frames, void* stream) {
    return xf_read_hook("i2v_vit_read_hook", n, hook, which, out, frames, stream);
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
extern "C" int i2v_vit_probs_ld(int T) { return xf_probs_ld(T); }
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
