// Planner and executor of the CaiT surrogates (include/i2v_cait.h) on the transformer stack: one arena per (net, max frames), the forward
// as a fixed launch sequence up to the deepest hooked block, and the input-gradient pass -- no weight gradients.  A CaiT self-attention
// block is the shared pre-norm block of i2v_xf.h with talking-heads attention as its attention step (i2v_cait.hip; without
// -DI2V_HAVE_CAIT the scalar restatement i2v_cait_host.h): the LayerScale vectors arrive folded into proj and fc2, and there is no prefix
// token, so the stem is ViT's patchify plus a Linear and a plain `+ pos_embed` launch in place.  The class-attention stage lies behind
// every hook and is not built.
//
// Saved per block as for ViT: x, qkv, P (post-softmax, pre-mix), y, h and four LayerNorm statistics per token.  The backward pass shares
// two scratch arrays of P's size between all blocks: the gradient of the scores and the mixed probabilities.
#include <math.h>

#include "../../include/i2v_cait.h"
#include "i2v_xf.h"
#ifdef I2V_HAVE_CAIT
#include "i2v_cait_kernels.h"
#else
#include "i2v_cait_host.h"      // (the host simulation's one-file build: the three launches as scalar code)
#endif

namespace {

struct CaitBlock : Block {
    const float *wl = nullptr, *bl = nullptr, *ww = nullptr, *bw = nullptr;      // attn.proj_l, attn.proj_w
};

}  // namespace

struct i2v_cait : XfStack<i2v_cait_config, CaitBlock> {
    int ld = 0;
    const float *pe_w = nullptr, *pe_b = nullptr, *pos = nullptr;
    float *dS = nullptr, *Pm = nullptr, *patches = nullptr;

    CaitAttn attn(const CaitBlock& B, int frames) const {
        CaitAttn a{};
        a.qkv = B.qkv; a.F = frames; a.T = T; a.H = cfg.heads; a.dh = cfg.dim / cfg.heads; a.scale = scale;
        a.wl = B.wl; a.bl = B.bl; a.ww = B.ww; a.bw = B.bw; a.P = B.P;
        return a;
    }
};

namespace {

int cait_plan(i2v_cait* n, const float* const* w, int nw, const int32_t* hooks, int n_hooks) {
    const i2v_cait_config& c = n->cfg;
    Arena& A = n->arena;
    if (!vit_shape_ok(c) || (c.dim / c.heads) % 4 != 0)
        return fail("i2v_cait_create: unsupported configuration (img %d patch %d dim %d heads %d mlp %d blocks %d)", c.img, c.patch, c.dim,
                    c.heads, c.mlp, c.blocks);
    n->gsz = c.img / c.patch;
    n->T = n->gsz * n->gsz;
    n->ld = cait_probs_ld(n->T);
    n->scale = 1.f / sqrtf((float)(c.dim / c.heads));
    if (c.heads > CAIT_MAX_HEADS || cait_lds_bytes(n->T, c.heads) > CAIT_LDS_MAX)
        return fail("i2v_cait_create: %d heads over %d tokens need %lld bytes of LDS per workgroup, over the budget of %d (and at most %d heads)",
                    c.heads, n->T, (long long)cait_lds_bytes(n->T, c.heads), (int)CAIT_LDS_MAX, (int)CAIT_MAX_HEADS);
    const int deepest = Hooks::deepest(hooks, n_hooks, c.blocks, A);
    if (deepest < 0) return 1;
    n->nb = A.depth = deepest + 1;
    if (nw != 3 + 16 * n->nb) return fail("i2v_cait_create: %d weight arrays given, %d expected for %d blocks", nw, 3 + 16 * n->nb, n->nb);
    const int64_t D = c.dim, T = n->T, F = n->max_frames, KP = (int64_t)c.in_chans * c.patch * c.patch, H = c.heads, Hm = c.mlp;
    std::vector<int64_t> sizes = {D * KP, D, T * D};
    for (int b = 0; b < n->nb; ++b)
        for (int64_t v : {D, D, 3 * D * D, 3 * D, H * H, H, H * H, H, D * D, D, D, D, Hm * D, Hm, D * Hm, D}) sizes.push_back(v);
    // the whole plan in floats, in 64 bits, before the first allocation: weights, per-block saves, shared scratch, hook gradients
    const int64_t FT = F * T, probs = F * H * T * n->ld;
    const int64_t per_block = FT * D + FT * 3 * D + probs + FT * D + FT * Hm + 4 * FT;
    const int64_t shared = FT * D + FT * D + FT * Hm + 2 * probs + FT * 3 * D + FT * D + FT * KP;
    int64_t total = n->nb * per_block + shared + (int64_t)n_hooks * FT * D;
    for (int64_t v : sizes) total += v;
    VCHK(A.plan(total, FT));
    if (probs >= (1ll << 31) || FT * Hm >= (1ll << 31) || FT * KP >= (1ll << 31) || F > 65535)
        return fail("i2v_cait_create: %lld bytes needed: too many frames for one net", (long long)A.planned);
    std::vector<const float*> dev;
    VCHK(A.upload(sizes, w, dev));
    n->pe_w = dev[0]; n->pe_b = dev[1]; n->pos = dev[2];
    n->blocks.resize(n->nb);
    for (int b = 0; b < n->nb; ++b) {
        CaitBlock& B = n->blocks[b];
        const float* const* q = &dev[3 + 16 * b];
        B.weights(q, q + 8);
        B.wl = q[4]; B.bl = q[5]; B.ww = q[6]; B.bw = q[7];
        VCHK(B.alloc_saves(A, FT, D, Hm, probs));
    }
    if (!(n->x_top = A.alloc(FT * D)) || !(n->t1 = A.alloc(FT * D)) || !(n->t2 = A.alloc(FT * Hm)) || !(n->dS = A.alloc(probs)) ||
        !(n->Pm = A.alloc(probs)) || !(n->dqkv = A.alloc(FT * 3 * D)) || !(n->G = A.alloc(FT * D)) || !(n->patches = A.alloc(FT * KP)))
        return A.oom("scratch");
    for (int i = 0; i < n_hooks; ++i) VCHK(n->hooks.add(A, hooks[i], FT * D));
    return 0;
}

int cait_forward(i2v_cait* n, const float* x, int frames, hipStream_t s) {
    const i2v_cait_config& c = n->cfg;
    float* x0 = n->blocks[0].x;
    VCHK(patch_rows(x, frames, c.in_chans, n->gsz, c.patch, n->pe_w, n->pe_b, c.dim, n->patches, x0, s));
    VCHK(cait_add_pos(x0, n->pos, frames, n->T, c.dim, s));
    return n->forward_blocks(frames, s, [&](int b, float* o) {
        CaitAttn a = n->attn(n->blocks[b], frames);
        a.out = o;
        return cait_attention(a, s);
    });
}

int cait_backward(i2v_cait* n, float* gx, int accumulate, hipStream_t s) {
    const i2v_cait_config& c = n->cfg;
    const int frames = n->frames;
    VCHK(n->backward_blocks(frames, s, [&](int b, const float* dout) {
        CaitAttn a = n->attn(n->blocks[b], frames);
        a.dout = dout; a.dS = n->dS; a.Pm = n->Pm; a.dqkv = n->dqkv;
        return cait_attention_bwd(a, s);
    }));
    // pos_embed is an addend: the patch rows' gradient is the stream's, times the patch weight
    return patch_rows_bwd(n->G, frames, c.in_chans, n->gsz, c.patch, n->pe_w, c.dim, n->patches, gx, accumulate, s);
}

}  // namespace

extern "C" int i2v_cait_create(int device, const i2v_cait_config* cfg, const float* const* weights, int n_weights, const int32_t* hook_blocks,
                               int n_hooks, int max_frames, i2v_cait_handle* out) {
    return xf_create("i2v_cait_create", "block", device, cfg, weights, hook_blocks, max_frames, out, [&](i2v_cait* n) {
        n->cfg = *cfg;
        return cait_plan(n, weights, n_weights, hook_blocks, n_hooks);
    });
}

extern "C" int i2v_cait_destroy(i2v_cait_handle net) { return xf_destroy(net); }

extern "C" int64_t i2v_cait_workspace_bytes(i2v_cait_handle net) { return xf_workspace_bytes(net); }

extern "C" int i2v_cait_forward(i2v_cait_handle n, const float* x, int frames, void* stream) {
    return xf_forward("i2v_cait_forward", n, x, frames, stream, cait_forward);
}

extern "C" int i2v_cait_backward(i2v_cait_handle n, float* gx, int accumulate, void* stream) {
    return xf_backward("i2v_cait_backward", n, gx, accumulate, stream, cait_backward);
}

extern "C" int i2v_cait_hook_info(i2v_cait_handle n, int hook, float** act, int64_t* act_stride, float** grad, int64_t* grad_stride, int64_t* D) {
    return xf_hook_info("i2v_cait_hook_info", n, hook, act, act_stride, grad, grad_stride, D);
}

extern "C" int i2v_cait_read_hook(i2v_cait_handle n, int hook, int which, float* out, int frames, void* stream) {
    return xf_read_hook("i2v_cait_read_hook", n, hook, which, out, frames, stream);
}

// ---- the kernel on its own ----
extern "C" int i2v_cait_attention_f32(const float* qkv, int frames, int T, int heads, int dh, float scale, const float* Wl, const float* bl,
                                      const float* Ww, const float* bw, float* probs, float* out, void* stream) {
    CaitAttn a{};
    a.qkv = qkv; a.F = frames; a.T = T; a.H = heads; a.dh = dh; a.scale = scale;
    a.wl = Wl; a.bl = bl; a.ww = Ww; a.bw = bw; a.P = probs; a.out = out;
    return cait_attention(a, (hipStream_t)stream);
}

extern "C" int i2v_cait_attention_bwd_f32(const float* qkv, const float* probs, const float* dout, int frames, int T, int heads, int dh,
                                          float scale, const float* Wl, const float* Ww, const float* bw, float* ds_scratch, float* pm_scratch,
                                          float* dqkv, void* stream) {
    CaitAttn a{};
    a.qkv = qkv; a.F = frames; a.T = T; a.H = heads; a.dh = dh; a.scale = scale;
    a.wl = Wl; a.ww = Ww; a.bw = bw; a.P = const_cast<float*>(probs); a.dout = dout; a.dS = ds_scratch; a.Pm = pm_scratch; a.dqkv = dqkv;
    return cait_attention_bwd(a, (hipStream_t)stream);
}

extern "C" int i2v_cait_add_pos_f32(float* x, const float* pos, int frames, int T, int C, void* stream) {
    return cait_add_pos(x, pos, frames, T, C, (hipStream_t)stream);
}
