// Planner and executor of the TNT surrogates (include/i2v_tnt.h) on the transformer stack: one arena per (net, max frames), the
// forward as a fixed launch sequence up to the deepest hooked block, and the input-gradient pass -- no weight gradients.  Both halves
// of a TNT block are the shared pre-norm block of i2v_xf.h (block_forward / block_backward as they are): the inner half over
// frames g^2 sequences of 16 pixel tokens, in_dim wide, its attention step tnt_attention (i2v_tnt.hip; without -DI2V_HAVE_TNT the
// scalar restatement i2v_tnt_host.h); the outer half over 1 + g^2 tokens, its attention step BEiT's launch without a bias
// (beit_attention, up to 208 tokens).  This file brings the pixel embedding, the patch embedding, the step between the halves, the sizes.
//   embed       rows = tnt_pixel_gather(x) | inner = Linear(rows) (the 7 x 7 convolution) | inner += pixel_pos (tnt_row_add, period 16)
//               patch = LN(Linear(LN(inner as (F g^2, 16 in_dim)))) | outer = [cls; patch] + patch_pos (vit_assemble) into block 0's x
//   block b     inner half: in.x -> the next block's in.x (or inner_top) | t1 = LN(that stream), statistics kept |
//               out.x[:, 1:] += Linear(t1 as (F, g^2, 16 in_dim)) IN PLACE (a batched vit_gemm whose residual is its output: the class
//               row is skipped by the strides) | outer half: out.x -> the next block's out.x (or x_top) | a hooked block that is not the
//               deepest copies that stream aside, because the next block's step adds into it
//   backward    per block from the deepest: the outer half leaves d out.x in G | the hook below, if any, is added to G only AFTER the
//               step's backward has read G (tnt_row_add) | the step: t1 = G[:, 1:] proj (batched), LN backward onto the inner running
//               gradient Gi (written at the deepest block, which gets gradient only through this step; added below it) | the inner
//               half on Gi.  At the foot: the class row stripped (a 2-D copy), LN, Linear, LN backward added to Gi, the pixel Linear's
//               backward into the rows, tnt_pixel_scatter.
// saved per block: both halves' x, qkv, y, h and four LayerNorm statistics per token, two statistics per pixel token for the step.
// Nothing of either attention core is saved.
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>

#include "../../include/i2v_tnt.h"
#include "i2v_xf.h"
#ifdef I2V_HAVE_TNT
#include "i2v_tnt_kernels.h"
#else
#include "i2v_tnt_host.h"       // (the host simulation's one-file build: the launches as scalar code)
#endif
#ifdef I2V_HAVE_BEIT
#include "i2v_beit_kernels.h"
#else
#include "i2v_beit_host.h"
#endif

namespace {

struct TntBlock {
    Block in, out;
    const float *pnw = nullptr, *pnb = nullptr, *pw = nullptr, *pb = nullptr;      // the step: norm1_proj, proj
    float *pmean = nullptr, *prstd = nullptr;
    float* hook_copy = nullptr;            // the stream behind the block, kept aside when a hook that is not the deepest reads it
};

}  // namespace

struct i2v_tnt : XfNet {
    i2v_tnt_config cfg{};
    int nb = 0, g = 0, np = 0, T = 0, Kp = 0, dh_in = 0, dh_out = 0;
    std::vector<TntBlock> blocks;
    const float *pxw = nullptr, *pxb = nullptr, *ppos = nullptr, *n1w = nullptr, *n1b = nullptr, *prw = nullptr, *prb = nullptr, *n2w = nullptr,
                *n2b = nullptr, *cls = nullptr, *pos = nullptr;
    float *rows = nullptr, *emb = nullptr, *stat = nullptr, *inner_top = nullptr, *x_top = nullptr, *Gi = nullptr;

    int64_t R(int frames) const { return (int64_t)frames * np * 16; }               // pixel tokens
    float* inner_after(int b) { return b + 1 < nb ? blocks[b + 1].in.x : inner_top; }
    float* outer_after(int b) { return b + 1 < nb ? blocks[b + 1].out.x : x_top; }
    float* hook_stream(int b) { return blocks[b].hook_copy ? blocks[b].hook_copy : outer_after(b); }
    int64_t hook_floats(int) const { return (int64_t)T * cfg.dim; }
    BlockRun run_in(int frames, hipStream_t s) const {
        return {frames * np, 16, cfg.in_dim, cfg.mlp_ratio * cfg.in_dim, (int64_t)max_frames * np * 16, cfg.ln_eps, t1, t2, dqkv, Gi, s};
    }
    BlockRun run_out(int frames, hipStream_t s) const {
        return {frames, T, cfg.dim, cfg.mlp_ratio * cfg.dim, (int64_t)max_frames * T, cfg.ln_eps, t1, t2, dqkv, G, s};
    }
    // the step's Linear over a frame's patches, reading or writing the outer stream behind its class row: C (+)= A W^T per frame
    VitGemm step(int frames, const float* A, int64_t a_bo, int64_t a_sm, int K, const float* W, int64_t b_sk, int64_t b_sn, float* Cm, int64_t c_bo,
                 int64_t c_sm, int N) const {
        VitGemm q{};
        q.A = A; q.a_bo = a_bo; q.a_sm = a_sm; q.a_sk = 1;
        q.B = W; q.b_sk = b_sk; q.b_sn = b_sn;
        q.C = Cm; q.c_bo = c_bo; q.c_sm = c_sm;
        q.M = np; q.N = N; q.K = K; q.batch = frames; q.nb_in = 1; q.alpha = 1.f; q.mode = VIT_EPI_PLAIN;
        return q;
    }
};

namespace {

int tnt_plan(i2v_tnt* n, const float* const* w, int nw, const int32_t* hooks, int n_hooks) {
    const i2v_tnt_config& c = n->cfg;
    Arena& A = n->arena;
    if (c.img <= 0 || c.img % 16 != 0 || c.in_chans <= 0 || (c.img / 16) * (c.img / 16) + 1 > BEIT_MAX_T)
        return fail("i2v_tnt_create: unsupported configuration (img %d: a multiple of 16 with at most %d outer tokens; %d input channels)", c.img,
                    (int)BEIT_MAX_T, c.in_chans);
    if (c.in_dim <= 0 || c.in_heads <= 0 || c.in_dim % c.in_heads != 0 || c.in_dim % 4 != 0 || c.in_dim / c.in_heads > TNT_MAX_DH || c.in_heads > TNT_MAX_H)
        return fail("i2v_tnt_create: inner width %d under %d heads: a multiple of 4, up to %d heads up to %d wide", c.in_dim, c.in_heads,
                    (int)TNT_MAX_H, (int)TNT_MAX_DH);
    if (c.dim <= 0 || c.heads <= 0 || c.dim % c.heads != 0 || (c.dim / c.heads) % 4 != 0 || c.dim / c.heads > BEIT_MAX_DH)
        return fail("i2v_tnt_create: outer width %d under %d heads: the head width must be a multiple of 4 up to %d", c.dim, c.heads, (int)BEIT_MAX_DH);
    if (c.mlp_ratio <= 0 || c.blocks <= 0) return fail("i2v_tnt_create: MLP ratio %d and %d blocks must be positive", c.mlp_ratio, c.blocks);
    const int deepest = Hooks::deepest(hooks, n_hooks, c.blocks, A);
    if (deepest < 0) return 1;
    n->nb = A.depth = deepest + 1;
    n->g = c.img / 16; n->np = n->g * n->g; n->T = n->np + 1; n->Kp = tnt_pixel_cols(c.in_chans);
    n->dh_in = c.in_dim / c.in_heads; n->dh_out = c.dim / c.heads;
    // every size of the plan in floats, in 64 bits, before the first allocation
    const int64_t F = n->max_frames, d = c.in_dim, D = c.dim, Mi = c.mlp_ratio * d, M = c.mlp_ratio * D, R = n->R(n->max_frames), FT = F * n->T,
                  FP = F * n->np, Kp = n->Kp;
    std::vector<int64_t> sizes = {d * Kp, d, 16 * d, 16 * d, 16 * d, D * 16 * d, D, D, D, D, n->T * D};
    for (int b = 0; b < n->nb; ++b)
        for (int64_t v : {d, d, 3 * d * d, 3 * d, d * d, d, d, d, Mi * d, Mi, d * Mi, d, d, d, D * 16 * d, D, D, D, 3 * D * D, 3 * D, D * D, D, D, D, M * D,
                          M, D * M, D})
            sizes.push_back(v);
    if ((int)sizes.size() != nw) return fail("i2v_tnt_create: %d weight arrays given, %zu expected for %d blocks", nw, sizes.size(), n->nb);
    const int64_t mS = std::max(R * d, FT * D), mM = std::max(R * Mi, FT * M);
    int64_t acts = n->nb * (5 * R * d + R * Mi + 4 * R + 2 * R + 5 * FT * D + FT * M + 4 * FT);      // per block: both halves' saves, the step's statistics
    acts += R * d + FT * D + FP * D + 4 * FP;                                // inner_top, x_top, the patch embedding before its LayerNorm, its statistics
    acts += mS + mM + 3 * mS + FT * D + R * d + R * Kp;                      // t1; t2; dqkv; G; Gi; the pixel rows
    for (int i = 0; i < n_hooks; ++i) acts += FT * D * (hooks[i] != deepest ? 2 : 1);
    int64_t total = acts;
    for (int64_t v : sizes) total += v;
    VCHK(A.plan(total, R));
    if (3 * mS >= (1ll << 31) || mM >= (1ll << 31) || R * Kp >= (1ll << 31) || F > 65535)
        return fail("i2v_tnt_create: %lld bytes needed: too many frames for one net", (long long)A.planned);
    std::vector<const float*> dev;
    VCHK(A.upload(sizes, w, dev));
    n->pxw = dev[0]; n->pxb = dev[1]; n->ppos = dev[2]; n->n1w = dev[3]; n->n1b = dev[4]; n->prw = dev[5]; n->prb = dev[6]; n->n2w = dev[7];
    n->n2b = dev[8]; n->cls = dev[9]; n->pos = dev[10];
    n->blocks.resize(n->nb);
    for (int b = 0; b < n->nb; ++b) {
        TntBlock& B = n->blocks[b];
        const float* const* a = &dev[11 + 28 * (size_t)b];
        B.in.weights(a, a + 4);
        B.pnw = a[12]; B.pnb = a[13]; B.pw = a[14]; B.pb = a[15];
        B.out.weights(a + 16, a + 20);
        VCHK(B.in.alloc_saves(A, R, d, Mi, 0));
        if (!(B.pmean = A.alloc(R)) || !(B.prstd = A.alloc(R))) return A.oom("the statistics of a block's step");
        VCHK(B.out.alloc_saves(A, FT, D, M, 0));
    }
    if (!(n->inner_top = A.alloc(R * d)) || !(n->x_top = A.alloc(FT * D)) || !(n->emb = A.alloc(FP * D)) || !(n->stat = A.alloc(4 * FP)))
        return A.oom("the top streams and the patch embedding");
    if (!(n->t1 = A.alloc(mS)) || !(n->t2 = A.alloc(mM)) || !(n->dqkv = A.alloc(3 * mS)) || !(n->G = A.alloc(FT * D)) || !(n->Gi = A.alloc(R * d)) ||
        !(n->rows = A.alloc(R * Kp)))
        return A.oom("scratch");
    for (int i = 0; i < n_hooks; ++i) {
        VCHK(n->hooks.add(A, hooks[i], FT * D));
        if (hooks[i] != deepest && !(n->blocks[hooks[i]].hook_copy = A.alloc(FT * D))) return A.oom("a hooked stream");
    }
    return 0;
}

TntAttn inner_attn(const i2v_tnt* n, const Block& B, int frames) {
    TntAttn a{};
    a.qkv = B.qkv; a.S = (int64_t)frames * n->np; a.T = 16; a.H = n->cfg.in_heads; a.dh = n->dh_in; a.scale = 1.f / sqrtf((float)n->dh_in);
    return a;
}

BeitAttn outer_attn(const i2v_tnt* n, const Block& B, int frames) {
    BeitAttn a{};
    a.qkv = B.qkv; a.F = frames; a.T = n->T; a.H = n->cfg.heads; a.dh = n->dh_out; a.scale = 1.f / sqrtf((float)n->dh_out);
    return a;
}

int tnt_forward(i2v_tnt* n, const float* x, int frames, hipStream_t s) {
    const i2v_tnt_config& c = n->cfg;
    const int d = c.in_dim, D = c.dim, np = n->np, T = n->T, FP = frames * np;
    const int64_t R = n->R(frames), sp = (int64_t)n->max_frames * np;
    TntPixels px{x, n->rows, frames, c.in_chans, c.img, 0};
    VCHK(tnt_pixel_gather(px, s));
    float* inner = n->blocks[0].in.x;
    VCHK(linear(n->rows, (int)R, n->Kp, n->pxw, n->pxb, d, nullptr, inner, nullptr, s));
    VCHK(tnt_row_add(inner, n->ppos, R, d, 16, s));
    VCHK(vit_layernorm(inner, FP, 16 * d, n->n1w, n->n1b, c.ln_eps, n->t1, n->stat, n->stat + sp, s));
    VCHK(linear(n->t1, FP, 16 * d, n->prw, n->prb, D, nullptr, n->emb, nullptr, s));
    VCHK(vit_layernorm(n->emb, FP, D, n->n2w, n->n2b, c.ln_eps, n->t2, n->stat + 2 * sp, n->stat + 3 * sp, s));
    VCHK(vit_assemble(n->t2, n->cls, 1, n->pos, n->blocks[0].out.x, frames, T, D, s));
    const BlockRun ri = n->run_in(frames, s), ro = n->run_out(frames, s);
    for (int b = 0; b < n->nb; ++b) {
        const TntBlock& B = n->blocks[b];
        float* nxt = n->inner_after(b);
        VCHK(block_forward(B.in, ri, nxt, [&](const Block& K, float* o) {
            TntAttn a = inner_attn(n, K, frames);
            a.out = o;
            return tnt_attention(a, s);
        }));
        VCHK(vit_layernorm(nxt, R, d, B.pnw, B.pnb, c.ln_eps, n->t1, B.pmean, B.prstd, s));
        VitGemm q = n->step(frames, n->t1, (int64_t)np * 16 * d, 16 * d, 16 * d, B.pw, 1, 16 * d, B.out.x + D, (int64_t)T * D, D, D);
        q.bias = B.pb; q.R = q.C;                                 // in place: the element's own thread reads it, then stores it
        VCHK(vit_gemm(q, s));
        VCHK(block_forward(B.out, ro, n->outer_after(b), [&](const Block& K, float* o) {
            BeitAttn a = outer_attn(n, K, frames);
            a.out = o;
            return beit_attention(a, s);
        }));
        if (B.hook_copy) HCHK(hipMemcpyAsync(B.hook_copy, n->outer_after(b), (size_t)frames * T * D * 4, hipMemcpyDeviceToDevice, s));
    }
    return 0;
}

int tnt_backward(i2v_tnt* n, float* gx, int accumulate, hipStream_t s) {
    const i2v_tnt_config& c = n->cfg;
    const int frames = n->frames, d = c.in_dim, D = c.dim, np = n->np, T = n->T, FP = frames * np;
    const int64_t R = n->R(frames), sp = (int64_t)n->max_frames * np;
    const BlockRun ri = n->run_in(frames, s), ro = n->run_out(frames, s);
    for (int b = n->nb - 1; b >= 0; --b) {
        const TntBlock& B = n->blocks[b];
        const bool top = b == n->nb - 1;
        VCHK(block_backward(B.out, ro, top ? n->hooks.grad_at(b) : n->G, nullptr, [&](const Block& K, const float* dout) {
            BeitAttn a = outer_attn(n, K, frames);
            a.dout = dout; a.dqkv = n->dqkv;
            return beit_attention_bwd(a, s);
        }));
        // G = d out.x.  The step: its patch rows times proj, back through norm1_proj onto the inner stream behind the inner half
        VCHK(vit_gemm(n->step(frames, n->G + D, (int64_t)T * D, D, D, B.pw, 16 * d, 1, n->t1, (int64_t)np * 16 * d, 16 * d, 16 * d), s));
        VCHK(vit_layernorm_bwd(n->t1, n->inner_after(b), B.pmean, B.prstd, B.pnw, R, d, top ? nullptr : n->Gi, nullptr, n->Gi, s));
        if (b > 0 && n->hooks.grad_at(b - 1)) VCHK(tnt_row_add(n->G, n->hooks.grad_at(b - 1), (int64_t)frames * T, D, (int64_t)frames * T, s));
        VCHK(block_backward(B.in, ri, n->Gi, nullptr, [&](const Block& K, const float* dout) {
            TntAttn a = inner_attn(n, K, frames);
            a.dout = dout; a.dqkv = n->dqkv;
            return tnt_attention_bwd(a, s);
        }));
    }
    // G: gradient of [cls; patch] + pos; Gi: gradient of the embedded pixels from block 0.  The class row is a parameter's.
    HCHK(hipMemcpy2DAsync(n->t2, (size_t)np * D * 4, n->G + D, (size_t)T * D * 4, (size_t)np * D * 4, (size_t)frames, hipMemcpyDeviceToDevice, s));
    VCHK(vit_layernorm_bwd(n->t2, n->emb, n->stat + 2 * sp, n->stat + 3 * sp, n->n2w, FP, D, nullptr, nullptr, n->t1, s));
    VCHK(linear_bwd(n->t1, FP, D, n->prw, 16 * d, nullptr, n->t2, s));
    VCHK(vit_layernorm_bwd(n->t2, n->blocks[0].in.x, n->stat, n->stat + sp, n->n1w, FP, 16 * d, n->Gi, nullptr, n->Gi, s));
    VCHK(linear_bwd(n->Gi, (int)R, d, n->pxw, n->Kp, nullptr, n->rows, s));
    TntPixels px{n->rows, gx, frames, c.in_chans, c.img, accumulate != 0};
    return tnt_pixel_scatter(px, s);
}

}  // namespace

extern "C" int i2v_tnt_create(int device, const i2v_tnt_config* cfg, const float* const* weights, int n_weights, const int32_t* hook_blocks,
                              int n_hooks, int max_frames, i2v_tnt_handle* out) {
    return xf_create("i2v_tnt_create", "block", device, cfg, weights, hook_blocks, max_frames, out, [&](i2v_tnt* n) {
        n->cfg = *cfg;
        return tnt_plan(n, weights, n_weights, hook_blocks, n_hooks);
    });
}

extern "C" int i2v_tnt_destroy(i2v_tnt_handle net) { return xf_destroy(net); }

extern "C" int64_t i2v_tnt_workspace_bytes(i2v_tnt_handle net) { return xf_workspace_bytes(net); }

extern "C" int i2v_tnt_forward(i2v_tnt_handle n, const float* x, int frames, void* stream) {
    return xf_forward("i2v_tnt_forward", n, x, frames, stream, tnt_forward);
}

extern "C" int i2v_tnt_backward(i2v_tnt_handle n, float* gx, int accumulate, void* stream) {
    return xf_backward("i2v_tnt_backward", n, gx, accumulate, stream, tnt_backward);
}

extern "C" int i2v_tnt_hook_info(i2v_tnt_handle n, int hook, float** act, int64_t* act_stride, float** grad, int64_t* grad_stride, int64_t* D) {
    return xf_hook_info("i2v_tnt_hook_info", n, hook, act, act_stride, grad, grad_stride, D);
}

extern "C" int i2v_tnt_read_hook(i2v_tnt_handle n, int hook, int which, float* out, int frames, void* stream) {
    return xf_read_hook("i2v_tnt_read_hook", n, hook, which, out, frames, stream);
}

// ---- the kernels on their own ----
extern "C" int i2v_tnt_attention_f32(const float* qkv, int64_t seqs, int T, int heads, int dh, float scale, float* out, void* stream) {
    TntAttn a{};
    a.qkv = qkv; a.S = seqs; a.T = T; a.H = heads; a.dh = dh; a.scale = scale; a.out = out;
    return tnt_attention(a, (hipStream_t)stream);
}

extern "C" int i2v_tnt_attention_bwd_f32(const float* qkv, const float* dout, int64_t seqs, int T, int heads, int dh, float scale, float* dqkv,
                                         void* stream) {
    TntAttn a{};
    a.qkv = qkv; a.S = seqs; a.T = T; a.H = heads; a.dh = dh; a.scale = scale; a.dout = dout; a.dqkv = dqkv;
    return tnt_attention_bwd(a, (hipStream_t)stream);
}

extern "C" int i2v_tnt_attention_group(int T, int heads, int dh) {
    if (T < 1 || T > TNT_MAX_T || heads < 1 || heads > TNT_MAX_H || dh < 1 || dh > TNT_MAX_DH) return 0;
    return tnt_group(T, heads, dh);
}

extern "C" int i2v_tnt_pixel_gather_f32(const float* x, int frames, int in_chans, int side, float* rows, void* stream) {
    TntPixels p{x, rows, frames, in_chans, side, 0};
    return tnt_pixel_gather(p, (hipStream_t)stream);
}

extern "C" int i2v_tnt_pixel_scatter_f32(const float* rows, int frames, int in_chans, int side, int accumulate, float* dx, void* stream) {
    TntPixels p{rows, dx, frames, in_chans, side, accumulate != 0};
    return tnt_pixel_scatter(p, (hipStream_t)stream);
}
