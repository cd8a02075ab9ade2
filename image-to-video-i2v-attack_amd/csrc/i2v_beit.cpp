// Planner and executor of the BEiT surrogates (include/i2v_beit.h) on the transformer stack: one arena per (net, max frames), the
// forward as a fixed launch sequence up to the deepest hook, and the input-gradient pass -- no weight gradients.  A BEiT block is the
// shared pre-norm block of i2v_xf.h once the weights are packed (the qkv bias built from q_bias / v_bias, LayerScale folded into proj and
// fc2, the relative position bias dense as (heads, T, T): BeitSpec.native_arrays), so block_forward / block_backward are used as they
// are and this file brings the embedding without a position table, the sizes, and the attention step: beit_attention (i2v_beit.hip;
// without -DI2V_HAVE_BEIT the scalar restatement i2v_beit_host.h).
// saved per block: x, qkv, y, h and four LayerNorm statistics per token.  Nothing of the attention core is saved.
// I2V_BEIT_ATTN=0, read when a net is planned, runs the core of every block as the shared launches instead of beit_attention:
//   forward   P = softmax(scale q k^T + B) (batched vit_gemm over frames x heads, beit_bias_add, the row softmax) kept per block |
//             t1 = P v (vit_gemm)
//   backward  dS = softmax'(dout v^T; P) | dq = dS k | dk = dS^T q | dv = P^T dout   (four vit_gemm launches and the softmax backward)
// at the cost of T x ld floats per head, frame and block for P (ld = T rounded up to 4), one such array of scratch and per block the
// bias padded to (heads, T, ld).  A developer switch: the baseline the kernel is measured against and a second implementation to test
// against.
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>

#include "../../include/i2v_beit.h"
#include "i2v_xf.h"
#ifdef I2V_HAVE_BEIT
#include "i2v_beit_kernels.h"
#else
#include "i2v_beit_host.h"      // (the host simulation's one-file build: the launches as scalar code)
#endif

namespace {

int beit_probs_ld(int T) { return (T + 3) / 4 * 4; }

// C[f, h] (M, N) = alpha A[f, h] (M, K) B[f, h] (K, N) over batch = frames x heads (outer = frame, inner = head)
int beit_bgemm(const float* A, int64_t a_bo, int64_t a_bi, int64_t a_sm, int64_t a_sk, const float* B, int64_t b_bo, int64_t b_bi, int64_t b_sk,
               int64_t b_sn, float* C, int64_t c_bo, int64_t c_bi, int64_t c_sm, int M, int N, int K, int frames, int heads, float alpha,
               hipStream_t s) {
    VitGemm g{};
    g.A = A; g.a_bo = a_bo; g.a_bi = a_bi; g.a_sm = a_sm; g.a_sk = a_sk;
    g.B = B; g.b_bo = b_bo; g.b_bi = b_bi; g.b_sk = b_sk; g.b_sn = b_sn;
    g.C = C; g.c_bo = c_bo; g.c_bi = c_bi; g.c_sm = c_sm;
    g.M = M; g.N = N; g.K = K; g.batch = frames * heads; g.nb_in = heads; g.alpha = alpha;
    g.mode = VIT_EPI_PLAIN;
    return vit_gemm(g, s);
}

// The attention core on the shared launches (I2V_BEIT_ATTN=0): out = softmax(scale q k^T + B) v with P (F, heads, T, ld) kept;
// `biasp`: the bias padded to (heads, T, ld)
int beit_composed(const float* qkv, const float* biasp, int F, int T, int heads, int dh, float scale, float* P, float* out, hipStream_t s) {
    const int C = heads * dh, ld = beit_probs_ld(T);
    const int64_t qs = 3LL * C * T, ps = (int64_t)T * ld;
    VCHK(beit_bgemm(qkv, qs, dh, 3 * C, 1, qkv + C, qs, dh, 1, 3 * C, P, heads * ps, ps, ld, T, T, dh, F, heads, scale, s));
    VCHK(beit_bias_add(P, biasp, F, heads * ps, s));
    VCHK(beit_softmax(P, (int64_t)F * heads * T, T, ld, s));
    return beit_bgemm(P, heads * ps, ps, ld, 1, qkv + 2 * C, qs, dh, 3 * C, 1, out, (int64_t)T * C, dh, C, T, dh, T, F, heads, 1.f, s);
}

// ... and its backward: dout -> dqkv, with dS (F, heads, T, ld) as scratch
int beit_composed_bwd(const float* qkv, const float* P, const float* dout, int F, int T, int heads, int dh, float scale, float* dS, float* dqkv,
                      hipStream_t s) {
    const int C = heads * dh, ld = beit_probs_ld(T);
    const int64_t qs = 3LL * C * T, ps = (int64_t)T * ld, os = (int64_t)T * C;
    VCHK(beit_bgemm(dout, os, dh, C, 1, qkv + 2 * C, qs, dh, 1, 3 * C, dS, heads * ps, ps, ld, T, T, dh, F, heads, 1.f, s));      // dP = dout v^T
    VCHK(beit_softmax_bwd(dS, P, (int64_t)F * heads * T, T, ld, scale, s));
    VCHK(beit_bgemm(dS, heads * ps, ps, ld, 1, qkv + C, qs, dh, 3 * C, 1, dqkv, qs, dh, 3 * C, T, dh, T, F, heads, 1.f, s));      // dq = dS k
    VCHK(beit_bgemm(dS, heads * ps, ps, 1, ld, qkv, qs, dh, 3 * C, 1, dqkv + C, qs, dh, 3 * C, T, dh, T, F, heads, 1.f, s));      // dk = dS^T q
    return beit_bgemm(P, heads * ps, ps, 1, ld, dout, os, dh, C, 1, dqkv + 2 * C, qs, dh, 3 * C, T, dh, T, F, heads, 1.f, s);     // dv = P^T dout
}

// the patch rows' gradient is the token gradient without the class row (a slice from row 1 of each frame, read in place by the GEMM),
// times W
int beit_embed_bwd(const float* dtok, int F, int Cin, int gsz, int P, const float* W, int dim, float* patches, float* gimg, int accumulate,
                   hipStream_t s) {
    const int np = gsz * gsz, KP = Cin * P * P;
    VitGemm g{};
    g.A = dtok + dim; g.a_bo = (int64_t)(np + 1) * dim; g.a_sm = dim; g.a_sk = 1;
    g.B = W; g.b_sk = KP; g.b_sn = 1;
    g.C = patches; g.c_bo = (int64_t)np * KP; g.c_sm = KP;
    g.M = np; g.N = KP; g.K = dim; g.batch = F; g.nb_in = 1; g.alpha = 1.f;
    VCHK(vit_gemm(g, s));
    return vit_patchify(nullptr, patches, F, Cin, gsz, gsz, P, gimg, accumulate, s);
}

}  // namespace

struct i2v_beit : XfNet {
    i2v_beit_config cfg{};
    int T = 0, gsz = 0, nb = 0, ld = 0;
    float scale = 0.f;
    const float *pe_w = nullptr, *pe_b = nullptr, *cls = nullptr, *zpos = nullptr;
    std::vector<Block> blocks;
    std::vector<const float*> bias, biasp;       // per block: the dense (heads, T, T) bias; padded to (heads, T, ld) on the composed route
    float* x_top = nullptr;                      // stream after the last block run
    float *patches = nullptr, *emb = nullptr;
    bool composed = false;                       // I2V_BEIT_ATTN=0 at plan time: the core on the shared launches, P saved per block
    float* dS = nullptr;                         // ... and its score-gradient scratch

    float* stream_after(int b) { return b + 1 < nb ? blocks[b + 1].x : x_top; }
    BlockRun run(int frames, hipStream_t s) const {
        return {frames, T, cfg.dim, cfg.mlp, (int64_t)max_frames * T, cfg.ln_eps, t1, t2, dqkv, G, s};
    }
    BeitAttn attn(int b, int frames) const {
        BeitAttn a{};
        a.qkv = blocks[b].qkv; a.bias = bias[b]; a.F = frames; a.T = T; a.H = cfg.heads; a.dh = cfg.dim / cfg.heads; a.scale = scale;
        return a;
    }
};

namespace {

int beit_plan(i2v_beit* n, const float* const* w, int nw, const int32_t* hooks, int n_hooks) {
    const i2v_beit_config& c = n->cfg;
    Arena& A = n->arena;
    if (c.img <= 0 || c.patch <= 0 || c.img % c.patch != 0 || c.patch % 4 != 0 || c.in_chans <= 0 || c.dim <= 0 || c.heads <= 0 ||
        c.dim % c.heads != 0 || c.dim % 4 != 0 || c.mlp <= 0 || c.mlp % 4 != 0 || c.blocks <= 0)
        return fail("i2v_beit_create: unsupported configuration (img %d patch %d dim %d heads %d mlp %d blocks %d)", c.img, c.patch, c.dim, c.heads,
                    c.mlp, c.blocks);
    const int dh = c.dim / c.heads;
    if (dh % 4 != 0 || dh > BEIT_MAX_DH) return fail("i2v_beit_create: heads of width %d: a multiple of 4 up to %d", dh, (int)BEIT_MAX_DH);
    n->gsz = c.img / c.patch;
    const int64_t Tl = 1 + (int64_t)n->gsz * n->gsz;
    if (Tl > BEIT_MAX_T)
        return fail("i2v_beit_create: %lld tokens: one head's K and V are staged whole, up to %d tokens", (long long)Tl, (int)BEIT_MAX_T);
    const int deepest = Hooks::deepest(hooks, n_hooks, c.blocks, A);
    if (deepest < 0) return 1;
    n->nb = A.depth = deepest + 1;
    if (nw != 3 + 13 * n->nb) return fail("i2v_beit_create: %d weight arrays given, %d expected for %d blocks", nw, 3 + 13 * n->nb, n->nb);
    n->T = (int)Tl;
    n->ld = beit_probs_ld(n->T);
    n->scale = 1.f / sqrtf((float)dh);                    // dh^-0.5 (exactly 0.125 for dh = 64)
    const char* sw = getenv("I2V_BEIT_ATTN");
    n->composed = sw && !strcmp(sw, "0");
    const int64_t D = c.dim, T = n->T, F = n->max_frames, KP = (int64_t)c.in_chans * c.patch * c.patch, H = c.heads;
    std::vector<int64_t> sizes = {D * KP, D, D};
    for (int b = 0; b < n->nb; ++b)
        for (int64_t v : {D, D, 3 * D * D, 3 * D, H * T * T, D * D, D, D, D, (int64_t)c.mlp * D, (int64_t)c.mlp, D * c.mlp, D}) sizes.push_back(v);
    // the whole plan in floats, in 64 bits, before the first allocation: weights, per-block saves, shared scratch, hook gradients
    const int64_t FT = F * T, Hm = c.mlp, NPt = T - 1, probs = n->composed ? F * H * T * n->ld : 0, padded = n->composed ? H * T * n->ld : 0;
    const int64_t per_block = FT * D + FT * 3 * D + FT * D + FT * Hm + 4 * FT + probs + padded;
    const int64_t shared = FT * D + FT * D + FT * Hm + FT * 3 * D + FT * D + F * NPt * KP + F * NPt * D + T * D + probs;
    int64_t total = n->nb * per_block + shared + (int64_t)n_hooks * FT * D;
    for (int64_t v : sizes) total += v;
    VCHK(A.plan(total, FT));
    if (3 * FT * D >= (1ll << 31) || FT * Hm >= (1ll << 31) || probs >= (1ll << 31) || F > 65535 || (n->composed && F * H > 65535))
        return fail("i2v_beit_create: %lld bytes needed: too many frames for one net", (long long)A.planned);
    std::vector<const float*> dev;
    VCHK(A.upload(sizes, w, dev));
    n->pe_w = dev[0]; n->pe_b = dev[1]; n->cls = dev[2];
    n->blocks.resize(n->nb);
    n->bias.resize(n->nb);
    n->biasp.resize(n->nb);
    for (int b = 0; b < n->nb; ++b) {
        Block& B = n->blocks[b];
        B.weights(&dev[3 + 13 * b], &dev[8 + 13 * b]);    // (the dense bias sits between the qkv bias and proj)
        n->bias[b] = dev[7 + 13 * b];
        if (!(B.x = A.alloc(FT * D)) || !(B.qkv = A.alloc(FT * 3 * D)) || !(B.y = A.alloc(FT * D)) || !(B.h = A.alloc(FT * Hm)) ||
            !(B.stats = A.alloc(4 * FT)))
            return A.oom("saved activations of a block");
        if (n->composed) {
            float* bp = A.alloc(padded);
            if (!(B.P = A.alloc(probs)) || !bp) return A.oom("saved probabilities of a block");
            std::vector<float> host((size_t)padded, 0.f);
            const float* src = w[7 + 13 * b];
            for (int64_t row = 0; row < H * T; ++row) memcpy(&host[(size_t)(row * n->ld)], src + row * T, (size_t)T * 4);
            HCHK(hipMemcpy(bp, host.data(), host.size() * 4, hipMemcpyHostToDevice));
            n->biasp[b] = bp;
        }
    }
    float* z = nullptr;
    if (!(n->x_top = A.alloc(FT * D)) || !(n->t1 = A.alloc(FT * D)) || !(n->t2 = A.alloc(FT * Hm)) || !(n->dqkv = A.alloc(FT * 3 * D)) ||
        !(n->G = A.alloc(FT * D)) || !(n->patches = A.alloc(F * NPt * KP)) || !(n->emb = A.alloc(F * NPt * D)) || !(z = A.alloc(T * D)))
        return A.oom("scratch");
    if (probs && !(n->dS = A.alloc(probs))) return A.oom("scratch");
    HCHK(hipMemset(z, 0, (size_t)(T * D) * 4));           // the position table the assemble launch takes: BEiT has none
    n->zpos = z;
    for (int i = 0; i < n_hooks; ++i) VCHK(n->hooks.add(A, hooks[i], FT * D));
    return 0;
}

}  // namespace

extern "C" int i2v_beit_create(int device, const i2v_beit_config* cfg, const float* const* weights, int n_weights, const int32_t* hook_blocks,
                               int n_hooks, int max_frames, i2v_beit_handle* out) {
    if (!cfg || !weights || !hook_blocks || !out) return fail("i2v_beit_create: null argument");
    return create_net("i2v_beit_create", "block", device, max_frames, out, [&](i2v_beit* n) {
        n->cfg = *cfg;
        return beit_plan(n, weights, n_weights, hook_blocks, n_hooks);
    });
}

extern "C" int i2v_beit_destroy(i2v_beit_handle net) {
    delete net;
    return 0;
}

extern "C" int64_t i2v_beit_workspace_bytes(i2v_beit_handle net) { return net ? net->arena.bytes : -1; }

extern "C" int i2v_beit_forward(i2v_beit_handle n, const float* x, int frames, void* stream) {
    if (!n || !x) return fail("i2v_beit_forward: null argument");
    if (frames <= 0 || frames > n->max_frames) return fail("i2v_beit_forward: %d frames, the net is planned for 1..%d", frames, n->max_frames);
    hipStream_t s = (hipStream_t)stream;
    const i2v_beit_config& c = n->cfg;
    const int heads = c.heads, dh = c.dim / heads, np = n->gsz * n->gsz;
    const BlockRun r = n->run(frames, s);
    n->frames = frames;
    VCHK(vit_patchify(x, n->patches, frames, c.in_chans, n->gsz, n->gsz, c.patch, nullptr, 0, s));
    VCHK(linear(n->patches, frames * np, c.in_chans * c.patch * c.patch, n->pe_w, n->pe_b, c.dim, nullptr, n->emb, nullptr, s));
    VCHK(beit_assemble(n->emb, n->cls, n->zpos, n->blocks[0].x, frames, n->T, c.dim, s));
    for (int b = 0; b < n->nb; ++b)
        VCHK(block_forward(n->blocks[b], r, n->stream_after(b), [&](const Block& B, float* o) {
            if (n->composed) return beit_composed(B.qkv, n->biasp[b], frames, n->T, heads, dh, n->scale, B.P, o, s);
            BeitAttn a = n->attn(b, frames);
            a.out = o;
            return beit_attention(a, s);
        }));
    return 0;
}

extern "C" int i2v_beit_backward(i2v_beit_handle n, float* gx, int accumulate, void* stream) {
    if (!n || !gx) return fail("i2v_beit_backward: null argument");
    if (n->frames <= 0) return fail("i2v_beit_backward: no forward pass to differentiate");
    hipStream_t s = (hipStream_t)stream;
    const i2v_beit_config& c = n->cfg;
    const int frames = n->frames, heads = c.heads, dh = c.dim / heads;
    const BlockRun r = n->run(frames, s);
    for (int b = n->nb - 1; b >= 0; --b) {
        // gradient of the stream after block b: the top hook's view for the deepest block, the running gradient G below it (where
        // the LN1 backward of block b + 1 has already added the hook at that stream)
        const float* gin = b == n->nb - 1 ? n->hooks.grad_at(b) : n->G;
        VCHK(block_backward(n->blocks[b], r, gin, b > 0 ? n->hooks.grad_at(b - 1) : nullptr, [&](const Block& B, const float* dout) {
            if (n->composed) return beit_composed_bwd(B.qkv, B.P, dout, frames, n->T, heads, dh, n->scale, n->dS, n->dqkv, s);
            BeitAttn a = n->attn(b, frames);
            a.dout = dout; a.dqkv = n->dqkv;
            return beit_attention_bwd(a, s);
        }));
    }
    return beit_embed_bwd(n->G, frames, c.in_chans, n->gsz, c.patch, n->pe_w, c.dim, n->patches, gx, accumulate, s);
}

extern "C" int i2v_beit_hook_info(i2v_beit_handle n, int hook, float** act, int64_t* act_stride, float** grad, int64_t* grad_stride, int64_t* D) {
    if (!n || !n->hooks.has(hook)) return fail("i2v_beit_hook_info: no hook %d", hook);
    return hook_info(n->stream_after(n->hooks.at[hook]), n->hooks.grad[hook], (int64_t)n->T * n->cfg.dim, act, act_stride, grad, grad_stride, D);
}

extern "C" int i2v_beit_read_hook(i2v_beit_handle n, int hook, int which, float* out, int frames, void* stream) {
    if (!n || !out || !n->hooks.has(hook)) return fail("i2v_beit_read_hook: no hook %d", hook);
    return read_hook("i2v_beit_read_hook", which ? n->hooks.grad[hook] : n->stream_after(n->hooks.at[hook]), (int64_t)n->T * n->cfg.dim, out,
                     frames, n->max_frames, stream);
}

// ---- the kernel on its own ----
extern "C" int i2v_beit_attention_f32(const float* qkv, const float* bias, int frames, int T, int heads, int dh, float scale, float* out,
                                      void* stream) {
    BeitAttn a{};
    a.qkv = qkv; a.bias = bias; a.F = frames; a.T = T; a.H = heads; a.dh = dh; a.scale = scale; a.out = out;
    return beit_attention(a, (hipStream_t)stream);
}

extern "C" int i2v_beit_attention_bwd_f32(const float* qkv, const float* bias, const float* dout, int frames, int T, int heads, int dh,
                                          float scale, float* dqkv, void* stream) {
    BeitAttn a{};
    a.qkv = qkv; a.bias = bias; a.F = frames; a.T = T; a.H = heads; a.dh = dh; a.scale = scale; a.dout = dout; a.dqkv = dqkv;
    return beit_attention_bwd(a, (hipStream_t)stream);
}

extern "C" int i2v_beit_bias_add_f32(float* S, const float* bias, int frames, int64_t per_frame, void* stream) {
    return beit_bias_add(S, bias, frames, per_frame, (hipStream_t)stream);
}
