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

struct i2v_beit : XfStack<i2v_beit_config> {
    int ld = 0;
    const float *pe_w = nullptr, *pe_b = nullptr, *cls = nullptr, *zpos = nullptr;
    std::vector<const float*> bias, biasp;       // per block: the dense (heads, T, T) bias; padded to (heads, T, ld) on the composed route
    float *patches = nullptr, *emb = nullptr;
    bool composed = false;                       // I2V_BEIT_ATTN=0 at plan time: the core on the shared launches, P saved per block
    float* dS = nullptr;                         // ... and its score-gradient scratch

    BeitAttn attn(int b, int frames) const {
        BeitAttn a{};
        a.qkv = blocks[b].qkv; a.bias = bias[b]; a.F = frames; a.T = T; a.H = cfg.heads; a.dh = cfg.dim / cfg.heads; a.scale = scale;
        return a;
    }
    XfAttn shared(int b, int frames) const { return xf_attn_qkv(blocks[b].qkv, frames, T, cfg.heads, cfg.dim / cfg.heads, scale); }
};

namespace {

int beit_plan(i2v_beit* n, const float* const* w, int nw, const int32_t* hooks, int n_hooks) {
    const i2v_beit_config& c = n->cfg;
    Arena& A = n->arena;
    if (!vit_shape_ok(c))
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
    n->ld = xf_probs_ld(n->T);
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
        VCHK(B.alloc_saves(A, FT, D, Hm, 0));             // (P of the composed route follows its padded bias, below)
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

int beit_forward(i2v_beit* n, const float* x, int frames, hipStream_t s) {
    const i2v_beit_config& c = n->cfg;
    VCHK(patch_rows(x, frames, c.in_chans, n->gsz, c.patch, n->pe_w, n->pe_b, c.dim, n->patches, n->emb, s));
    VCHK(vit_assemble(n->emb, n->cls, 1, n->zpos, n->blocks[0].x, frames, n->T, c.dim, s));
    return n->forward_blocks(frames, s, [&](int b, float* o) {
        if (n->composed)      // P = softmax(scale q k^T + B): the bias add between the score product and the softmax
            return xf_attention(n->shared(b, frames), n->blocks[b].P, o, s, [&] {
                return beit_bias_add(n->blocks[b].P, n->biasp[b], frames, (int64_t)c.heads * n->T * n->ld, s);
            });
        BeitAttn a = n->attn(b, frames);
        a.out = o;
        return beit_attention(a, s);
    });
}

int beit_backward(i2v_beit* n, float* gx, int accumulate, hipStream_t s) {
    const i2v_beit_config& c = n->cfg;
    const int frames = n->frames;
    VCHK(n->backward_blocks(frames, s, [&](int b, const float* dout) {
        if (n->composed)
            return xf_attention_bwd(n->shared(b, frames), n->blocks[b].P, dout, n->dS, n->dqkv, n->dqkv + c.dim, n->dqkv + 2 * c.dim, s);
        BeitAttn a = n->attn(b, frames);
        a.dout = dout; a.dqkv = n->dqkv;
        return beit_attention_bwd(a, s);
    }));
    return patch_rows_bwd_prefix(n->G, frames, c.in_chans, n->gsz, c.patch, n->pe_w, c.dim, 1, n->patches, gx, accumulate, s);
}

}  // namespace

extern "C" int i2v_beit_create(int device, const i2v_beit_config* cfg, const float* const* weights, int n_weights, const int32_t* hook_blocks,
                               int n_hooks, int max_frames, i2v_beit_handle* out) {
    return xf_create("i2v_beit_create", "block", device, cfg, weights, hook_blocks, max_frames, out, [&](i2v_beit* n) {
        n->cfg = *cfg;
        return beit_plan(n, weights, n_weights, hook_blocks, n_hooks);
    });
}

extern "C" int i2v_beit_destroy(i2v_beit_handle net) { return xf_destroy(net); }

extern "C" int64_t i2v_beit_workspace_bytes(i2v_beit_handle net) { return xf_workspace_bytes(net); }

extern "C" int i2v_beit_forward(i2v_beit_handle n, const float* x, int frames, void* stream) {
    return xf_forward("i2v_beit_forward", n, x, frames, stream, beit_forward);
}

extern "C" int i2v_beit_backward(i2v_beit_handle n, float* gx, int accumulate, void* stream) {
    return xf_backward("i2v_beit_backward", n, gx, accumulate, stream, beit_backward);
}

extern "C" int i2v_beit_hook_info(i2v_beit_handle n, int hook, float** act, int64_t* act_stride, float** grad, int64_t* grad_stride, int64_t* D) {
    return xf_hook_info("i2v_beit_hook_info", n, hook, act, act_stride, grad, grad_stride, D);
}

extern "C" int i2v_beit_read_hook(i2v_beit_handle n, int hook, int which, float* out, int frames, void* stream) {
    return xf_read_hook("i2v_beit_read_hook", n, hook, which, out, frames, stream);
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
