// Planner and executor of the PiT surrogates (include/i2v_pit.h) on the transformer stack: one arena per (net, max frames), the forward
// as a fixed launch sequence up to the deepest hooked block, and the input-gradient pass -- no weight gradients.  A PiT block is the
// shared pre-norm block of i2v_xf.h (block_forward / block_backward as they are), run stage by stage at the stage's token count and
// width; this file brings the overlapping patch embedding, the pooling between the stages, the sizes, and the attention step:
// pit_attention (i2v_pit.hip; without -DI2V_HAVE_PIT the scalar restatement i2v_pit_host.h).
//   embedding   rows = gather(x) | emb = rows W^T + b | x0 = [cls; emb] + [0; pos]   (vit_assemble)
//   pooling     grid rows: pit_pool into the next stage's stream behind its prefix rows | prefix rows: the shared linear, per frame
//   backward    the same in reverse; a hook behind the last block of a stage is added where the pooling's gradient lands
// saved per block: x, qkv, y, h, four LayerNorm statistics per token, and of the attention core its output and the row log-sum-exp,
// (F, T, D) + (F, H, T) floats.  Per stage: the stream behind its last block.
// I2V_PIT_ATTN=0, read when a net is planned, runs the core of every block as the shared launches instead of pit_attention:
//   forward   P = softmax(scale q k^T) (batched vit_gemm over frames x heads, the row softmax) kept per block | t1 = P v (vit_gemm)
//   backward  dS = softmax'(dout v^T; P) | dq = dS k | dk = dS^T q | dv = P^T dout   (four vit_gemm launches and the softmax backward)
// at the cost of T x ld floats per head, frame and block for P (ld = T rounded up to 4) and one such array of scratch, in place of the
// output and the log-sum-exp.  A developer switch: the yardstick the kernel is measured against and the recourse.
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>

#include "../../include/i2v_pit.h"
#include "i2v_xf.h"
#ifdef I2V_HAVE_PIT
#include "i2v_pit_kernels.h"
#else
#include "i2v_pit_host.h"       // (the host simulation's one-file build: the launches as scalar code)
#endif

namespace {

struct PitBlock : Block {
    int stage = 0;
    float *att = nullptr, *lse = nullptr, *out = nullptr;      // saved attention output and log-sum-exp; the stream behind the block
};

struct PitStage {
    int grid = 0, width = 0, heads = 0, T = 0, first = 0, count = 0;      // first: flat index of its block 0; count: its blocks that run
    const float *pcw = nullptr, *pcb = nullptr, *pfw = nullptr, *pfb = nullptr;      // the pooling BEHIND this stage (when the next one runs)
    float* out = nullptr;                                                 // the stream behind its last block that runs
};

}  // namespace

struct i2v_pit : XfNet {
    i2v_pit_config cfg{};
    int ns = 0, nb = 0, g0 = 0;
    std::vector<PitStage> stages;
    std::vector<PitBlock> blocks;
    const float *pe_w = nullptr, *pe_b = nullptr, *pos = nullptr, *cls = nullptr;
    float *patches = nullptr, *emb = nullptr, *G2 = nullptr, *delta = nullptr, *dS = nullptr;
    bool composed = false;            // I2V_PIT_ATTN=0 at plan time: the core on the shared launches, P saved per block

    float* hook_stream(int b) { return blocks[b].out; }
    int64_t hook_floats(int b) const { const PitStage& S = stages[blocks[b].stage]; return (int64_t)S.T * S.width; }
    BlockRun run(const PitStage& S, int frames, hipStream_t s) const {
        return {frames, S.T, S.width, 4 * S.width, (int64_t)max_frames * S.T, cfg.ln_eps, t1, t2, dqkv, G, s};
    }
    PitAttn attn(const PitBlock& B, int frames) const {
        const PitStage& S = stages[B.stage];
        PitAttn a{};
        a.qkv = B.qkv; a.F = frames; a.T = S.T; a.H = S.heads; a.dh = S.width / S.heads; a.scale = 1.f / sqrtf((float)a.dh);
        a.out = B.att; a.lse = B.lse;
        return a;
    }
    XfAttn shared(const PitBlock& B, int frames) const {
        const PitStage& S = stages[B.stage];
        return xf_attn_qkv(B.qkv, frames, S.T, S.heads, S.width / S.heads, 1.f / sqrtf((float)(S.width / S.heads)));
    }
};

namespace {

// y rows (F frames of `rows` rows at frame stride ys, N wide) = x rows (frame stride xs, K wide) W^T + bias: the shared linear, per frame
int linear_rows(const float* x, int64_t xs, int F, int rows, int K, const float* W, const float* bias, int N, float* y, int64_t ys, hipStream_t s) {
    VitGemm g{};
    g.A = x; g.a_bo = xs; g.a_sm = K; g.a_sk = 1;
    g.B = W; g.b_sk = 1; g.b_sn = K;
    g.C = y; g.c_bo = ys; g.c_sm = N;
    g.bias = bias;
    g.M = rows; g.N = N; g.K = K; g.batch = F; g.nb_in = 1; g.alpha = 1.f;
    g.mode = VIT_EPI_PLAIN;
    return vit_gemm(g, s);
}

// dx rows (frame stride xs, K wide) = dy rows (frame stride ys, N wide) W (+ dx itself with `add`), W (N, K)
int linear_rows_bwd(const float* dy, int64_t ys, int F, int rows, int N, const float* W, int K, bool add, float* dx, int64_t xs, hipStream_t s) {
    VitGemm g{};
    g.A = dy; g.a_bo = ys; g.a_sm = N; g.a_sk = 1;
    g.B = W; g.b_sk = K; g.b_sn = 1;
    g.C = dx; g.c_bo = xs; g.c_sm = K;
    g.R = add ? dx : nullptr;                               // (R may alias C: i2v_vit_kernels.h)
    g.M = rows; g.N = K; g.K = N; g.batch = F; g.nb_in = 1; g.alpha = 1.f;
    g.mode = VIT_EPI_PLAIN;
    return vit_gemm(g, s);
}

int pit_plan(i2v_pit* n, const float* const* w, int nw, const int32_t* hooks, int n_hooks) {
    const i2v_pit_config& c = n->cfg;
    Arena& A = n->arena;
    if (c.img <= 0 || c.in_chans <= 0 || c.patch <= 0 || c.stride <= 0 || c.stride > c.patch || c.patch > c.img ||
        (c.img - c.patch) % c.stride != 0 || (c.in_chans * c.patch * c.patch) % 4 != 0 || c.prefix < 1 || c.prefix > 2)
        return fail("i2v_pit_create: unsupported configuration (img %d patch %d stride %d prefix tokens %d)", c.img, c.patch, c.stride, c.prefix);
    n->g0 = (c.img - c.patch) / c.stride + 1;
    int total_blocks = 0;
    for (int k = 0; k < I2V_PIT_STAGES; ++k) {
        const int D = c.dims[k], H = c.heads[k];
        if (D <= 0 || H <= 0 || D % H != 0 || (D / H) % 4 != 0 || c.depths[k] <= 0 || (k && D != 2 * c.dims[k - 1]))
            return fail("i2v_pit_create: stage %d has width %d, %d heads and %d blocks (a width is twice its predecessor's)", k, D, H, c.depths[k]);
        if (D / H > PIT_MAX_DH) return fail("i2v_pit_create: heads of width %d in stage %d: up to %d", D / H, k, (int)PIT_MAX_DH);
        total_blocks += c.depths[k];
    }
    const int deepest = Hooks::deepest(hooks, n_hooks, total_blocks, A);
    if (deepest < 0) return 1;
    n->nb = A.depth = deepest + 1;
    const char* sw = getenv("I2V_PIT_ATTN");
    n->composed = sw && !strcmp(sw, "0");
    const int64_t F = n->max_frames, KP = (int64_t)c.in_chans * c.patch * c.patch, NP = (int64_t)n->g0 * n->g0;
    // the stages that run, and every size of the plan in floats, in 64 bits, before the first allocation
    n->stages.clear();
    for (int k = 0, first = 0, g = n->g0; k < I2V_PIT_STAGES && first < n->nb; ++k, g = (g - 1) / 2 + 1) {
        PitStage S;
        S.grid = g; S.width = c.dims[k]; S.heads = c.heads[k]; S.T = c.prefix + g * g; S.first = first;
        S.count = std::min(c.depths[k], n->nb - first);
        n->stages.push_back(S);
        first += c.depths[k];
    }
    n->ns = (int)n->stages.size();
    std::vector<int64_t> sizes = {c.dims[0] * KP, c.dims[0], (c.prefix + NP) * c.dims[0], (int64_t)c.prefix * c.dims[0]};
    int64_t acts = 0, mFTD = 0, mStat = 0, mP = 0;
    for (int k = 0; k < n->ns; ++k) {
        const PitStage& S = n->stages[k];
        const int64_t D = S.width, FT = F * S.T, H = S.heads;
        const int64_t probs = n->composed ? F * H * S.T * xf_probs_ld(S.T) : 0, core = n->composed ? probs : FT * D + F * H * S.T;
        for (int b = 0; b < S.count; ++b) {
            for (int64_t v : {D, D, 3 * D * D, 3 * D, D * D, D, D, D, 4 * D * D, 4 * D, 4 * D * D, D}) sizes.push_back(v);
            acts += FT * D + 3 * FT * D + FT * D + 4 * FT * D + 4 * FT + core;      // x, qkv, y, h, statistics, the core's saves
        }
        if (k + 1 < n->ns)
            for (int64_t v : {2 * D * 9, 2 * D, 2 * D * D, 2 * D}) sizes.push_back(v);
        acts += FT * D;                                                     // the stream behind the stage
        mFTD = std::max(mFTD, FT * D); mStat = std::max(mStat, F * H * S.T); mP = std::max(mP, probs);
        if (probs >= (1ll << 31) || (n->composed && F * H > 65535)) mP = 1ll << 31;
    }
    // shared scratch: t1, G, G2; t2 (4 wide); dqkv (3 wide); the patch rows and their embedding; delta or the score gradient
    acts += 3 * mFTD + 4 * mFTD + 3 * mFTD + F * NP * KP + F * NP * c.dims[0] + (n->composed ? mP : mStat);
    for (int i = 0; i < n_hooks; ++i) {
        int k = 0;
        while (k + 1 < n->ns && hooks[i] >= n->stages[k + 1].first) ++k;
        acts += F * n->stages[k].T * n->stages[k].width;
    }
    if ((int)sizes.size() != nw) return fail("i2v_pit_create: %d weight arrays given, %zu expected for %d blocks", nw, sizes.size(), n->nb);
    int64_t total = acts;
    for (int64_t v : sizes) total += v;
    VCHK(A.plan(total, F * n->stages[0].T));
    if (4 * mFTD >= (1ll << 31) || F * NP * KP >= (1ll << 31) || mP >= (1ll << 31) || F > 65535)
        return fail("i2v_pit_create: %lld bytes needed: too many frames for one net", (long long)A.planned);
    std::vector<const float*> dev;
    VCHK(A.upload(sizes, w, dev));
    n->pe_w = dev[0]; n->pe_b = dev[1]; n->pos = dev[2]; n->cls = dev[3];
    size_t wi = 4;
    n->blocks.resize(n->nb);
    for (int k = 0; k < n->ns; ++k) {
        PitStage& S = n->stages[k];
        const int64_t D = S.width, FT = F * S.T, H = S.heads;
        for (int b = 0; b < S.count; ++b) {
            PitBlock& B = n->blocks[S.first + b];
            B.stage = k;
            B.weights(&dev[wi], &dev[wi + 4]);
            wi += 12;
            VCHK(B.alloc_saves(A, FT, D, 4 * D, n->composed ? F * H * S.T * xf_probs_ld(S.T) : 0));
            if (!n->composed && (!(B.att = A.alloc(FT * D)) || !(B.lse = A.alloc(F * H * S.T)))) return A.oom("saved attention output of a block");
        }
        if (k + 1 < n->ns) {
            S.pcw = dev[wi]; S.pcb = dev[wi + 1]; S.pfw = dev[wi + 2]; S.pfb = dev[wi + 3];
            wi += 4;
        }
        if (!(S.out = A.alloc(FT * D))) return A.oom("a stage's output");
        for (int b = 0; b < S.count; ++b) n->blocks[S.first + b].out = b + 1 < S.count ? n->blocks[S.first + b + 1].x : S.out;
    }
    if (!(n->t1 = A.alloc(mFTD)) || !(n->G = A.alloc(mFTD)) || !(n->G2 = A.alloc(mFTD)) || !(n->t2 = A.alloc(4 * mFTD)) ||
        !(n->dqkv = A.alloc(3 * mFTD)) || !(n->patches = A.alloc(F * NP * KP)) || !(n->emb = A.alloc(F * NP * c.dims[0])))
        return A.oom("scratch");
    if (n->composed ? !(n->dS = A.alloc(mP)) : !(n->delta = A.alloc(mStat))) return A.oom("scratch");
    for (int i = 0; i < n_hooks; ++i) VCHK(n->hooks.add(A, hooks[i], F * n->hook_floats(hooks[i])));
    return 0;
}

int pit_forward(i2v_pit* n, const float* x, int frames, hipStream_t s) {
    const i2v_pit_config& c = n->cfg;
    const int NP = n->g0 * n->g0, KP = c.in_chans * c.patch * c.patch;
    PitPatch pp{};
    pp.src = x; pp.dst = n->patches; pp.F = frames; pp.Cin = c.in_chans; pp.side = c.img; pp.p = c.patch; pp.s = c.stride;
    VCHK(pit_patch_gather(pp, s));
    VCHK(linear(n->patches, frames * NP, KP, n->pe_w, n->pe_b, c.dims[0], nullptr, n->emb, nullptr, s));
    VCHK(vit_assemble(n->emb, n->cls, c.prefix, n->pos, n->blocks[0].x, frames, n->stages[0].T, c.dims[0], s));
    for (int k = 0; k < n->ns; ++k) {
        const PitStage& S = n->stages[k];
        const BlockRun r = n->run(S, frames, s);
        const int64_t FTD = (int64_t)frames * S.T * S.width;
        for (int b = 0; b < S.count; ++b) {
            const PitBlock& B = n->blocks[S.first + b];
            VCHK(block_forward(B, r, B.out, [&](const Block&, float* o) {
                if (n->composed) return xf_attention(n->shared(B, frames), B.P, o, s);
                VCHK(pit_attention(n->attn(B, frames), s));                 // out and lse kept for the backward; the block reads a copy
                HCHK(hipMemcpyAsync(o, B.att, (size_t)FTD * 4, hipMemcpyDeviceToDevice, s));
                return 0;
            }));
        }
        if (k + 1 < n->ns) {
            const PitStage& N = n->stages[k + 1];
            float* y = n->blocks[N.first].x;
            PitPool q{};
            q.x = S.out + (int64_t)c.prefix * S.width; q.w = S.pcw; q.b = S.pcb; q.y = y + (int64_t)c.prefix * N.width;
            q.F = frames; q.g = S.grid; q.C = S.width; q.xs = (int64_t)S.T * S.width; q.ys = (int64_t)N.T * N.width;
            VCHK(pit_pool(q, s));
            VCHK(linear_rows(S.out, q.xs, frames, c.prefix, S.width, S.pfw, S.pfb, N.width, y, q.ys, s));
        }
    }
    return 0;
}

int pit_backward(i2v_pit* n, float* gx, int accumulate, hipStream_t s) {
    const i2v_pit_config& c = n->cfg;
    const int frames = n->frames, NP = n->g0 * n->g0, KP = c.in_chans * c.patch * c.patch;
    for (int k = n->ns - 1; k >= 0; --k) {
        const PitStage& S = n->stages[k];
        const BlockRun r = n->run(S, frames, s);
        for (int b = S.count - 1; b >= 0; --b) {
            const int fb = S.first + b;
            const PitBlock& B = n->blocks[fb];
            // gradient of the stream behind block fb: the deepest block's hook view; behind the last block of a lower stage what the
            // pooling's backward left in G2 (the hook there added); the running gradient G otherwise
            const float* gin = fb == n->nb - 1 ? n->hooks.grad_at(fb) : b == S.count - 1 ? n->G2 : n->G;
            const float* add1 = b > 0 ? n->hooks.grad_at(fb - 1) : nullptr;      // (a hook behind the stage below: added by the pooling's backward)
            VCHK(block_backward(B, r, gin, add1, [&](const Block&, const float* dout) {
                const int D = S.width;
                if (n->composed) return xf_attention_bwd(n->shared(B, frames), B.P, dout, n->dS, n->dqkv, n->dqkv + D, n->dqkv + 2 * D, s);
                PitAttn a = n->attn(B, frames);
                a.dout = dout; a.delta = n->delta; a.dqkv = n->dqkv;
                return pit_attention_bwd(a, s);
            }));
        }
        if (k > 0) {                                                        // G: gradient of this stage's input stream; back through the pooling
            const PitStage& Pv = n->stages[k - 1];
            const float* hook = n->hooks.grad_at(S.first - 1);
            const int64_t xs = (int64_t)Pv.T * Pv.width, ys = (int64_t)S.T * S.width;
            if (hook) HCHK(hipMemcpyAsync(n->G2, hook, (size_t)frames * xs * 4, hipMemcpyDeviceToDevice, s));
            PitPool q{};
            q.x = n->G + (int64_t)c.prefix * S.width; q.w = Pv.pcw; q.y = n->G2 + (int64_t)c.prefix * Pv.width;
            q.F = frames; q.g = Pv.grid; q.C = Pv.width; q.xs = xs; q.ys = ys; q.accumulate = hook != nullptr;
            VCHK(pit_pool_bwd(q, s));
            VCHK(linear_rows_bwd(n->G, ys, frames, c.prefix, S.width, Pv.pfw, Pv.width, hook != nullptr, n->G2, xs, s));
        }
    }
    // the patch rows' gradient is the token gradient without the prefix rows (read in place by the GEMM), times W; then the scatter
    VCHK(linear_rows_bwd(n->G + (int64_t)c.prefix * c.dims[0], (int64_t)n->stages[0].T * c.dims[0], frames, NP, c.dims[0], n->pe_w, KP, false,
                         n->patches, (int64_t)NP * KP, s));
    PitPatch pp{};
    pp.src = n->patches; pp.dst = gx; pp.F = frames; pp.Cin = c.in_chans; pp.side = c.img; pp.p = c.patch; pp.s = c.stride; pp.accumulate = accumulate;
    return pit_patch_scatter(pp, s);
}

}  // namespace

extern "C" int i2v_pit_create(int device, const i2v_pit_config* cfg, const float* const* weights, int n_weights, const int32_t* hook_blocks,
                              int n_hooks, int max_frames, i2v_pit_handle* out) {
    return xf_create("i2v_pit_create", "block", device, cfg, weights, hook_blocks, max_frames, out, [&](i2v_pit* n) {
        n->cfg = *cfg;
        return pit_plan(n, weights, n_weights, hook_blocks, n_hooks);
    });
}

extern "C" int i2v_pit_destroy(i2v_pit_handle net) { return xf_destroy(net); }

extern "C" int64_t i2v_pit_workspace_bytes(i2v_pit_handle net) { return xf_workspace_bytes(net); }

extern "C" int i2v_pit_forward(i2v_pit_handle n, const float* x, int frames, void* stream) {
    return xf_forward("i2v_pit_forward", n, x, frames, stream, pit_forward);
}

extern "C" int i2v_pit_backward(i2v_pit_handle n, float* gx, int accumulate, void* stream) {
    return xf_backward("i2v_pit_backward", n, gx, accumulate, stream, pit_backward);
}

extern "C" int i2v_pit_hook_info(i2v_pit_handle n, int hook, float** act, int64_t* act_stride, float** grad, int64_t* grad_stride, int64_t* D) {
    return xf_hook_info("i2v_pit_hook_info", n, hook, act, act_stride, grad, grad_stride, D);
}

extern "C" int i2v_pit_read_hook(i2v_pit_handle n, int hook, int which, float* out, int frames, void* stream) {
    return xf_read_hook("i2v_pit_read_hook", n, hook, which, out, frames, stream);
}

// ---- the kernels on their own ----
extern "C" int i2v_pit_attention_f32(const float* qkv, int frames, int T, int heads, int dh, float scale, float* out, float* lse, void* stream) {
    PitAttn a{};
    a.qkv = qkv; a.F = frames; a.T = T; a.H = heads; a.dh = dh; a.scale = scale; a.out = out; a.lse = lse;
    return pit_attention(a, (hipStream_t)stream);
}

extern "C" int i2v_pit_attention_bwd_f32(const float* qkv, const float* out, const float* lse, const float* dout, int frames, int T, int heads,
                                         int dh, float scale, float* delta, float* dqkv, void* stream) {
    PitAttn a{};
    a.qkv = qkv; a.F = frames; a.T = T; a.H = heads; a.dh = dh; a.scale = scale;
    a.out = const_cast<float*>(out); a.lse = const_cast<float*>(lse);      // (read only by the backward)
    a.dout = dout; a.delta = delta; a.dqkv = dqkv;
    return pit_attention_bwd(a, (hipStream_t)stream);
}

namespace {
PitPool pool_of(const float* x, const float* w, const float* b, int frames, int g, int C, int prefix, float* y, bool bwd) {
    const int64_t go = g > 0 ? (g - 1) / 2 + 1 : 0, pre = prefix > 0 ? prefix : 0;
    PitPool q{};
    q.w = w; q.b = b; q.F = frames; q.g = g; q.C = C;
    q.xs = (pre + (int64_t)g * g) * C; q.ys = (pre + go * go) * 2 * C;
    q.x = x ? x + pre * (bwd ? 2 * C : C) : nullptr;
    q.y = y ? y + pre * (bwd ? C : 2 * C) : nullptr;
    return q;
}
}  // namespace

extern "C" int i2v_pit_pool_f32(const float* x, const float* w, const float* b, int frames, int g, int C, int prefix, float* y, void* stream) {
    if (prefix < 0) return fail("i2v_pit_pool_f32: hipErrorInvalidValue: a negative count of prefix rows");
    return pit_pool(pool_of(x, w, b, frames, g, C, prefix, y, false), (hipStream_t)stream);
}

extern "C" int i2v_pit_pool_bwd_f32(const float* dy, const float* w, int frames, int g, int C, int prefix, int accumulate, float* dx, void* stream) {
    if (prefix < 0) return fail("i2v_pit_pool_bwd_f32: hipErrorInvalidValue: a negative count of prefix rows");
    PitPool q = pool_of(dy, w, nullptr, frames, g, C, prefix, dx, true);
    q.accumulate = accumulate;
    return pit_pool_bwd(q, (hipStream_t)stream);
}

extern "C" int i2v_pit_patch_gather_f32(const float* img, int frames, int in_chans, int side, int p, int s, float* rows, void* stream) {
    PitPatch pp{};
    pp.src = img; pp.dst = rows; pp.F = frames; pp.Cin = in_chans; pp.side = side; pp.p = p; pp.s = s;
    return pit_patch_gather(pp, (hipStream_t)stream);
}

extern "C" int i2v_pit_patch_scatter_f32(const float* rows, int frames, int in_chans, int side, int p, int s, int accumulate, float* gimg,
                                         void* stream) {
    PitPatch pp{};
    pp.src = rows; pp.dst = gimg; pp.F = frames; pp.Cin = in_chans; pp.side = side; pp.p = p; pp.s = s; pp.accumulate = accumulate;
    return pit_patch_scatter(pp, (hipStream_t)stream);
}
