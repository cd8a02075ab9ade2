// Planner and executor of the Twins surrogates (include/i2v_twins.h) on the transformer stack: one arena per (net, max frames), the
// forward as a fixed launch sequence up to the deepest hooked stage, and the input-gradient pass -- no weight gradients.  A Twins block
// takes its keys from a sub-sampled plane, so it is composed here from the shared launches (linear / linear_bwd, the LayerNorm pair,
// patchify, the 2 x 2 merge pair), XCiT's depthwise 3 x 3 and the Twins ones (i2v_twins.hip; without -DI2V_HAVE_TWINS the scalar
// restatement i2v_twins_host.h):
//   GSA forward   t1 = LN1 x | q = q(t1) | rows = gather_s(t1), r = sr(rows), u = LN(r) (sr > 1; else u = t1) | kv = kv(u) |
//                 t1 = attention(q, kv) | y = x + proj(t1)
//   LSA forward   t1 = LN1 x | qkv = qkv(t1) | t1 = window attention(qkv) | y = x + proj(t1)
//   both          t1 = LN2 y | h = fc1(t1), t2 = gelu(h) | x' = y + fc2(t2)
//   backward      the same in reverse; the gradient of t1 is the q path's plus the kv path's: the scatter adds the sr path into it
//                 (sr > 1), or the kv product takes it as its residual (sr = 1)
//   PEG           behind block 0 of a stage: x' = x + dw3(x) + b; backward g' = g + dw3^T(g) with the filter's taps reversed
// saved per block: x, y, h, four LayerNorm statistics per token, and qkv (LSA) or q, kv, the sub-sampled plane before its LayerNorm
// and its two statistics per key (GSA).  Per stage: the embedding before its LayerNorm with two statistics per token, and the stage's
// output stream.
// I2V_TWINS_ATTN=0, read when a net is planned, runs the core of every GSA block as the shared launches instead of twins_attention:
//   forward   P = softmax(scale q k^T) (batched vit_gemm over frames x heads, the row softmax) kept per block | t1 = P v (vit_gemm)
//   backward  dS = softmax'(dout v^T; P) | dq = dS k | dk = dS^T q | dv = P^T dout   (four vit_gemm launches and the softmax backward)
// at the cost of Tq x ld floats per head, frame and block for P (ld = Tk rounded up to 4) and one such array of scratch.  A developer
// switch: the attention launch loses to this route backward on two of the PCPVT shapes, and both stay comparable.
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>

#include "../../include/i2v_twins.h"
#include "i2v_swin_kernels.h"
#include "i2v_xf.h"
#ifdef I2V_HAVE_TWINS
#include "i2v_twins_kernels.h"
#else
#include "i2v_twins_host.h"     // (the host simulation's one-file build: the launches as scalar code)
#endif
#ifdef I2V_HAVE_XCIT
#include "i2v_xcit_kernels.h"   // xcit_dw3: the token-major depthwise 3 x 3 of the position encoding
#else
#include "i2v_xcit_host.h"
#endif

namespace {

struct TwBlock : Block {
    bool lsa = false;
    const float *qw = nullptr, *qb = nullptr, *kvw = nullptr, *kvb = nullptr, *srw = nullptr, *srb = nullptr, *snw = nullptr, *snb = nullptr;
    float *q = nullptr, *kv = nullptr, *srp = nullptr, *sstats = nullptr;      // (Block::qkv is the LSA block's)
};

struct TwStage {
    int grid = 0, width = 0, heads = 0, mlp = 0, sr = 1;
    std::vector<TwBlock> blocks;
    const float *pew = nullptr, *peb = nullptr, *penw = nullptr, *penb = nullptr, *pegw = nullptr, *pegb = nullptr, *pegm = nullptr;
    float *emb = nullptr, *estats = nullptr, *out = nullptr;      // the embedding before its LayerNorm, its statistics; the hooked stream
    int64_t T() const { return (int64_t)grid * grid; }
    int64_t Tk() const { return (int64_t)(grid / sr) * (grid / sr); }
    float* stream_after(size_t b) { return b + 1 < blocks.size() ? blocks[b + 1].x : out; }
};

}  // namespace

struct i2v_twins : XfNet {
    i2v_twins_config cfg{};
    int ns = 0;
    std::vector<TwStage> stages;
    const float* ztab = nullptr;      // the zeros the Swin window launch takes for its bias table
    float *patches = nullptr, *rows = nullptr, *peg = nullptr, *skv = nullptr, *st = nullptr, *st2 = nullptr;
    bool composed = false;            // I2V_TWINS_ATTN=0 at plan time: the GSA core on the shared launches, P saved per block
    float* dS = nullptr;              // ... and its score-gradient scratch

    TwinsAttn attn(const TwStage& S, const TwBlock& B, int frames) const {
        TwinsAttn a{};
        a.q = B.q; a.kv = B.kv; a.F = frames; a.Tq = (int)S.T(); a.Tk = (int)S.Tk(); a.H = S.heads; a.dh = S.width / S.heads;
        a.scale = 1.f / sqrtf((float)a.dh);
        return a;
    }
    float* hook_stream(int k) { return stages[k].out; }
    int64_t hook_floats(int k) const { return stages[k].T() * stages[k].width; }
    // the GSA core's operands for the shared launches: q (F, T, D), k and v the two halves of kv (F, Tk, 2 D)
    XfAttn shared(const TwStage& S, const TwBlock& B, int frames) const {
        const int64_t D = S.width;
        return {B.q, B.kv, B.kv + D, S.T() * D, D, S.Tk() * 2 * D, 2 * D, frames, (int)S.T(), (int)S.Tk(), S.heads, S.width / S.heads,
                1.f / sqrtf((float)(S.width / S.heads))};
    }
    XcitDw3 dw(const TwStage& S, const float* x, const float* w, const float* b, float* y, int frames) const {
        XcitDw3 d{};
        d.x = x; d.w = w; d.b = b; d.add = x; d.y = y; d.N = frames; d.H = S.grid; d.W = S.grid; d.C = S.width;
        return d;
    }
};

namespace {

int twins_plan(i2v_twins* n, const float* const* w, int nw, const int32_t* hooks, int n_hooks) {
    const i2v_twins_config& c = n->cfg;
    Arena& A = n->arena;
    if (c.img <= 0 || c.in_chans <= 0 || c.patch <= 0 || c.patch % 4 != 0 || c.img % c.patch != 0 || c.stages <= 0 ||
        c.stages > I2V_TWINS_MAX_STAGES || !(c.window == 0 || c.window == 7 || c.window == 4))
        return fail("i2v_twins_create: unsupported configuration (img %d patch %d window %d stages %d)", c.img, c.patch, c.window, c.stages);
    const int g0 = c.img / c.patch;
    for (int k = 0; k < c.stages; ++k) {
        const int g = g0 >> k, D = c.dims[k], H = c.heads[k], sr = c.sr[k];
        if (g <= 0 || (g << k) != g0)
            return fail("i2v_twins_create: the %d x %d grid of stage 0 does not halve %d times", g0, g0, k);
        if (D <= 0 || H <= 0 || D % H != 0 || (D / H) % 4 != 0 || c.mlp[k] <= 0 || c.mlp[k] % 4 != 0 || c.depths[k] <= 0)
            return fail("i2v_twins_create: stage %d has width %d, %d heads, MLP width %d and %d blocks", k, D, H, c.mlp[k], c.depths[k]);
        if (D / H > TWINS_MAX_DH) return fail("i2v_twins_create: heads of width %d in stage %d: up to %d", D / H, k, (int)TWINS_MAX_DH);
        if (!(sr == 1 || sr == 2 || sr == 4 || sr == 8) || g % sr != 0)
            return fail("i2v_twins_create: stage %d sub-samples its %d x %d grid by %d: 1, 2, 4 or 8, in whole blocks", k, g, g, sr);
        if ((g / sr) * (g / sr) > TWINS_MAX_TK)
            return fail("i2v_twins_create: stage %d attends to %d keys: one head's K and V are staged whole, up to %d keys", k,
                        (g / sr) * (g / sr), (int)TWINS_MAX_TK);
        if (c.window && (g % c.window != 0 || D / H != (c.window == 7 ? 32 : 16)))
            return fail("i2v_twins_create: stage %d (grid %d, head width %d) under window %d: whole windows, head width %d", k, g, D / H,
                        c.window, c.window == 7 ? 32 : 16);
    }
    const int deepest = Hooks::deepest(hooks, n_hooks, c.stages, A);
    if (deepest < 0) return 1;
    n->ns = A.depth = deepest + 1;
    const int64_t F = n->max_frames, KP = (int64_t)c.in_chans * c.patch * c.patch;
    // every size of the plan in floats, in 64 bits, before the first allocation
    std::vector<int64_t> sizes;
    int64_t acts = 0, mFTD = 0, mFTM = 0, mKV = 0, maxH = 0, mP = 0;
    const char* sw = getenv("I2V_TWINS_ATTN");
    n->composed = sw && !strcmp(sw, "0");
    for (int k = 0; k < n->ns; ++k) {
        const int64_t g = g0 >> k, D = c.dims[k], M = c.mlp[k], sr = c.sr[k], T = g * g, Tk = (g / sr) * (g / sr), FT = F * T;
        const int64_t FP = n->composed ? FT * c.heads[k] * xf_probs_ld((int)Tk) : 0;      // one block's saved probabilities
        for (int64_t v : {D * (k ? 4 * c.dims[k - 1] : KP), D, D, D}) sizes.push_back(v);
        acts += FT * D + 2 * FT;                                            // the embedding before its LayerNorm, its statistics
        for (int b = 0; b < c.depths[k]; ++b) {
            const bool lsa = c.window && b % 2 == 0;
            sizes.push_back(D); sizes.push_back(D);
            if (lsa) {
                for (int64_t v : {3 * D * D, 3 * D}) sizes.push_back(v);
                acts += 3 * FT * D;
            } else {
                for (int64_t v : {D * D, D, 2 * D * D, 2 * D}) sizes.push_back(v);
                if (sr > 1) {
                    for (int64_t v : {D * sr * sr * D, D, D, D}) sizes.push_back(v);
                    acts += F * Tk * (D + 2);                                // the sub-sampled plane before its LayerNorm, its statistics
                }
                acts += FT * D + 2 * F * Tk * D + FP;                       // q, kv (, P)
                mP = std::max(mP, FP);
            }
            for (int64_t v : {D * D, D, D, D, M * D, M, D * M, D}) sizes.push_back(v);
            if (b == 0) { sizes.push_back(9 * D); sizes.push_back(D); acts += 9 * D; }      // (the filter with its taps reversed)
            acts += 2 * FT * D + FT * M + 4 * FT;                           // x, y, h, statistics
        }
        acts += FT * D;                                                     // the stage's output stream
        mFTD = std::max(mFTD, FT * D); mFTM = std::max(mFTM, FT * M); mKV = std::max(mKV, 2 * F * Tk * D); maxH = std::max<int64_t>(maxH, c.heads[k]);
    }
    const int64_t NI = c.window ? (int64_t)(2 * c.window - 1) * (2 * c.window - 1) * maxH : 0;
    // shared scratch: patches, t1, G, the gathered rows, the stream in front of a position encoding; t2; dqkv (dq alone without
    // windows); dkv and two sub-sampled planes; the zero table
    acts += F * g0 * g0 * KP + 4 * mFTD + mFTM + (c.window ? 3 : 1) * mFTD + 2 * mKV + NI + mP;
    for (int i = 0; i < n_hooks; ++i) acts += F * (int64_t)(g0 >> hooks[i]) * (g0 >> hooks[i]) * c.dims[hooks[i]];
    if ((int)sizes.size() != nw) return fail("i2v_twins_create: %d weight arrays given, %zu expected for %d stages", nw, sizes.size(), n->ns);
    int64_t total = acts;
    for (int64_t v : sizes) total += v;
    VCHK(A.plan(total, F * g0 * g0));
    if (3 * mFTD >= (1ll << 31) || mFTM >= (1ll << 31) || mP >= (1ll << 31) || F > 65535 || (n->composed && F * maxH > 65535))
        return fail("i2v_twins_create: %lld bytes needed: too many frames for one net", (long long)A.planned);
    std::vector<const float*> dev;
    VCHK(A.upload(sizes, w, dev));
    size_t wi = 0;
    n->stages.resize(n->ns);
    for (int k = 0; k < n->ns; ++k) {
        TwStage& S = n->stages[k];
        S.grid = g0 >> k; S.width = c.dims[k]; S.heads = c.heads[k]; S.mlp = c.mlp[k]; S.sr = c.sr[k];
        const int64_t D = S.width, FT = F * S.T(), FK = F * S.Tk();
        S.pew = dev[wi]; S.peb = dev[wi + 1]; S.penw = dev[wi + 2]; S.penb = dev[wi + 3];
        wi += 4;
        if (!(S.emb = A.alloc(FT * D)) || !(S.estats = A.alloc(2 * FT))) return A.oom("a patch embedding");
        S.blocks.resize(c.depths[k]);
        for (int b = 0; b < c.depths[k]; ++b) {
            TwBlock& B = S.blocks[b];
            B.lsa = c.window && b % 2 == 0;
            const size_t w0 = wi;
            if (B.lsa) {
                wi += 4;
                if (!(B.qkv = A.alloc(3 * FT * D))) return A.oom("saved activations of a block");
            } else {
                B.qw = dev[wi + 2]; B.qb = dev[wi + 3]; B.kvw = dev[wi + 4]; B.kvb = dev[wi + 5];
                wi += 6;
                if (S.sr > 1) {
                    B.srw = dev[wi]; B.srb = dev[wi + 1]; B.snw = dev[wi + 2]; B.snb = dev[wi + 3];
                    wi += 4;
                    if (!(B.srp = A.alloc(FK * D)) || !(B.sstats = A.alloc(2 * FK))) return A.oom("saved activations of a block");
                }
                if (!(B.q = A.alloc(FT * D)) || !(B.kv = A.alloc(2 * FK * D))) return A.oom("saved activations of a block");
                if (n->composed && !(B.P = A.alloc(FT * S.heads * xf_probs_ld((int)S.Tk())))) return A.oom("saved probabilities of a block");
            }
            B.weights(&dev[w0], &dev[wi]);                                  // (an LSA block's qkv at [2..3]; a GSA block's are its own)
            wi += 8;
            if (b == 0) {
                S.pegw = dev[wi]; S.pegb = dev[wi + 1];
                std::vector<float> mir((size_t)9 * D);
                const float* host = w[wi];
                for (int t = 0; t < 9; ++t)
                    for (int64_t ch = 0; ch < D; ++ch) mir[(size_t)t * D + ch] = host[(size_t)(8 - t) * D + ch];
                float* dm = A.alloc(9 * D);
                if (!dm) return A.oom("a mirrored filter");
                HCHK(hipMemcpy(dm, mir.data(), mir.size() * 4, hipMemcpyHostToDevice));
                S.pegm = dm;
                wi += 2;
            }
            if (!(B.x = A.alloc(FT * D)) || !(B.y = A.alloc(FT * D)) || !(B.h = A.alloc(FT * S.mlp)) || !(B.stats = A.alloc(4 * FT)))
                return A.oom("saved activations of a block");
        }
        if (!(S.out = A.alloc(FT * D))) return A.oom("a stage's output");
    }
    if (!(n->patches = A.alloc(F * g0 * g0 * KP)) || !(n->t1 = A.alloc(mFTD)) || !(n->G = A.alloc(mFTD)) || !(n->rows = A.alloc(mFTD)) ||
        !(n->peg = A.alloc(mFTD)) || !(n->t2 = A.alloc(mFTM)) || !(n->dqkv = A.alloc((c.window ? 3 : 1) * mFTD)) || !(n->skv = A.alloc(mKV)) ||
        !(n->st = A.alloc(mKV / 2)) || !(n->st2 = A.alloc(mKV / 2)))
        return A.oom("scratch");
    if (mP && !(n->dS = A.alloc(mP))) return A.oom("scratch");
    if (NI) {
        float* z = A.alloc(NI);
        if (!z) return A.oom("scratch");
        HCHK(hipMemset(z, 0, (size_t)NI * 4));
        n->ztab = z;
    }
    for (int i = 0; i < n_hooks; ++i) {
        const TwStage& S = n->stages[hooks[i]];
        VCHK(n->hooks.add(A, hooks[i], F * S.T() * S.width));
    }
    return 0;
}

int tw_block_forward(i2v_twins* n, const TwStage& S, const TwBlock& B, int frames, float* out, hipStream_t s) {
    const i2v_twins_config& c = n->cfg;
    const int D = S.width, g = S.grid, M = frames * (int)S.T(), Mk = frames * (int)S.Tk(), dh = D / S.heads;
    const int64_t FT = M, sp = (int64_t)n->max_frames * S.T(), spk = (int64_t)n->max_frames * S.Tk();
    float* st = B.stats;                                                    // [mean1 | rstd1 | mean2 | rstd2] at max_frames spacing
    VCHK(vit_layernorm(B.x, FT, D, B.n1w, B.n1b, c.ln_eps, n->t1, st, st + sp, s));
    if (B.lsa) {
        VCHK(linear(n->t1, M, D, B.qkvw, B.qkvb, 3 * D, nullptr, B.qkv, nullptr, s));
        VCHK(twins_window_attention(B.qkv, frames, g, g, c.window, S.heads, dh, n->ztab, n->t1, s));
    } else {
        VCHK(linear(n->t1, M, D, B.qw, B.qb, D, nullptr, B.q, nullptr, s));
        const float* u = n->t1;
        if (S.sr > 1) {                                                     // the sr convolution: gather, Linear; then its LayerNorm
            VCHK(twins_block_gather(n->t1, n->rows, frames, g, g, D, S.sr, s));
            VCHK(linear(n->rows, Mk, S.sr * S.sr * D, B.srw, B.srb, D, nullptr, B.srp, nullptr, s));
            VCHK(vit_layernorm(B.srp, Mk, D, B.snw, B.snb, c.pe_eps, n->st, B.sstats, B.sstats + spk, s));
            u = n->st;
        }
        VCHK(linear(u, Mk, D, B.kvw, B.kvb, 2 * D, nullptr, B.kv, nullptr, s));
        if (n->composed) {
            VCHK(xf_attention(n->shared(S, B, frames), B.P, n->t1, s));             // P kept in B.P
        } else {
            TwinsAttn a = n->attn(S, B, frames);
            a.out = n->t1;
            VCHK(twins_attention(a, s));
        }
    }
    VCHK(linear(n->t1, M, D, B.projw, B.projb, D, B.x, B.y, nullptr, s));                     // y = x + proj(attn)
    VCHK(vit_layernorm(B.y, FT, D, B.n2w, B.n2b, c.ln_eps, n->t1, st + 2 * sp, st + 3 * sp, s));
    VCHK(linear(n->t1, M, D, B.fc1w, B.fc1b, S.mlp, nullptr, B.h, n->t2, s));                  // h = fc1(LN2 y), t2 = gelu(h)
    return linear(n->t2, M, S.mlp, B.fc2w, B.fc2b, D, B.y, out, nullptr, s);                  // x' = y + fc2(gelu(h))
}

// `gin`: gradient of the stream after the block; leaves the gradient of its input in G
int tw_block_backward(i2v_twins* n, const TwStage& S, const TwBlock& B, int frames, const float* gin, hipStream_t s) {
    const i2v_twins_config& c = n->cfg;
    const int D = S.width, g = S.grid, M = frames * (int)S.T(), Mk = frames * (int)S.Tk(), dh = D / S.heads;
    const int64_t FT = M, sp = (int64_t)n->max_frames * S.T(), spk = (int64_t)n->max_frames * S.Tk();
    const float* st = B.stats;
    VCHK(linear_bwd(gin, M, D, B.fc2w, S.mlp, B.h, n->t2, s));                                 // dh = (g fc2) * gelu'(h)
    VCHK(linear_bwd(n->t2, M, S.mlp, B.fc1w, D, nullptr, n->t1, s));                           // d LN2 out
    VCHK(vit_layernorm_bwd(n->t1, B.y, st + 2 * sp, st + 3 * sp, B.n2w, FT, D, gin, nullptr, n->G, s));      // G = dy
    VCHK(linear_bwd(n->G, M, D, B.projw, D, nullptr, n->t1, s));                               // d attention out
    if (B.lsa) {
        VCHK(twins_window_attention_bwd(B.qkv, n->t1, frames, g, g, c.window, S.heads, dh, n->ztab, n->dqkv, s));
        VCHK(linear_bwd(n->dqkv, M, 3 * D, B.qkvw, D, nullptr, n->t1, s));                     // d LN1 out
    } else {
        if (n->composed) {
            VCHK(xf_attention_bwd(n->shared(S, B, frames), B.P, n->t1, n->dS, n->dqkv, n->skv, n->skv + D, s));      // dq; (dk, dv) in skv
        } else {
            TwinsAttn a = n->attn(S, B, frames);
            a.dout = n->t1; a.dq = n->dqkv; a.dkv = n->skv;
            VCHK(twins_attention_bwd(a, s));
        }
        VCHK(linear_bwd(n->dqkv, M, D, B.qw, D, nullptr, n->t1, s));                           // d LN1 out: the q path
        if (S.sr > 1) {
            VCHK(linear_bwd(n->skv, Mk, 2 * D, B.kvw, D, nullptr, n->st, s));
            VCHK(vit_layernorm_bwd(n->st, B.srp, B.sstats, B.sstats + spk, B.snw, Mk, D, nullptr, nullptr, n->st2, s));
            VCHK(linear_bwd(n->st2, Mk, D, B.srw, S.sr * S.sr * D, nullptr, n->rows, s));
            VCHK(twins_block_scatter(n->rows, n->t1, frames, g, g, D, S.sr, 1, s));            // ... plus the kv path
        } else {                                                                               // (R is C: i2v_vit_kernels.h allows it)
            VCHK(linear_bwd_add(n->skv, M, 2 * D, B.kvw, D, n->t1, n->t1, s));
        }
    }
    return vit_layernorm_bwd(n->t1, B.x, st, st + sp, B.n1w, FT, D, n->G, nullptr, n->G, s);   // G = dx
}

int twins_forward(i2v_twins* n, const float* x, int frames, hipStream_t s) {
    const i2v_twins_config& c = n->cfg;
    for (int k = 0; k < n->ns; ++k) {
        TwStage& S = n->stages[k];
        const int D = S.width, g = S.grid, M = frames * (int)S.T();
        const int64_t sp = (int64_t)n->max_frames * S.T();
        if (k == 0) {                                                       // the patch embedding: rows, Linear, LayerNorm
            VCHK(patch_rows(x, frames, c.in_chans, g, c.patch, S.pew, S.peb, D, n->patches, S.emb, s));
        } else {
            const TwStage& Pv = n->stages[k - 1];
            VCHK(swin_merge_gather(Pv.out, frames, Pv.grid, Pv.grid, Pv.width, n->rows, s));
            VCHK(linear(n->rows, M, 4 * Pv.width, S.pew, S.peb, D, nullptr, S.emb, nullptr, s));
        }
        VCHK(vit_layernorm(S.emb, M, D, S.penw, S.penb, c.pe_eps, S.blocks[0].x, S.estats, S.estats + sp, s));
        for (size_t b = 0; b < S.blocks.size(); ++b) {
            VCHK(tw_block_forward(n, S, S.blocks[b], frames, b == 0 ? n->peg : S.stream_after(b), s));
            if (b == 0) VCHK(xcit_dw3(n->dw(S, n->peg, S.pegw, S.pegb, S.stream_after(0), frames), s));      // x + dw3(x) + b
        }
    }
    return 0;
}

int twins_backward(i2v_twins* n, float* gx, int accumulate, hipStream_t s) {
    const i2v_twins_config& c = n->cfg;
    const int frames = n->frames;
    for (int k = n->ns - 1; k >= 0; --k) {
        TwStage& S = n->stages[k];
        const int D = S.width, g = S.grid, M = frames * (int)S.T();
        const int64_t sp = (int64_t)n->max_frames * S.T();
        for (int b = (int)S.blocks.size() - 1; b >= 0; --b) {
            // gradient of the stream after block b: the deepest stage's hook view for the very last block, the running gradient G
            // otherwise (where the next stage's embedding backward has already added this stage's hook)
            const float* gin = (k == n->ns - 1 && b == (int)S.blocks.size() - 1) ? n->hooks.grad_at(k) : n->G;
            if (b == 0) {                                                   // back through the position encoding: g + dw3^T(g)
                VCHK(xcit_dw3(n->dw(S, gin, S.pegm, nullptr, n->peg, frames), s));
                gin = n->peg;
            }
            VCHK(tw_block_backward(n, S, S.blocks[b], frames, gin, s));
        }
        VCHK(vit_layernorm_bwd(n->G, S.emb, S.estats, S.estats + sp, S.penw, M, D, nullptr, nullptr, n->t1, s));
        if (k > 0) {
            const TwStage& Pv = n->stages[k - 1];
            VCHK(linear_bwd(n->t1, M, D, S.pew, 4 * Pv.width, nullptr, n->rows, s));
            VCHK(swin_merge_scatter(n->rows, frames, Pv.grid, Pv.grid, Pv.width, n->hooks.grad_at(k - 1), n->G, s));
        } else {
            VCHK(patch_rows_bwd(n->t1, frames, c.in_chans, g, c.patch, S.pew, D, n->patches, gx, accumulate, s));
        }
    }
    return 0;
}

}  // namespace

extern "C" int i2v_twins_create(int device, const i2v_twins_config* cfg, const float* const* weights, int n_weights, const int32_t* hook_stages,
                                int n_hooks, int max_frames, i2v_twins_handle* out) {
    return xf_create("i2v_twins_create", "stage", device, cfg, weights, hook_stages, max_frames, out, [&](i2v_twins* n) {
        n->cfg = *cfg;
        return twins_plan(n, weights, n_weights, hook_stages, n_hooks);
    });
}

extern "C" int i2v_twins_destroy(i2v_twins_handle net) { return xf_destroy(net); }

extern "C" int64_t i2v_twins_workspace_bytes(i2v_twins_handle net) { return xf_workspace_bytes(net); }

extern "C" int i2v_twins_forward(i2v_twins_handle n, const float* x, int frames, void* stream) {
    return xf_forward("i2v_twins_forward", n, x, frames, stream, twins_forward);
}

extern "C" int i2v_twins_backward(i2v_twins_handle n, float* gx, int accumulate, void* stream) {
    return xf_backward("i2v_twins_backward", n, gx, accumulate, stream, twins_backward);
}

extern "C" int i2v_twins_hook_info(i2v_twins_handle n, int hook, float** act, int64_t* act_stride, float** grad, int64_t* grad_stride, int64_t* D) {
    return xf_hook_info("i2v_twins_hook_info", n, hook, act, act_stride, grad, grad_stride, D);
}

extern "C" int i2v_twins_read_hook(i2v_twins_handle n, int hook, int which, float* out, int frames, void* stream) {
    return xf_read_hook("i2v_twins_read_hook", n, hook, which, out, frames, stream);
}

// ---- the kernels on their own ----
extern "C" int i2v_twins_attention_f32(const float* q, const float* kv, int frames, int Tq, int Tk, int heads, int dh, float scale, float* out,
                                       void* stream) {
    TwinsAttn a{};
    a.q = q; a.kv = kv; a.F = frames; a.Tq = Tq; a.Tk = Tk; a.H = heads; a.dh = dh; a.scale = scale; a.out = out;
    return twins_attention(a, (hipStream_t)stream);
}

extern "C" int i2v_twins_attention_bwd_f32(const float* q, const float* kv, const float* dout, int frames, int Tq, int Tk, int heads, int dh,
                                           float scale, float* dq, float* dkv, void* stream) {
    TwinsAttn a{};
    a.q = q; a.kv = kv; a.F = frames; a.Tq = Tq; a.Tk = Tk; a.H = heads; a.dh = dh; a.scale = scale; a.dout = dout; a.dq = dq; a.dkv = dkv;
    return twins_attention_bwd(a, (hipStream_t)stream);
}

extern "C" int i2v_twins_block_gather_f32(const float* x, float* rows, int frames, int H, int W, int C, int sr, void* stream) {
    return twins_block_gather(x, rows, frames, H, W, C, sr, (hipStream_t)stream);
}

extern "C" int i2v_twins_block_scatter_f32(const float* drows, float* dx, int frames, int H, int W, int C, int sr, int accumulate, void* stream) {
    return twins_block_scatter(drows, dx, frames, H, W, C, sr, accumulate, (hipStream_t)stream);
}

extern "C" int i2v_twins_window_attention_f32(const float* qkv, int frames, int H, int W, int window, int heads, int dh, const float* zero_table,
                                              float* out, void* stream) {
    return twins_window_attention(qkv, frames, H, W, window, heads, dh, zero_table, out, (hipStream_t)stream);
}

extern "C" int i2v_twins_window_attention_bwd_f32(const float* qkv, const float* dout, int frames, int H, int W, int window, int heads, int dh,
                                                  const float* zero_table, float* dqkv, void* stream) {
    return twins_window_attention_bwd(qkv, dout, frames, H, W, window, heads, dh, zero_table, dqkv, (hipStream_t)stream);
}
