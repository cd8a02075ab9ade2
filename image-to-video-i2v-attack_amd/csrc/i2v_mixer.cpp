// Planner and executor of the all-MLP surrogates (include/i2v_mixer.h: MLP-Mixer and ResMLP) on the transformer stack: one arena per
// (net, max frames), the forward as a fixed launch sequence up to the deepest hooked block, and the input-gradient pass -- no weight
// gradients.  The channel half of a block is the LayerNorm + MLP half of a transformer block, so the arena, the hook list, the two
// linear launches and the LayerNorm pair are the shared ones of i2v_xf.h and the stem is ViT's patchify plus a Linear; this file brings
// the launch order and the sizes.  The token half is the kernel of i2v_mixer.hip.
//
// MLP-Mixer block, streams (F, S, D):
//   forward   t1 = LN1(x) | y = x + tokmix(t1) | t1 = LN2(y) | h = fc1(t1), t2 = gelu(h) | x' = y + fc2(t2)                 (6 launches)
//   backward  t2 = (g fc2) * gelu'(h) | t1 = t2 fc1 | G = LN2'(t1; y) + g | t1 = LN1(x) again | dqkv = tokmix'(t1, G) |
//             G = LN1'(dqkv; x) + G (+ the hook gradient of the stream x)                                                   (6 launches)
//   saved per block: x, y, h and the four LayerNorm statistics per token; the token hidden activation is recomputed in LDS.
// ResMLP block, in place on one stream (a hooked block writes its output to that hook's own buffer instead):
//   forward   y = x + ls1 * tokmix(a1 x + b1) | h = fc1'(y), t2 = gelu(h) | x' = y + fc2'(t2)                                (3 launches)
//   backward  t2 = (g fc2') * gelu'(h) | G = g + t2 fc1' | G = G + a1 * tokmix'(ls1 * G) (+ the hook gradient)              (3 launches)
//   saved per block: h.  (The affine is linear: its backward needs no activation.)
#include "../../include/i2v_mixer.h"
#include "i2v_xf.h"
#ifndef I2V_HAVE_MIXER
#include "i2v_mixer_host.h"     // (the host simulation's one-file build: the token launch as scalar code)
#endif

namespace {

struct MxBlock {
    // kind 0: n1w n1b | w1 b1 w2 b2 | n2w n2b; kind 1: a1 be1 ls1 | w1 (= W) b1 (= b)
    const float *n1w, *n1b, *w1, *b1, *w2, *b2, *n2w, *n2b, *a1, *be1, *ls1, *fc1w, *fc1b, *fc2w, *fc2b;
    const float *w1t, *w2t;                      // transposed copies made at create time (kind 1: w1t = W^T)
    float *x, *y, *h, *stats, *out;              // kind 0: saved input, mid stream, fc1 pre-activation, LN stats; out: where x' goes
    I2VMixTokParams fwd, bwd;
};

}  // namespace

struct i2v_mixer : XfNet {
    i2v_mixer_config cfg{};
    int nb = 0, gsz = 0, S = 0;
    const float *pe_w = nullptr, *pe_b = nullptr;
    std::vector<MxBlock> blocks;
    float *patches = nullptr, *stream = nullptr;

    float* hook_stream(int b) { return blocks[b].out; }      // (a hooked ResMLP block writes a buffer of its own)
    int64_t hook_floats(int) const { return (int64_t)S * cfg.dim; }
};

namespace {

int tok_plan(I2VMixTokParams* p) {
#ifdef I2V_HAVE_MIXER
    const int bad = k_mixer_tokens_plan(p);
#else
    const int bad = eng::mixer_host::plan(p);
#endif
    if (bad) return fail("i2v_mixer_create: %d tokens and %d hidden rows of a 32-channel tile do not fit the token launch's LDS", p->S, p->Sh);
    return 0;
}

int tok_run(I2VMixTokParams p, int frames, hipStream_t s) {
    p.F = frames;
#ifdef I2V_HAVE_MIXER
    if (k_mixer_tokens(p, (i2v_stream_t)s) != 0) {
        const char* e = be_error();
        return fail("%s", e ? e : "k_mixer_tokens failed");
    }
#else
    (void)s;
    if (eng::mixer_host::tokens(p) != 0) return fail("mixer_host::tokens: launch not planned");
#endif
    return 0;
}

// the (rows, cols) host matrix transposed onto the device
int upload_transposed(Arena& A, const float* host, int64_t rows, int64_t cols, const float** out) {
    std::vector<float> t((size_t)(rows * cols));
    for (int64_t r = 0; r < rows; ++r)
        for (int64_t c = 0; c < cols; ++c) t[(size_t)(c * rows + r)] = host[r * cols + c];
    float* d = A.alloc(rows * cols);
    if (!d) return A.oom("a transposed token weight");
    HCHK(hipMemcpy(d, t.data(), t.size() * 4, hipMemcpyHostToDevice));
    *out = d;
    return 0;
}

int mixer_plan(i2v_mixer* n, const float* const* w, int nw, const int32_t* hooks, int n_hooks) {
    const i2v_mixer_config& c = n->cfg;
    Arena& A = n->arena;
    if (c.img <= 0 || c.patch <= 0 || c.patch % 4 != 0 || c.img % c.patch != 0 || c.in_chans <= 0 || c.dim <= 0 || c.dim % 4 != 0 ||
        c.blocks <= 0 || c.mlp <= 0 || c.mlp % 4 != 0 || (c.kind != 0 && c.kind != 1) || (c.kind == 0 ? c.tokens_hidden <= 0 : c.tokens_hidden != 0))
        return fail("i2v_mixer_create: unsupported configuration (img %d patch %d dim %d blocks %d tokens_hidden %d mlp %d kind %d)", c.img,
                    c.patch, c.dim, c.blocks, c.tokens_hidden, c.mlp, c.kind);
    n->gsz = c.img / c.patch;
    n->S = n->gsz * n->gsz;
    const int deepest = Hooks::deepest(hooks, n_hooks, c.blocks, A);
    if (deepest < 0) return 1;
    n->nb = A.depth = deepest + 1;
    const bool res = c.kind == 1;
    const int64_t F = n->max_frames, KP = (int64_t)c.in_chans * c.patch * c.patch, S = n->S, Sh = c.tokens_hidden, D = c.dim, Hm = c.mlp;
    const int64_t FT = F * S;
    // every size of the plan in floats, in 64 bits, before the first allocation
    std::vector<int64_t> sizes = {D * KP, D};
    int64_t acts = FT * KP;                                                     // patches
    for (int b = 0; b < n->nb; ++b) {
        if (!res) {
            for (int64_t v : {D, D, Sh * S, Sh, S * Sh, S, D, D, Hm * D, Hm, D * Hm, D}) sizes.push_back(v);
            acts += 2 * S * Sh + 2 * FT * D + FT * Hm + 4 * FT;                 // transposed token weights; x, y, h, stats
        } else {
            for (int64_t v : {D, D, D, S * S, S, Hm * D, Hm, D * Hm, D}) sizes.push_back(v);
            acts += S * S + FT * Hm;                                            // transposed token weight; h
        }
    }
    if (!res) acts += FT * D + (FT * D + FT * Hm + FT * D + FT * D);            // the last block's output; scratch t1, t2, dqkv, G
    else acts += FT * D + (FT * Hm + FT * D) + n_hooks * FT * D;                // the stream; scratch t2, G; one stream copy per hook
    acts += n_hooks * FT * D;                                                   // hook gradients
    if ((int)sizes.size() != nw) return fail("i2v_mixer_create: %d weight arrays given, %zu expected for %d blocks", nw, sizes.size(), n->nb);
    int64_t total = acts;
    for (int64_t v : sizes) total += v;
    VCHK(A.plan(total, FT));
    if (FT * Hm >= (1ll << 31) || FT * KP >= (1ll << 31))
        return fail("i2v_mixer_create: %lld bytes needed: too many frames for one net", (long long)A.planned);
    std::vector<const float*> dev;
    VCHK(A.upload(sizes, w, dev));
    n->pe_w = dev[0]; n->pe_b = dev[1];
    if (!(n->patches = A.alloc(FT * KP))) return A.oom("stem");
    if (!res && !(n->t1 = A.alloc(FT * D))) return A.oom("scratch");
    if (!(n->t2 = A.alloc(FT * Hm)) || !(n->G = A.alloc(FT * D))) return A.oom("scratch");
    if (!res && !(n->dqkv = A.alloc(FT * D))) return A.oom("scratch");
    if (res && !(n->stream = A.alloc(FT * D))) return A.oom("the stream");
    n->blocks.resize(n->nb);
    size_t wi = 2;
    for (int b = 0; b < n->nb; ++b) {
        MxBlock& B = n->blocks[b];
        B = MxBlock{};
        const float* const* q = &dev[wi];
        if (!res) {
            B.n1w = q[0]; B.n1b = q[1]; B.w1 = q[2]; B.b1 = q[3]; B.w2 = q[4]; B.b2 = q[5]; B.n2w = q[6]; B.n2b = q[7];
            B.fc1w = q[8]; B.fc1b = q[9]; B.fc2w = q[10]; B.fc2b = q[11];
            VCHK(upload_transposed(A, w[wi + 2], Sh, S, &B.w1t));               // (S, Sh)
            VCHK(upload_transposed(A, w[wi + 4], S, Sh, &B.w2t));               // (Sh, S)
            wi += 12;
            if (!(B.x = b ? n->blocks[b - 1].out : A.alloc(FT * D)) || !(B.y = A.alloc(FT * D)) || !(B.h = A.alloc(FT * Hm)) ||
                !(B.stats = A.alloc(4 * FT)) || !(B.out = A.alloc(FT * D)))
                return A.oom("saved activations of a block");
        } else {
            B.a1 = q[0]; B.be1 = q[1]; B.ls1 = q[2]; B.w1 = q[3]; B.b1 = q[4]; B.fc1w = q[5]; B.fc1b = q[6]; B.fc2w = q[7]; B.fc2b = q[8];
            VCHK(upload_transposed(A, w[wi + 3], S, S, &B.w1t));
            wi += 9;
            if (!(B.h = A.alloc(FT * Hm))) return A.oom("saved activations of a block");
            B.x = b ? n->blocks[b - 1].out : n->stream;
            B.y = n->stream;
            B.out = n->stream;                                                  // (a hooked block: its hook's buffer, below)
        }
    }
    for (int i = 0; i < n_hooks; ++i) {
        MxBlock& B = n->blocks[hooks[i]];
        if (res) {
            if (!(B.out = A.alloc(FT * D))) return A.oom("a hooked stream");
            if (hooks[i] + 1 < n->nb) n->blocks[hooks[i] + 1].x = B.out;
        }
        VCHK(n->hooks.add(A, hooks[i], FT * D));
    }
    // the token launches
    for (int b = 0; b < n->nb; ++b) {
        MxBlock& B = n->blocks[b];
        I2VMixTokParams& f = B.fwd;
        f = I2VMixTokParams{};
        f.S = (int)S; f.Sh = (int)Sh; f.C = (int)D;
        I2VMixTokParams& g = B.bwd;
        if (!res) {
            f.z = n->t1; f.r = B.x; f.out = B.y; f.wa = B.w1; f.ba = B.b1; f.wb = B.w2; f.bb = B.b2;
            g = f;
            g.bwd = 1; g.r = n->G; g.out = n->dqkv; g.wb = B.w2t; g.bb = nullptr; g.wc = B.w1t;
        } else {
            f.z = B.x; f.r = B.x; f.out = B.y; f.wa = B.w1; f.ba = B.b1; f.in_scale = B.a1; f.in_shift = B.be1; f.out_scale = B.ls1;
            g = f;
            g.bwd = 1; g.z = nullptr; g.wa = nullptr; g.ba = nullptr; g.wb = B.w1t; g.r = n->G; g.add0 = n->G; g.out = n->G;
            g.add1 = b ? n->hooks.grad_at(b - 1) : nullptr;
        }
        VCHK(tok_plan(&f));
        VCHK(tok_plan(&g));
    }
    return 0;
}

int mixer_forward(i2v_mixer* n, const float* x, int frames, hipStream_t s) {
    const i2v_mixer_config& c = n->cfg;
    const int D = c.dim, M = frames * n->S;
    const int64_t FT = (int64_t)frames * n->S, sp = (int64_t)n->max_frames * n->S;
    VCHK(patch_rows(x, frames, c.in_chans, n->gsz, c.patch, n->pe_w, n->pe_b, D, n->patches, n->blocks[0].x, s));
    for (MxBlock& B : n->blocks) {
        if (c.kind == 0) {
            float* st = B.stats;                                                  // [mean1 | rstd1 | mean2 | rstd2] at max_frames spacing
            VCHK(vit_layernorm(B.x, FT, D, B.n1w, B.n1b, c.ln_eps, n->t1, st, st + sp, s));
            VCHK(tok_run(B.fwd, frames, s));                                      // y = x + tokmix(t1)
            VCHK(vit_layernorm(B.y, FT, D, B.n2w, B.n2b, c.ln_eps, n->t1, st + 2 * sp, st + 3 * sp, s));
            VCHK(linear(n->t1, M, D, B.fc1w, B.fc1b, c.mlp, nullptr, B.h, n->t2, s));     // h = fc1(LN2 y), t2 = gelu(h)
            VCHK(linear(n->t2, M, c.mlp, B.fc2w, B.fc2b, D, B.y, B.out, nullptr, s));     // x' = y + fc2(t2)
        } else {
            VCHK(tok_run(B.fwd, frames, s));                                      // y = x + ls1 * (W (a1 x + b1) + b), into the stream
            VCHK(linear(B.y, M, D, B.fc1w, B.fc1b, c.mlp, nullptr, B.h, n->t2, s));
            VCHK(linear(n->t2, M, c.mlp, B.fc2w, B.fc2b, D, B.y, B.out, nullptr, s));     // x' = y + fc2'(t2): in place, or into a hook's buffer
        }
    }
    return 0;
}

int mixer_backward(i2v_mixer* n, float* gx, int accumulate, hipStream_t s) {
    const i2v_mixer_config& c = n->cfg;
    const int frames = n->frames, D = c.dim, M = frames * n->S;
    const int64_t FT = (int64_t)frames * n->S, sp = (int64_t)n->max_frames * n->S;
    for (int b = n->nb - 1; b >= 0; --b) {
        MxBlock& B = n->blocks[b];
        // gradient of the block's output: the deepest block's hook view, the running gradient G (which holds the later hooks' too) below it
        const float* gin = n->grad_in(b, n->nb);
        const float* below = n->grad_below(b);                                   // a hook at the stream this block reads
        VCHK(linear_bwd(gin, M, D, B.fc2w, c.mlp, B.h, n->t2, s));               // dh = (g fc2) * gelu'(h)
        if (c.kind == 0) {
            float* st = B.stats;
            VCHK(linear_bwd(n->t2, M, c.mlp, B.fc1w, D, nullptr, n->t1, s));     // d LN2 out
            VCHK(vit_layernorm_bwd(n->t1, B.y, st + 2 * sp, st + 3 * sp, B.n2w, FT, D, gin, nullptr, n->G, s));    // G = dy
            VCHK(vit_layernorm(B.x, FT, D, B.n1w, B.n1b, c.ln_eps, n->t1, st, st + sp, s));                       // t1 = LN1(x) again
            VCHK(tok_run(B.bwd, frames, s));                                     // dqkv = d t1
            VCHK(vit_layernorm_bwd(n->dqkv, B.x, st, st + sp, B.n1w, FT, D, n->G, below, n->G, s));                // G = dx (+ hook)
        } else {
            VCHK(linear_bwd_add(n->t2, M, c.mlp, B.fc1w, D, gin, n->G, s));      // G = dy = g + dh fc1'
            VCHK(tok_run(B.bwd, frames, s));                                     // G = dy + a1 * W^T (ls1 * dy) (+ hook)
        }
    }
    return patch_rows_bwd(n->G, frames, c.in_chans, n->gsz, c.patch, n->pe_w, D, n->patches, gx, accumulate, s);
}

}  // namespace

extern "C" int i2v_mixer_create(int device, const i2v_mixer_config* cfg, const float* const* weights, int n_weights, const int32_t* hook_blocks,
                                int n_hooks, int max_frames, i2v_mixer_handle* out) {
    return xf_create("i2v_mixer_create", "block", device, cfg, weights, hook_blocks, max_frames, out, [&](i2v_mixer* n) {
        n->cfg = *cfg;
        return mixer_plan(n, weights, n_weights, hook_blocks, n_hooks);
    });
}

extern "C" int i2v_mixer_destroy(i2v_mixer_handle net) { return xf_destroy(net); }

extern "C" int64_t i2v_mixer_workspace_bytes(i2v_mixer_handle net) { return xf_workspace_bytes(net); }

extern "C" int i2v_mixer_forward(i2v_mixer_handle n, const float* x, int frames, void* stream) {
    return xf_forward("i2v_mixer_forward", n, x, frames, stream, mixer_forward);
}

extern "C" int i2v_mixer_backward(i2v_mixer_handle n, float* gx, int accumulate, void* stream) {
    return xf_backward("i2v_mixer_backward", n, gx, accumulate, stream, mixer_backward);
}

extern "C" int i2v_mixer_hook_info(i2v_mixer_handle n, int hook, float** act, int64_t* act_stride, float** grad, int64_t* grad_stride,
                                   int64_t* D) {
    return xf_hook_info("i2v_mixer_hook_info", n, hook, act, act_stride, grad, grad_stride, D);
}

extern "C" int i2v_mixer_read_hook(i2v_mixer_handle n, int hook, int which, float* out, int frames, void* stream) {
    return xf_read_hook("i2v_mixer_read_hook", n, hook, which, out, frames, stream);
}
