// Planner and executor of the Swin surrogates (include/i2v_swin.h): one arena per (net, max frames), the forward as a fixed launch
// sequence up to the deepest hooked stage, and the input-gradient pass -- no weight gradients, as the CNN and ViT paths.  The window
// attention and patch-merging kernels are in i2v_swin.hip; the linear layers, LayerNorms and patch rows are the ViT kernels.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../include/i2v_swin.h"
#include "i2v_kernels.h"
#include "i2v_swin_kernels.h"
#include "i2v_vit_kernels.h"

namespace {

int fail(const char* fmt, ...) __attribute__((format(printf, 1, 2)));
int fail(const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    return i2v_api_fail(buf);
}
#define VCHK(expr) do { if ((expr) != 0) return 1; } while (0)
#define HCHK(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) return fail("%s: %s", #expr, hipGetErrorString(e_)); } while (0)

// y (M, N) = x (M, K) W^T (+ bias) (+ residual), W (N, K)
int linear(const float* x, int M, int K, const float* W, const float* bias, int N, const float* residual, float* y, float* gelu_out,
           hipStream_t s) {
    VitGemm g{};
    g.A = x; g.a_sm = K; g.a_sk = 1;
    g.B = W; g.b_sk = 1; g.b_sn = K;
    g.C = y; g.c_sm = N;
    g.bias = bias; g.R = residual; g.C2 = gelu_out;
    g.M = M; g.N = N; g.K = K; g.batch = 1; g.nb_in = 1; g.alpha = 1.f;
    g.mode = gelu_out ? VIT_EPI_GELU : VIT_EPI_PLAIN;
    return vit_gemm(g, s);
}

// dx (M, K) = dy (M, N) W (* gelu'(pre))
int linear_bwd(const float* dy, int M, int N, const float* W, int K, const float* pre, float* dx, hipStream_t s) {
    VitGemm g{};
    g.A = dy; g.a_sm = N; g.a_sk = 1;
    g.B = W; g.b_sk = K; g.b_sn = 1;
    g.C = dx; g.c_sm = K;
    g.H = pre;
    g.M = M; g.N = K; g.K = N; g.batch = 1; g.nb_in = 1; g.alpha = 1.f;
    g.mode = pre ? VIT_EPI_GELU_BWD : VIT_EPI_PLAIN;
    return vit_gemm(g, s);
}

int embed(const float* img, int F, int Cin, int gsz, int P, const float* W, const float* b, const float* nw, const float* nb, float eps,
          int dim, float* patches, float* emb, float* mean, float* rstd, float* tokens, hipStream_t s) {
    const int np = gsz * gsz, KP = Cin * P * P;
    VCHK(vit_patchify(img, patches, F, Cin, gsz, gsz, P, nullptr, 0, s));
    VCHK(linear(patches, F * np, KP, W, b, dim, nullptr, emb, nullptr, s));
    return vit_layernorm(emb, (int64_t)F * np, dim, nw, nb, eps, tokens, mean, rstd, s);
}

int embed_bwd(const float* dtok, int F, int Cin, int gsz, int P, const float* W, const float* nw, int dim, const float* emb,
              const float* mean, const float* rstd, float* demb, float* patches, float* gimg, int accumulate, hipStream_t s) {
    const int np = gsz * gsz, KP = Cin * P * P;
    VCHK(vit_layernorm_bwd(dtok, emb, mean, rstd, nw, (int64_t)F * np, dim, nullptr, nullptr, demb, s));
    VCHK(linear_bwd(demb, F * np, dim, W, KP, nullptr, patches, s));
    return vit_patchify(nullptr, patches, F, Cin, gsz, gsz, P, gimg, accumulate, s);
}

struct Block {
    const float *n1w, *n1b, *qkvw, *qkvb, *table, *projw, *projb, *n2w, *n2b, *fc1w, *fc1b, *fc2w, *fc2b;
    float *x, *qkv, *y, *h, *stats;         // saved per block: input stream, qkv, mid stream, fc1 pre-activation, LN stats
    int shift;
};

struct Stage {
    int grid = 0, width = 0, heads = 0, ws = 0;
    std::vector<Block> blocks;
    float* out = nullptr;                    // stream after the last block: the hooked feature
    // the patch merging behind the stage (when a deeper stage runs)
    const float *mnw = nullptr, *mnb = nullptr, *mred = nullptr;
    float *mg = nullptr, *mstats = nullptr;  // saved: the gathered rows (F, grid^2 / 4, 4 width), their LN stats
    int64_t T() const { return (int64_t)grid * grid; }
};

}  // namespace

struct i2v_swin {
    i2v_swin_config cfg{};
    int device = 0, ns = 0, max_frames = 0, frames = 0, gsz = 0;
    std::vector<void*> allocs;
    const float *pe_w = nullptr, *pe_b = nullptr, *pe_nw = nullptr, *pe_nb = nullptr;
    std::vector<Stage> stages;
    float *patches = nullptr, *emb = nullptr, *estats = nullptr;
    float *t1 = nullptr, *t2 = nullptr, *dqkv = nullptr, *G = nullptr;
    std::vector<int> hook_stage;
    std::vector<float*> hook_grad;
    int64_t bytes = 0, planned = 0;

    float* alloc(int64_t n) {
        void* p = nullptr;
        if (hipMalloc(&p, (size_t)n * 4) != hipSuccess) return nullptr;
        allocs.push_back(p);
        bytes += n * 4;
        return (float*)p;
    }
    int oom(const char* what) {
        (void)hipGetLastError();
        return fail("i2v_swin_create: out of device memory (%s): the net needs %lld bytes for %d frames and %d stages "
                    "(%lld allocated when it failed); plan fewer frames or a shallower hook", what, (long long)planned, max_frames, ns,
                    (long long)bytes);
    }
    ~i2v_swin() {
        for (void* p : allocs) (void)hipFree(p);
    }
    float* stream_after(Stage& S, size_t b) { return b + 1 < S.blocks.size() ? S.blocks[b + 1].x : S.out; }
    const float* grad_at(int stage) const {
        for (size_t i = 0; i < hook_stage.size(); ++i)
            if (hook_stage[i] == stage) return hook_grad[i];
        return nullptr;
    }
};

namespace {

int swin_plan(i2v_swin* n, const float* const* w, int nw, const int32_t* hooks, int n_hooks) {
    const i2v_swin_config& c = n->cfg;
    if (c.img <= 0 || c.patch <= 0 || c.patch % 4 != 0 || c.img % c.patch != 0 || c.in_chans <= 0 || c.dim <= 0 || c.dim % 4 != 0 ||
        c.stages <= 0 || c.stages > I2V_SWIN_MAX_STAGES || !(c.window == 7 || c.window == 4))
        return fail("i2v_swin_create: unsupported configuration (img %d patch %d dim %d window %d stages %d)", c.img, c.patch, c.dim, c.window,
                    c.stages);
    const int dh = c.window == 7 ? 32 : 16;
    n->gsz = c.img / c.patch;
    for (int i = 0; i < c.stages; ++i) {
        const int width = c.dim << i;
        if (c.depths[i] <= 0 || c.heads[i] <= 0 || c.heads[i] * dh != width)
            return fail("i2v_swin_create: stage %d has %d blocks and %d heads at width %d (head width %d with window %d)", i, c.depths[i],
                        c.heads[i], width, dh, c.window);
        if (n->gsz % (1 << i) != 0 || (n->gsz >> i) % c.window != 0)
            return fail("i2v_swin_create: the %d x %d grid of stage %d is not a whole number of %d x %d windows", n->gsz >> i, n->gsz >> i, i,
                        c.window, c.window);
    }
    if (n_hooks <= 0) return fail("i2v_swin_create: no hooks");
    int deepest = -1;
    for (int i = 0; i < n_hooks; ++i) {
        if (hooks[i] < 0 || hooks[i] >= c.stages) return fail("i2v_swin_create: hook stage %d outside 0..%d", hooks[i], c.stages - 1);
        for (int j = 0; j < i; ++j)
            if (hooks[j] == hooks[i]) return fail("i2v_swin_create: stage %d hooked twice", hooks[i]);
        deepest = hooks[i] > deepest ? hooks[i] : deepest;
    }
    n->ns = deepest + 1;
    const int64_t F = n->max_frames, KP = (int64_t)c.in_chans * c.patch * c.patch, NI = (int64_t)(2 * c.window - 1) * (2 * c.window - 1);
    const int64_t T0 = (int64_t)n->gsz * n->gsz, D0 = c.dim;
    // every size of the plan in floats, in 64 bits, before the first allocation
    std::vector<int64_t> sizes = {D0 * KP, D0, D0, D0};
    int64_t acts = F * T0 * KP + F * T0 * D0 + 2 * F * T0;                     // patches, emb, embedding LN stats
    for (int i = 0; i < n->ns; ++i) {
        const int64_t D = D0 << i, FT = F * (T0 >> (2 * i));
        for (int b = 0; b < c.depths[i]; ++b) {
            for (int64_t v : {D, D, 3 * D * D, 3 * D, NI * c.heads[i], D * D, D, D, D, 4 * D * D, 4 * D, 4 * D * D, D}) sizes.push_back(v);
            acts += FT * D + 3 * FT * D + FT * D + 4 * FT * D + 4 * FT;         // x, qkv, y, h, stats
        }
        acts += FT * D;                                                         // the stage's output stream
        if (i + 1 < n->ns) {
            for (int64_t v : {4 * D, 4 * D, 8 * D * D}) sizes.push_back(v);
            acts += FT * D + 2 * (FT / 4);                                      // gathered rows, their LN stats
        }
    }
    const int64_t FT0 = F * T0;
    acts += FT0 * D0 + 4 * FT0 * D0 + 3 * FT0 * D0 + FT0 * D0;                  // shared scratch: t1, t2, dqkv, G (stage 0 is the largest)
    for (int i = 0; i < n_hooks; ++i) acts += F * (T0 >> (2 * hooks[i])) * (D0 << hooks[i]);
    if ((int)sizes.size() != nw) return fail("i2v_swin_create: %d weight arrays given, %zu expected for %d stages", nw, sizes.size(), n->ns);
    int64_t total = acts;
    for (int64_t v : sizes) total += v;
    n->planned = total * 4;
    if (FT0 > 0x7fffffffLL / 4) return fail("i2v_swin_create: %lld bytes needed: too many frames for one net", (long long)n->planned);
    std::vector<const float*> dev(sizes.size());
    for (size_t i = 0; i < sizes.size(); ++i) {
        if (!w[i]) return fail("i2v_swin_create: weight array %zu is null", i);
        float* p = n->alloc(sizes[i]);
        if (!p) return n->oom("weights");
        HCHK(hipMemcpy(p, w[i], (size_t)sizes[i] * 4, hipMemcpyHostToDevice));
        dev[i] = p;
    }
    n->pe_w = dev[0]; n->pe_b = dev[1]; n->pe_nw = dev[2]; n->pe_nb = dev[3];
    if (!(n->patches = n->alloc(F * T0 * KP)) || !(n->emb = n->alloc(F * T0 * D0)) || !(n->estats = n->alloc(2 * F * T0)))
        return n->oom("embedding");
    size_t wi = 4;
    n->stages.resize(n->ns);
    for (int i = 0; i < n->ns; ++i) {
        Stage& S = n->stages[i];
        S.grid = n->gsz >> i; S.width = c.dim << i; S.heads = c.heads[i];
        S.ws = c.window;
        const int64_t D = S.width, FT = F * S.T();
        S.blocks.resize(c.depths[i]);
        for (int b = 0; b < c.depths[i]; ++b) {
            Block& B = S.blocks[b];
            const float* const* q = &dev[wi];
            wi += 13;
            B.n1w = q[0]; B.n1b = q[1]; B.qkvw = q[2]; B.qkvb = q[3]; B.table = q[4]; B.projw = q[5]; B.projb = q[6];
            B.n2w = q[7]; B.n2b = q[8]; B.fc1w = q[9]; B.fc1b = q[10]; B.fc2w = q[11]; B.fc2b = q[12];
            B.shift = (b % 2 == 1 && S.grid > S.ws) ? S.ws / 2 : 0;
            if (!(B.x = n->alloc(FT * D)) || !(B.qkv = n->alloc(3 * FT * D)) || !(B.y = n->alloc(FT * D)) || !(B.h = n->alloc(4 * FT * D)) ||
                !(B.stats = n->alloc(4 * FT)))
                return n->oom("saved activations of a block");
        }
        if (!(S.out = n->alloc(FT * D))) return n->oom("a stage's output");
        if (i + 1 < n->ns) {
            S.mnw = dev[wi]; S.mnb = dev[wi + 1]; S.mred = dev[wi + 2];
            wi += 3;
            if (!(S.mg = n->alloc(FT * D)) || !(S.mstats = n->alloc(2 * (FT / 4)))) return n->oom("patch merging");
        }
    }
    if (!(n->t1 = n->alloc(FT0 * D0)) || !(n->t2 = n->alloc(4 * FT0 * D0)) || !(n->dqkv = n->alloc(3 * FT0 * D0)) || !(n->G = n->alloc(FT0 * D0)))
        return n->oom("scratch");
    for (int i = 0; i < n_hooks; ++i) {
        const Stage& S = n->stages[hooks[i]];
        const int64_t cnt = F * S.T() * S.width;
        n->hook_stage.push_back(hooks[i]);
        float* g = n->alloc(cnt);
        if (!g) return n->oom("hook gradients");
        HCHK(hipMemset(g, 0, (size_t)cnt * 4));
        n->hook_grad.push_back(g);
    }
    return 0;
}

}  // namespace

extern "C" int i2v_swin_create(int device, const i2v_swin_config* cfg, const float* const* weights, int n_weights, const int32_t* hook_stages,
                               int n_hooks, int max_frames, i2v_swin_handle* out) {
    if (!cfg || !weights || !hook_stages || !out) return fail("i2v_swin_create: null argument");
    if (max_frames <= 0) return fail("i2v_swin_create: max_frames must be positive");
    *out = nullptr;
    HCHK(hipSetDevice(device));
    i2v_swin* n = new i2v_swin();
    n->cfg = *cfg;
    n->device = device;
    n->max_frames = max_frames;
    if (swin_plan(n, weights, n_weights, hook_stages, n_hooks) != 0) {
        delete n;
        return 1;
    }
    *out = n;
    return 0;
}

extern "C" int i2v_swin_destroy(i2v_swin_handle net) {
    delete net;
    return 0;
}

extern "C" int64_t i2v_swin_workspace_bytes(i2v_swin_handle net) { return net ? net->bytes : -1; }

extern "C" int i2v_swin_forward(i2v_swin_handle n, const float* x, int frames, void* stream) {
    if (!n || !x) return fail("i2v_swin_forward: null argument");
    if (frames <= 0 || frames > n->max_frames) return fail("i2v_swin_forward: %d frames, the net is planned for 1..%d", frames, n->max_frames);
    hipStream_t s = (hipStream_t)stream;
    const i2v_swin_config& c = n->cfg;
    n->frames = frames;
    const int64_t esp = (int64_t)n->max_frames * n->gsz * n->gsz;
    VCHK(embed(x, frames, c.in_chans, n->gsz, c.patch, n->pe_w, n->pe_b, n->pe_nw, n->pe_nb, c.ln_eps, c.dim, n->patches, n->emb, n->estats,
               n->estats + esp, n->stages[0].blocks[0].x, s));
    for (int i = 0; i < n->ns; ++i) {
        Stage& S = n->stages[i];
        const int D = S.width, g = S.grid, dh = D / S.heads;
        const int64_t FT = frames * S.T(), sp = n->max_frames * S.T();
        const int M = (int)FT;
        for (size_t b = 0; b < S.blocks.size(); ++b) {
            Block& B = S.blocks[b];
            float* st = B.stats;                                   // [mean1 | rstd1 | mean2 | rstd2], at max_frames spacing
            VCHK(vit_layernorm(B.x, FT, D, B.n1w, B.n1b, c.ln_eps, n->t1, st, st + sp, s));
            VCHK(linear(n->t1, M, D, B.qkvw, B.qkvb, 3 * D, nullptr, B.qkv, nullptr, s));
            VCHK(swin_window_attention(B.qkv, frames, g, g, S.ws, B.shift, S.heads, dh, B.table, n->t1, s));
            VCHK(linear(n->t1, M, D, B.projw, B.projb, D, B.x, B.y, nullptr, s));             // y = x + proj(attn)
            VCHK(vit_layernorm(B.y, FT, D, B.n2w, B.n2b, c.ln_eps, n->t1, st + 2 * sp, st + 3 * sp, s));
            VCHK(linear(n->t1, M, D, B.fc1w, B.fc1b, 4 * D, nullptr, B.h, n->t2, s));         // h = fc1(LN2(y)), t2 = gelu(h)
            VCHK(linear(n->t2, M, 4 * D, B.fc2w, B.fc2b, D, B.y, n->stream_after(S, b), nullptr, s));
        }
        if (i + 1 < n->ns) {                                       // patch merging: gather, LayerNorm over 4 width, reduce to 2 width
            VCHK(swin_merge_gather(S.out, frames, g, g, D, S.mg, s));
            VCHK(vit_layernorm(S.mg, FT / 4, 4 * D, S.mnw, S.mnb, c.ln_eps, n->t1, S.mstats, S.mstats + sp / 4, s));
            VCHK(linear(n->t1, M / 4, 4 * D, S.mred, nullptr, 2 * D, nullptr, n->stages[i + 1].blocks[0].x, nullptr, s));
        }
    }
    return 0;
}

extern "C" int i2v_swin_backward(i2v_swin_handle n, float* gx, int accumulate, void* stream) {
    if (!n || !gx) return fail("i2v_swin_backward: null argument");
    if (n->frames <= 0) return fail("i2v_swin_backward: no forward pass to differentiate");
    hipStream_t s = (hipStream_t)stream;
    const i2v_swin_config& c = n->cfg;
    const int frames = n->frames;
    for (int i = n->ns - 1; i >= 0; --i) {
        Stage& S = n->stages[i];
        const int D = S.width, g = S.grid, dh = D / S.heads;
        const int64_t FT = frames * S.T(), sp = n->max_frames * S.T();
        const int M = (int)FT;
        if (i + 1 < n->ns) {
            // G holds the gradient of the next stage's input (FT / 4 rows of 2 width): back through the reduction, the LayerNorm and the
            // gather, plus this stage's own hook gradient when it has one
            VCHK(linear_bwd(n->G, M / 4, 2 * D, S.mred, 4 * D, nullptr, n->t1, s));
            VCHK(vit_layernorm_bwd(n->t1, S.mg, S.mstats, S.mstats + sp / 4, S.mnw, FT / 4, 4 * D, nullptr, nullptr, n->dqkv, s));
            VCHK(swin_merge_scatter(n->dqkv, frames, g, g, D, n->grad_at(i), n->G, s));
        }
        for (int b = (int)S.blocks.size() - 1; b >= 0; --b) {
            Block& B = S.blocks[b];
            const float* st = B.stats;
            // gradient of the stream after block b: the deepest stage's hook view for the very last block, the running gradient G otherwise
            const float* gin = (i == n->ns - 1 && b == (int)S.blocks.size() - 1) ? n->grad_at(i) : n->G;
            VCHK(linear_bwd(gin, M, D, B.fc2w, 4 * D, B.h, n->t2, s));                      // dh = (g fc2) * gelu'(h)
            VCHK(linear_bwd(n->t2, M, 4 * D, B.fc1w, D, nullptr, n->t1, s));                // d LN2 out
            VCHK(vit_layernorm_bwd(n->t1, B.y, st + 2 * sp, st + 3 * sp, B.n2w, FT, D, gin, nullptr, n->G, s));   // G = dy
            VCHK(linear_bwd(n->G, M, D, B.projw, D, nullptr, n->t1, s));                    // d attention out
            VCHK(swin_window_attention_bwd(B.qkv, n->t1, frames, g, g, S.ws, B.shift, S.heads, dh, B.table, n->dqkv, s));
            VCHK(linear_bwd(n->dqkv, M, 3 * D, B.qkvw, D, nullptr, n->t1, s));              // d LN1 out
            VCHK(vit_layernorm_bwd(n->t1, B.x, st, st + sp, B.n1w, FT, D, n->G, nullptr, n->G, s));   // G = dx
        }
    }
    const int64_t esp = (int64_t)n->max_frames * n->gsz * n->gsz;
    return embed_bwd(n->G, frames, c.in_chans, n->gsz, c.patch, n->pe_w, n->pe_nw, c.dim, n->emb, n->estats, n->estats + esp, n->t1, n->patches,
                     gx, accumulate, s);
}

extern "C" int i2v_swin_hook_info(i2v_swin_handle n, int hook, float** act, int64_t* act_stride, float** grad, int64_t* grad_stride, int64_t* D) {
    if (!n || hook < 0 || hook >= (int)n->hook_stage.size()) return fail("i2v_swin_hook_info: no hook %d", hook);
    const Stage& S = n->stages[n->hook_stage[hook]];
    const int64_t d = S.T() * S.width;
    if (act) *act = S.out;
    if (act_stride) *act_stride = d;
    if (grad) *grad = n->hook_grad[hook];
    if (grad_stride) *grad_stride = d;
    if (D) *D = d;
    return 0;
}

extern "C" int i2v_swin_read_hook(i2v_swin_handle n, int hook, int which, float* out, int frames, void* stream) {
    if (!n || !out || hook < 0 || hook >= (int)n->hook_stage.size()) return fail("i2v_swin_read_hook: no hook %d", hook);
    if (frames <= 0 || frames > n->max_frames) return fail("i2v_swin_read_hook: %d frames, the net is planned for 1..%d", frames, n->max_frames);
    const Stage& S = n->stages[n->hook_stage[hook]];
    const float* src = which ? n->hook_grad[hook] : S.out;
    HCHK(hipMemcpyAsync(out, src, (size_t)frames * S.T() * S.width * 4, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return 0;
}

// ---- the kernels on their own ----
extern "C" int i2v_swin_window_attention_f32(const float* qkv, int frames, int H, int W, int window, int shift, int heads, int dh,
                                             const float* table, float* out, void* stream) {
    return swin_window_attention(qkv, frames, H, W, window, shift, heads, dh, table, out, (hipStream_t)stream);
}
extern "C" int i2v_swin_window_attention_bwd_f32(const float* qkv, const float* dout, int frames, int H, int W, int window, int shift,
                                                 int heads, int dh, const float* table, float* dqkv, void* stream) {
    return swin_window_attention_bwd(qkv, dout, frames, H, W, window, shift, heads, dh, table, dqkv, (hipStream_t)stream);
}
extern "C" int i2v_swin_merge_f32(const float* x, int frames, int H, int W, int C, float* out, void* stream) {
    return swin_merge_gather(x, frames, H, W, C, out, (hipStream_t)stream);
}
extern "C" int i2v_swin_merge_bwd_f32(const float* dout, int frames, int H, int W, int C, float* dx, int accumulate, void* stream) {
    return swin_merge_scatter(dout, frames, H, W, C, accumulate ? dx : nullptr, dx, (hipStream_t)stream);
}
extern "C" int i2v_swin_embed_f32(const float* img, int frames, int in_chans, int g, int patch, const float* W, const float* b,
                                  const float* norm_w, const float* norm_b, float eps, int dim, float* patches, float* emb, float* mean,
                                  float* rstd, float* tokens, void* stream) {
    return embed(img, frames, in_chans, g, patch, W, b, norm_w, norm_b, eps, dim, patches, emb, mean, rstd, tokens, (hipStream_t)stream);
}
extern "C" int i2v_swin_embed_bwd_f32(const float* dtokens, int frames, int in_chans, int g, int patch, const float* W, const float* norm_w,
                                      int dim, const float* emb, const float* mean, const float* rstd, float* demb, float* patches,
                                      float* gimg, int accumulate, void* stream) {
    return embed_bwd(dtokens, frames, in_chans, g, patch, W, norm_w, dim, emb, mean, rstd, demb, patches, gimg, accumulate, (hipStream_t)stream);
}
