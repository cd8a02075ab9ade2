// What the transformer planners share (ViT / DeiT, Swin, ConvNeXt, MLP-Mixer / ResMLP, CaiT, ConViT, XCiT, Twins, BEiT):
//   - error reporting, the arena that owns a net's device memory, the weight upload, the hook list with its gradient views;
//   - the seven C entries of a family as function templates (xf_create .. xf_read_hook): the null, frame-range and no-forward guards and
//     the hook lookup are written here once, a planner's extern "C" functions are one-line calls and bring their own name for the refusals;
//   - the linear launches (linear, linear_bwd, linear_bwd_add) and the stems built from them: patch_rows (patchify + Linear) with its
//     backward, the same behind prefix rows, and the LayerNorm stem of Swin and ConvNeXt;
//   - attention composed from the shared launches (xf_attention / xf_attention_bwd: batched vit_gemm, the row softmax, and their backward)
//     over separate q, k and v operands: ViT's attention, and the developer routes I2V_BEIT_ATTN=0 and I2V_TWINS_ATTN=0;
//   - the pre-norm block -- seven launches forward, seven backward, with the family's attention step passed in as a callable -- and the
//     ViT-shaped stack of such blocks (XfStack: ViT, CaiT, BEiT; ConViT uses its pieces on either side of its join).
// A family brings its config, its plan sizes, its attention step and its own kernels.  Internal: each planner includes it once.
#pragma once
#ifdef __HIP__
#include <hip/hip_runtime.h>
#else
#include "i2v_xf_host.h"      // (no HIP: the host simulation's build)
#endif
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "i2v_kernels.h"
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

// y (M, N) = x (M, K) W^T (+ bias) (+ residual), W (N, K).  `residual` may BE y (the ConvNeXt blocks run in place): vit_gemm reads
// R[m][n] and writes C[m][n] in the one thread that owns the element, after its whole K loop, and never splits K across blocks
// (i2v_vit_kernels.h states it); x must not overlap y.
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

// dx (M, K) = dy (M, N) W + add, W (N, K): linear_bwd with vit_gemm's residual operand (which may be dx itself)
int linear_bwd_add(const float* dy, int M, int N, const float* W, int K, const float* add, float* dx, hipStream_t s) {
    VitGemm g{};
    g.A = dy; g.a_sm = N; g.a_sk = 1;
    g.B = W; g.b_sk = K; g.b_sn = 1;
    g.C = dx; g.c_sm = K;
    g.R = add;
    g.M = M; g.N = K; g.K = N; g.batch = 1; g.nb_in = 1; g.alpha = 1.f;
    g.mode = VIT_EPI_PLAIN;
    return vit_gemm(g, s);
}

// The stem of a patch embedding: the gsz x gsz patches of P x P pixels of F frames as rows, and their Linear into out (F gsz^2, dim)
int patch_rows(const float* img, int F, int Cin, int gsz, int P, const float* W, const float* b, int dim, float* patches, float* out,
               hipStream_t s) {
    VCHK(vit_patchify(img, patches, F, Cin, gsz, gsz, P, nullptr, 0, s));
    return linear(patches, F * gsz * gsz, Cin * P * P, W, b, dim, nullptr, out, nullptr, s);
}

// ... and its backward: the rows' gradient times W, back to the image (written, or added with `accumulate`)
int patch_rows_bwd(const float* drows, int F, int Cin, int gsz, int P, const float* W, int dim, float* patches, float* gimg, int accumulate,
                   hipStream_t s) {
    VCHK(linear_bwd(drows, F * gsz * gsz, dim, W, Cin * P * P, nullptr, patches, s));
    return vit_patchify(nullptr, patches, F, Cin, gsz, gsz, P, gimg, accumulate, s);
}

// The same behind `npre` prefix rows per frame: the patch rows' gradient is the token gradient without the prefix rows (a slice from row
// npre of each frame, read in place by the GEMM), times W
int patch_rows_bwd_prefix(const float* dtok, int F, int Cin, int gsz, int P, const float* W, int dim, int npre, float* patches, float* gimg,
                          int accumulate, hipStream_t s) {
    const int np = gsz * gsz, KP = Cin * P * P;
    VitGemm g{};
    g.A = dtok + (int64_t)npre * dim; g.a_bo = (int64_t)(np + npre) * dim; g.a_sm = dim; g.a_sk = 1;
    g.B = W; g.b_sk = KP; g.b_sn = 1;
    g.C = patches; g.c_bo = (int64_t)np * KP; g.c_sm = KP;
    g.M = np; g.N = KP; g.K = dim; g.batch = F; g.nb_in = 1; g.alpha = 1.f;
    VCHK(vit_gemm(g, s));
    return vit_patchify(nullptr, patches, F, Cin, gsz, gsz, P, gimg, accumulate, s);
}

// The LayerNorm stem (Swin, ConvNeXt): patch rows, Linear with bias into emb, LayerNorm into tokens -- and its backward
int ln_stem(const float* img, int F, int Cin, int gsz, int P, const float* W, const float* b, const float* nw, const float* nb, float eps,
            int dim, float* patches, float* emb, float* mean, float* rstd, float* tokens, hipStream_t s) {
    VCHK(patch_rows(img, F, Cin, gsz, P, W, b, dim, patches, emb, s));
    return vit_layernorm(emb, (int64_t)F * gsz * gsz, dim, nw, nb, eps, tokens, mean, rstd, s);
}

int ln_stem_bwd(const float* dtok, int F, int Cin, int gsz, int P, const float* W, const float* nw, int dim, const float* emb,
                const float* mean, const float* rstd, float* demb, float* patches, float* gimg, int accumulate, hipStream_t s) {
    VCHK(vit_layernorm_bwd(dtok, emb, mean, rstd, nw, (int64_t)F * gsz * gsz, dim, nullptr, nullptr, demb, s));
    return patch_rows_bwd(demb, F, Cin, gsz, P, W, dim, patches, gimg, accumulate, s);
}

// Attention composed from the shared launches, over batch = frames x heads (outer = frame, inner = head).  Element (f, h, row, d) of q is
// q[f * q_fs + h * dh + row * q_rs + d]; k and v share kv_fs and kv_rs; dq, dk and dv are laid out as q, k and v; out and dout are
// (F, Tq, heads * dh).  P and the score gradient are (F, heads, Tq, ld) with rows of ld = xf_probs_ld(Tk) floats.
struct XfAttn {
    const float *q, *k, *v;
    int64_t q_fs, q_rs, kv_fs, kv_rs;
    int F, Tq, Tk, heads, dh;
    float scale;
};

int xf_probs_ld(int Tk) { return (Tk + 3) / 4 * 4; }

// C[f, h] (M, N) = alpha A[f, h] (M, K) B[f, h] (K, N)
int xf_bgemm(const XfAttn& a, const float* A, int64_t a_bo, int64_t a_bi, int64_t a_sm, int64_t a_sk, const float* B, int64_t b_bo, int64_t b_bi,
             int64_t b_sk, int64_t b_sn, float* C, int64_t c_bo, int64_t c_bi, int64_t c_sm, int M, int N, int K, float alpha, hipStream_t s) {
    VitGemm g{};
    g.A = A; g.a_bo = a_bo; g.a_bi = a_bi; g.a_sm = a_sm; g.a_sk = a_sk;
    g.B = B; g.b_bo = b_bo; g.b_bi = b_bi; g.b_sk = b_sk; g.b_sn = b_sn;
    g.C = C; g.c_bo = c_bo; g.c_bi = c_bi; g.c_sm = c_sm;
    g.M = M; g.N = N; g.K = K; g.batch = a.F * a.heads; g.nb_in = a.heads; g.alpha = alpha;
    g.mode = VIT_EPI_PLAIN;
    return vit_gemm(g, s);
}

// out = softmax(scale q k^T) v with P kept; `mid()` runs between the score product and the softmax (BEiT adds its bias there)
template <class Mid>
int xf_attention(const XfAttn& a, float* P, float* out, hipStream_t s, Mid mid) {
    const int dh = a.dh, C = a.heads * dh, ld = xf_probs_ld(a.Tk);
    const int64_t ps = (int64_t)a.Tq * ld, hps = a.heads * ps;
    VCHK(xf_bgemm(a, a.q, a.q_fs, dh, a.q_rs, 1, a.k, a.kv_fs, dh, 1, a.kv_rs, P, hps, ps, ld, a.Tq, a.Tk, dh, a.scale, s));    // S = scale q k^T
    VCHK(mid());
    VCHK(vit_softmax(P, (int64_t)a.F * a.heads * a.Tq, a.Tk, ld, s));
    return xf_bgemm(a, P, hps, ps, ld, 1, a.v, a.kv_fs, dh, a.kv_rs, 1, out, (int64_t)a.Tq * C, dh, C, a.Tq, dh, a.Tk, 1.f, s);  // out = P v
}

int xf_attention(const XfAttn& a, float* P, float* out, hipStream_t s) {
    return xf_attention(a, P, out, s, [] { return 0; });
}

// ... and its backward: dout -> dq, dk, dv, with dS (the size of P) as scratch
int xf_attention_bwd(const XfAttn& a, const float* P, const float* dout, float* dS, float* dq, float* dk, float* dv, hipStream_t s) {
    const int dh = a.dh, C = a.heads * dh, ld = xf_probs_ld(a.Tk);
    const int64_t ps = (int64_t)a.Tq * ld, hps = a.heads * ps, os = (int64_t)a.Tq * C;
    VCHK(xf_bgemm(a, dout, os, dh, C, 1, a.v, a.kv_fs, dh, 1, a.kv_rs, dS, hps, ps, ld, a.Tq, a.Tk, dh, 1.f, s));              // dP = dout v^T
    VCHK(vit_softmax_bwd(dS, P, (int64_t)a.F * a.heads * a.Tq, a.Tk, ld, a.scale, s));        // dS = scale * P (dP - rowsum(dP P))
    VCHK(xf_bgemm(a, dS, hps, ps, ld, 1, a.k, a.kv_fs, dh, a.kv_rs, 1, dq, a.q_fs, dh, a.q_rs, a.Tq, dh, a.Tk, 1.f, s));       // dq = dS k
    VCHK(xf_bgemm(a, dS, hps, ps, 1, ld, a.q, a.q_fs, dh, a.q_rs, 1, dk, a.kv_fs, dh, a.kv_rs, a.Tk, dh, a.Tq, 1.f, s));       // dk = dS^T q
    return xf_bgemm(a, P, hps, ps, 1, ld, dout, os, dh, C, 1, dv, a.kv_fs, dh, a.kv_rs, a.Tk, dh, a.Tq, 1.f, s);               // dv = P^T dout
}

// q, k and v of head h at columns h dh, C + h dh and 2 C + h dh of qkv (F, T, 3 C)
XfAttn xf_attn_qkv(const float* qkv, int F, int T, int heads, int dh, float scale) {
    const int C = heads * dh;
    return {qkv, qkv + C, qkv + 2 * C, 3LL * C * T, 3 * C, 3LL * C * T, 3 * C, F, T, T, heads, dh, scale};
}

// Owner of a net's device memory: one hipMalloc per array of the plan.  `entry` and `unit` word the refusals of the family that plans.
struct Arena {
    const char *entry = "", *unit = "";          // "i2v_vit_create", "block"
    int max_frames = 0, depth = 0;               // what the plan was made for: frames, and blocks / stages up to the deepest hook
    std::vector<void*> allocs;
    int64_t bytes = 0, planned = 0;              // held so far; what the whole plan takes (weights, saves, scratch, hook gradients)

    Arena() = default;
    Arena(const Arena&) = delete;
    Arena& operator=(const Arena&) = delete;
    ~Arena() {
        for (void* p : allocs) (void)hipFree(p);
    }
    // the whole plan in floats, before the first allocation; the kernels count the rows of the largest stream in an int
    int plan(int64_t floats, int64_t rows) {
        planned = floats * 4;
        if (rows > 0x7fffffffLL / 4) return fail("%s: %lld bytes needed: too many frames for one net", entry, (long long)planned);
        return 0;
    }
    float* alloc(int64_t n) {
        void* p = nullptr;
        if (hipMalloc(&p, (size_t)n * 4) != hipSuccess) return nullptr;
        allocs.push_back(p);
        bytes += n * 4;
        return (float*)p;
    }
    int oom(const char* what) {                  // an allocation of the plan failed: say what the whole plan needs
        (void)hipGetLastError();
        return fail("%s: out of device memory (%s): the net needs %lld bytes for %d frames and %d %ss "
                    "(%lld allocated when it failed); plan fewer frames or a shallower hook", entry, what, (long long)planned, max_frames,
                    depth, unit, (long long)bytes);
    }
    // the host arrays `w` of `sizes` floats each, copied to the device
    int upload(const std::vector<int64_t>& sizes, const float* const* w, std::vector<const float*>& dev) {
        dev.resize(sizes.size());
        for (size_t i = 0; i < sizes.size(); ++i) {
            if (!w[i]) return fail("%s: weight array %zu is null", entry, i);
            float* p = alloc(sizes[i]);
            if (!p) return oom("weights");
            HCHK(hipMemcpy(p, w[i], (size_t)sizes[i] * 4, hipMemcpyHostToDevice));
            dev[i] = p;
        }
        return 0;
    }
};

// The hooked blocks / stages in the caller's order, and the gradient view a loss kernel writes for each.
struct Hooks {
    std::vector<int> at;
    std::vector<float*> grad;

    bool has(int hook) const { return hook >= 0 && hook < (int)at.size(); }
    const float* grad_at(int where) const {      // hook gradient of the stream after block / stage `where`, or null
        for (size_t i = 0; i < at.size(); ++i)
            if (at[i] == where) return grad[i];
        return nullptr;
    }
    // the deepest of `n` hooks below `limit`, or -1 with the refusal reported
    static int deepest(const int32_t* hooks, int n, int limit, const Arena& a) {
        if (n <= 0) return fail("%s: no hooks", a.entry), -1;
        int deep = -1;
        for (int i = 0; i < n; ++i) {
            if (hooks[i] < 0 || hooks[i] >= limit) return fail("%s: hook %s %d outside 0..%d", a.entry, a.unit, hooks[i], limit - 1), -1;
            for (int j = 0; j < i; ++j)
                if (hooks[j] == hooks[i]) return fail("%s: %s %d hooked twice", a.entry, a.unit, hooks[i]), -1;
            deep = hooks[i] > deep ? hooks[i] : deep;
        }
        return deep;
    }
    int add(Arena& a, int where, int64_t floats) {   // a zeroed gradient view of `floats` floats for a hook behind `where`
        float* g = a.alloc(floats);
        if (!g) return a.oom("hook gradients");
        HCHK(hipMemset(g, 0, (size_t)floats * 4));
        at.push_back(where);
        grad.push_back(g);
        return 0;
    }
};

// What every transformer net holds next to its family's own members.  A family's net also offers hook_stream(where), the stream behind
// block / stage `where`, and hook_floats(where), its floats per frame: the entries below read hooks through them.
struct XfNet {
    Arena arena;
    Hooks hooks;
    int device = 0, max_frames = 0, frames = 0;
    float *t1 = nullptr, *t2 = nullptr, *dqkv = nullptr, *G = nullptr;      // scratch shared by all blocks; G: the running gradient

    // gradient of the stream after block b of nb: the top hook's view for the deepest block, the running gradient G below it (where the
    // LN1 backward of block b + 1 has already added the hook at that stream); and the hook at the stream block b reads, or null
    const float* grad_in(int b, int nb) const { return b == nb - 1 ? hooks.grad_at(b) : G; }
    const float* grad_below(int b) const { return b > 0 ? hooks.grad_at(b - 1) : nullptr; }
};

// The seven C entries of a family.  `entry` is the calling function's own name and words its refusals; `unit` as in Arena.
// create: new Net on `device`, planned by `plan(net)`; *out stays null when the plan is refused
template <class Net, class Plan>
int xf_create(const char* entry, const char* unit, int device, const void* cfg, const void* weights, const void* hooks, int max_frames,
              Net** out, Plan plan) {
    if (!cfg || !weights || !hooks || !out) return fail("%s: null argument", entry);
    if (max_frames <= 0) return fail("%s: max_frames must be positive", entry);
    *out = nullptr;
    HCHK(hipSetDevice(device));
    Net* n = new Net();
    n->arena.entry = entry;
    n->arena.unit = unit;
    n->device = device;
    n->max_frames = n->arena.max_frames = max_frames;
    if (plan(n) != 0) {
        delete n;
        return 1;
    }
    *out = n;
    return 0;
}

template <class Net>
int xf_destroy(Net* n) {
    delete n;
    return 0;
}

template <class Net>
int64_t xf_workspace_bytes(const Net* n) { return n ? n->arena.bytes : -1; }

int frames_in_plan(const char* entry, int frames, int max_frames) {
    if (frames <= 0 || frames > max_frames) return fail("%s: %d frames, the net is planned for 1..%d", entry, frames, max_frames);
    return 0;
}

// forward: `run(n, x, frames, s)` is the family's launch sequence
template <class Net, class Run>
int xf_forward(const char* entry, Net* n, const float* x, int frames, void* stream, Run run) {
    if (!n || !x) return fail("%s: null argument", entry);
    VCHK(frames_in_plan(entry, frames, n->max_frames));
    n->frames = frames;
    return run(n, x, frames, (hipStream_t)stream);
}

// backward of the last forward: `run(n, gx, accumulate, s)`
template <class Net, class Run>
int xf_backward(const char* entry, Net* n, float* gx, int accumulate, void* stream, Run run) {
    if (!n || !gx) return fail("%s: null argument", entry);
    if (n->frames <= 0) return fail("%s: no forward pass to differentiate", entry);
    return run(n, gx, accumulate, (hipStream_t)stream);
}

template <class Net>
int xf_hook_info(const char* entry, Net* n, int hook, float** act, int64_t* act_stride, float** grad, int64_t* grad_stride, int64_t* D) {
    if (!n || !n->hooks.has(hook)) return fail("%s: no hook %d", entry, hook);
    const int where = n->hooks.at[hook];
    const int64_t per_frame = n->hook_floats(where);
    if (act) *act = n->hook_stream(where);
    if (act_stride) *act_stride = per_frame;
    if (grad) *grad = n->hooks.grad[hook];
    if (grad_stride) *grad_stride = per_frame;
    if (D) *D = per_frame;
    return 0;
}

// which: 0 the hooked activation, else its gradient view
template <class Net>
int xf_read_hook(const char* entry, Net* n, int hook, int which, float* out, int frames, void* stream) {
    if (!n || !out || !n->hooks.has(hook)) return fail("%s: no hook %d", entry, hook);
    VCHK(frames_in_plan(entry, frames, n->max_frames));
    const int where = n->hooks.at[hook];
    const float* src = which ? n->hooks.grad[hook] : n->hook_stream(where);
    HCHK(hipMemcpyAsync(out, src, (size_t)frames * n->hook_floats(where) * 4, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return 0;
}

struct Block {
    const float *n1w, *n1b, *qkvw, *qkvb, *projw, *projb, *n2w, *n2b, *fc1w, *fc1b, *fc2w, *fc2b;
    float *x, *qkv, *y, *h, *stats;        // saved per block: input stream, qkv, mid stream, fc1 pre-activation, LN stats
    float* P = nullptr;                    // ViT: the saved attention probabilities
    const float* table = nullptr;          // Swin: the relative position bias table, and the window shift
    int shift = 0;

    // native order: norm1 and qkv at a[0..3]; proj, norm2, fc1 and fc2 at p[0..7] (a family may keep arrays of its own between them)
    void weights(const float* const* a, const float* const* p) {
        n1w = a[0]; n1b = a[1]; qkvw = a[2]; qkvb = a[3]; projw = p[0]; projb = p[1];
        n2w = p[2]; n2b = p[3]; fc1w = p[4]; fc1b = p[5]; fc2w = p[6]; fc2b = p[7];
    }
    // the saves of a block over FT rows, D wide, with an MLP of Hm: x, qkv, P (`probs` floats, when the family keeps them there), y, h, stats
    int alloc_saves(Arena& A, int64_t FT, int64_t D, int64_t Hm, int64_t probs) {
        if (!(x = A.alloc(FT * D)) || !(qkv = A.alloc(FT * 3 * D)) || (probs && !(P = A.alloc(probs))) || !(y = A.alloc(FT * D)) ||
            !(h = A.alloc(FT * Hm)) || !(stats = A.alloc(4 * FT)))
            return A.oom("saved activations of a block");
        return 0;
    }
};

// One run of blocks over `frames` frames of T tokens, D wide: `sp` is the spacing of the four LN statistics (max_frames * T).
struct BlockRun {
    int frames, T, D, mlp;
    int64_t sp;
    float ln_eps;
    float *t1, *t2, *dqkv, *G;
    hipStream_t s;
};

// x' = y + fc2(gelu(fc1(LN2 y))), y = x + proj(attn(qkv(LN1 x))) into `out`; `attn(B, o)` writes the attention output of B.qkv to o
template <class Attn>
int block_forward(const Block& B, const BlockRun& r, float* out, Attn attn) {
    const int M = r.frames * r.T, D = r.D;
    const int64_t FT = (int64_t)r.frames * r.T, sp = r.sp;
    float* st = B.stats;                                   // [mean1 | rstd1 | mean2 | rstd2], FT each at max_frames spacing
    VCHK(vit_layernorm(B.x, FT, D, B.n1w, B.n1b, r.ln_eps, r.t1, st, st + sp, r.s));
    VCHK(linear(r.t1, M, D, B.qkvw, B.qkvb, 3 * D, nullptr, B.qkv, nullptr, r.s));
    VCHK(attn(B, r.t1));
    VCHK(linear(r.t1, M, D, B.projw, B.projb, D, B.x, B.y, nullptr, r.s));               // y = x + proj(attn)
    VCHK(vit_layernorm(B.y, FT, D, B.n2w, B.n2b, r.ln_eps, r.t1, st + 2 * sp, st + 3 * sp, r.s));
    VCHK(linear(r.t1, M, D, B.fc1w, B.fc1b, r.mlp, nullptr, B.h, r.t2, r.s));            // h = fc1(LN2(y)), t2 = gelu(h)
    return linear(r.t2, M, r.mlp, B.fc2w, B.fc2b, D, B.y, out, nullptr, r.s);            // x' = y + fc2(gelu(h))
}

// `gin`: gradient of the stream after the block; leaves the gradient of its input in G, plus `add1` (a hook at that stream) when given.
// `attn_bwd(B, dout)` writes r.dqkv from the attention output's gradient
template <class AttnBwd>
int block_backward(const Block& B, const BlockRun& r, const float* gin, const float* add1, AttnBwd attn_bwd) {
    const int M = r.frames * r.T, D = r.D;
    const int64_t FT = (int64_t)r.frames * r.T, sp = r.sp;
    const float* st = B.stats;
    VCHK(linear_bwd(gin, M, D, B.fc2w, r.mlp, B.h, r.t2, r.s));                          // dh = (g fc2) * gelu'(h)
    VCHK(linear_bwd(r.t2, M, r.mlp, B.fc1w, D, nullptr, r.t1, r.s));                     // d LN2 out
    VCHK(vit_layernorm_bwd(r.t1, B.y, st + 2 * sp, st + 3 * sp, B.n2w, FT, D, gin, nullptr, r.G, r.s));   // G = dy
    VCHK(linear_bwd(r.G, M, D, B.projw, D, nullptr, r.t1, r.s));                         // d attention out
    VCHK(attn_bwd(B, r.t1));
    VCHK(linear_bwd(r.dqkv, M, 3 * D, B.qkvw, D, nullptr, r.t1, r.s));                   // d LN1 out
    return vit_layernorm_bwd(r.t1, B.x, st, st + sp, B.n1w, FT, D, r.G, add1, r.G, r.s); // G = dx (+ hook)
}

// The sizes every ViT-shaped family refuses alike (a family adds its own conditions and words the refusal itself)
template <class Cfg>
bool vit_shape_ok(const Cfg& c) {
    return c.img > 0 && c.patch > 0 && c.img % c.patch == 0 && c.patch % 4 == 0 && c.in_chans > 0 && c.dim > 0 && c.heads > 0 &&
           c.dim % c.heads == 0 && c.dim % 4 == 0 && c.mlp > 0 && c.mlp % 4 == 0 && c.blocks > 0;
}

// A ViT-shaped net: nb pre-norm blocks over T tokens, cfg.dim wide; the stream after block b is block b + 1's saved input, or x_top.
template <class Cfg, class Blk = Block>
struct XfStack : XfNet {
    Cfg cfg{};
    int T = 0, gsz = 0, nb = 0;
    float scale = 0.f;
    std::vector<Blk> blocks;
    float* x_top = nullptr;                      // stream after the last block run

    float* stream_after(int b) { return b + 1 < nb ? blocks[b + 1].x : x_top; }
    float* hook_stream(int b) { return stream_after(b); }
    int64_t hook_floats(int) const { return (int64_t)T * cfg.dim; }
    BlockRun run(int frames, hipStream_t s) const {
        return {frames, T, cfg.dim, cfg.mlp, (int64_t)max_frames * T, cfg.ln_eps, t1, t2, dqkv, G, s};
    }
    // the blocks in order; `attn(b, out)` writes the attention output of block b
    template <class Attn>
    int forward_blocks(int frames, hipStream_t s, Attn attn) {
        const BlockRun r = run(frames, s);
        for (int b = 0; b < nb; ++b)
            VCHK(block_forward(blocks[b], r, stream_after(b), [&](const Block&, float* o) { return attn(b, o); }));
        return 0;
    }
    // ... and from the deepest down, leaving the gradient of block 0's input in G; `attn_bwd(b, dout)` writes dqkv
    template <class AttnBwd>
    int backward_blocks(int frames, hipStream_t s, AttnBwd attn_bwd) {
        const BlockRun r = run(frames, s);
        for (int b = nb - 1; b >= 0; --b)
            VCHK(block_backward(blocks[b], r, grad_in(b, nb), grad_below(b), [&](const Block&, const float* dout) { return attn_bwd(b, dout); }));
        return 0;
    }
};

}  // namespace
