// What the transformer planners share (i2v_vit.cpp, i2v_swin.cpp): error reporting, the two linear-layer launches, the arena that owns a
// net's device memory, the weight upload, the hook list with its gradient views, the create wrapper, and the pre-norm block -- seven
// launches forward, seven backward, with the family's attention step passed in as a callable.  Internal: each planner includes it once.
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

// What every transformer net holds next to its family's own members.
struct XfNet {
    Arena arena;
    Hooks hooks;
    int device = 0, max_frames = 0, frames = 0;
    float *t1 = nullptr, *t2 = nullptr, *dqkv = nullptr, *G = nullptr;      // scratch shared by all blocks; G: the running gradient
};

// new Net on `device`, planned by `plan(net)`; *out stays null when the plan is refused.  `entry` and `unit` as in Arena
template <class Net, class Plan>
int create_net(const char* entry, const char* unit, int device, int max_frames, Net** out, Plan plan) {
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

int hook_info(float* act, float* grad, int64_t per_frame, float** act_out, int64_t* act_stride, float** grad_out, int64_t* grad_stride,
              int64_t* D) {
    if (act_out) *act_out = act;
    if (act_stride) *act_stride = per_frame;
    if (grad_out) *grad_out = grad;
    if (grad_stride) *grad_stride = per_frame;
    if (D) *D = per_frame;
    return 0;
}

int read_hook(const char* entry, const float* src, int64_t per_frame, float* out, int frames, int max_frames, void* stream) {
    if (frames <= 0 || frames > max_frames) return fail("%s: %d frames, the net is planned for 1..%d", entry, frames, max_frames);
    HCHK(hipMemcpyAsync(out, src, (size_t)frames * per_frame * 4, hipMemcpyDeviceToDevice, (hipStream_t)stream));
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

}  // namespace
