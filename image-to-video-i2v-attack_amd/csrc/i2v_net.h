// What the engine units share (i2v_engine.cpp, i2v_pack.cpp, i2v_plan.cpp, i2v_tune.cpp, i2v_run.cpp, i2v_loop_api.cpp): the error
// slot, the description of a net (buffers, tensor views, nodes, packed operands), its two launch lists, and the functions that cross
// units.  Internal: nothing outside those units includes it, and nothing in it is exported from the library.
#pragma once
#include "../../include/i2v_hip.h"
#include "i2v_kernels.h"

#include <stdint.h>

#include <algorithm>
#include <deque>
#include <mutex>
#include <string>
#include <utility>
#include <vector>

namespace eng {

#pragma GCC visibility push(hidden)         // functions and variables of the engine units: shared between them, not exported
extern thread_local std::string g_err;      // what i2v_last_error() returns (defined in i2v_engine.cpp)
int fail(const char* fmt, ...);             // sets it; returns 1
#pragma GCC visibility pop

#define CHECK_BE(expr)                                                            \
    do {                                                                          \
        if ((expr) != 0) return fail("%s: %s", #expr, be_error() ? be_error() : "backend error"); \
    } while (0)

struct Buffer { int C, H, W; int T = 1; size_t act_off = 0, grad_off = 0; bool is_input = false;    // T: frames per clip (video networks)
                size_t gate_off = 0; int gate_words = 0; bool gated = false; };   // 1-bit ReLU gates: C rows of gate_words 32-bit words
struct Tensor { int buf, c_off, C; bool post_relu; float bwd_gain = 1.f; };   // bwd_gain: i2v_net_set_relu_gain

struct Packed {               // one implicit-GEMM operand set
    float* wp = nullptr; I2VKEntry* ktab = nullptr;
    float* wpc = nullptr;     // compact copy of wp for conv_igvfma_kernel (I2VConvParams::wpc)
    uint16_t* wp3 = nullptr;  // split-bf16 copy of `wp` (I2VConvParams::wp3), only in the bf16x3 math mode
    int K = 0, Kpad = 0, Cd = 0, Cdpad = 0, tap_uniform = 0;
    int halo = 0;           // 9 for a 3x3 / stride-1 / pad-1 packing in (16-channel group, tap, channel) order (kernel MODE 5), else 0
    int ph = 0, pw = 0, Hg = 0, Wg = 0;
    int pt = 0, Tg = 1;       // temporal parity class / grid frames per clip (video networks)
    int has_dt = 0;           // some k-table row carries a temporal tap offset
    int quad = 0, quad_kw = 0, quad_dw0 = 0;     // "quad rows" packing (I2VConvParams::quad): quads per row run, taps per run, first tap
    int tpair = 0;            // forward packing with TWO output frames per grid frame (rows = (frame class, channel)): see pack_fwd
    int ig_tt = 0, ig_th = 0, ig_tw = 0;      // image-gradient packing in tap-uniform order: union taps per axis (I2VConvParams::ig_*)
    int ig_p77 = 0;           // quad-row image gradient whose zero weights follow the stride-2 7 x 7 pattern (I2VConvParams::ig_p77)
};

struct Node {
    int type;                 // 0 conv, 1 maxpool, 2 avgpool, 3 attention core (non-local block), 4 squeeze-and-excitation
    // type 4 (i2v_net_add_se): fc1's weight [rd][C] and bias, fc2's weight TRANSPOSED [rd][C] and bias, host and uploaded; `se_off`: the
    // node's per-frame vectors in the arena -- m [N][C], h [N][rd], s [N][C] (forward to backward), t [N][C], dm / HW [N][C] (backward)
    i2v_se_desc sd{};
    std::vector<float> se_w1, se_b1, se_w2t, se_b2;
    float* se_w1_d = nullptr; float* se_b1_d = nullptr; float* se_w2t_d = nullptr; float* se_b2_d = nullptr;
    size_t se_off = 0, se_floats = 0;
    i2v_attn_desc ad{};       // type 3
    size_t p_off = 0;         // type 3: the attention matrix P [clips][M][N] (kept for the input-gradient pass), arena offset
    int src0() const { return type == 0 ? cd.src : type == 3 ? ad.theta : type == 4 ? sd.src : pd.src; }
    int dst0() const { return type == 0 ? cd.dst : type == 3 ? ad.dst : type == 4 ? sd.dst : pd.dst; }
    int residual0() const { return type == 0 ? cd.residual : type == 4 ? sd.residual : -1; }
    i2v_conv3d_desc cd; i2v_pool3d_desc pd;        // image nodes are stored as kt = 1 video nodes
    std::vector<float> w;     // [cout][cin][kt][kh][kw] with scale folded
    std::vector<float> shift;
    std::vector<float> pre_scale, pre_shift;      // pre-activation conv (DenseNet): per input channel
    float* shift_d = nullptr; float* pre_scale_d = nullptr; float* pre_shift_d = nullptr;   // *_d padded to Kpad
    bool preact() const { return !pre_scale.empty(); }
    Packed fwd; std::vector<Packed> bwd;
    // grouped convolution (i2v_net_add_conv_grouped): `w` above is the block-diagonal DENSE expansion (what the dense route packs and the
    // host simulation runs), `wg` the compact [cout][cin / groups][3][3] kernel, scale folded.  `gconv`: this plan runs the node on
    // k_gconv (product build, I2V_GCONV not 0) -- then only the compact operands gw_fwd / gw_bwd (I2VGConvParams::w) are uploaded.
    int groups = 1; std::vector<float> wg; bool gconv = false;
    float* gw_fwd = nullptr; float* gw_bwd = nullptr; int gw_tapmask[4] = {0, 0, 0, 0};
    // depthwise convolution (i2v_net_add_conv_depthwise): groups = C, `dw` the filter size k (0: not depthwise), `wg` the compact [C][k k]
    // filter, scale folded.  `dwconv`: this plan runs the node on k_dwconv (product build, I2V_DWCONV not 0) with the operands gw_fwd /
    // gw_bwd ([C][k k] and [class][C][k k] mirrored; gw_tapmask per class); else the dense route expands `wg` into `w` while packing.
    int dw = 0; bool dwconv = false;
    // input gradient of a convolution that reads the network input (class-packed): one launch -- or one per temporal class (pack_img)
    struct ImgGrad {
        Packed P; int blk = 0, sh = 1, blkt = 1;
        int ost = 1, ot0 = 0;                                // temporal output stride / offset
        int st = 1, oct = 1; bool skips = false;             // dz frames per grid frame, frames between its temporal classes, frames left to a memset
        double flop_share = 1.0;                             // this launch's part of the node's algorithmic flops
    };
    std::vector<ImgGrad> imgs;
    size_t idx_off = 0;                           // maxpool: arg-max bytes, arena offset in floats
};

enum Kind { L_CONV, L_IMGGRAD, L_POOLF, L_POOLB, L_ADDMASK, L_AVGF, L_AVGB, L_MEMSET, L_POOL3F, L_POOL3B, L_AGEMM, L_SOFTMAX, L_GCONV, L_DWCONV,
            L_SE_SQUEEZE, L_SE_EXCITE, L_SE_SCALE };   // L_IMGGRAD: conv_igemm with class-packed Cd
// L_GCONV: a grouped 3x3 node on k_gconv -- `gc` is what the kernel gets; `conv` carries the same views (src, dst, gate, gate_out, mask, Cd, K =
// 9 x group width) for the address-range analyses and the timing records, which treat it as the convolution launch it is
// L_DWCONV: a depthwise node on k_dwconv -- `dc` is what the kernel gets, `conv` mirrors the views in the same way (K = k k)
// L_SE_*: the three launches of a squeeze-and-excitation node per pass (`se`; se.backward tells the pass).  No pass that matches on
// L_CONV sees them; the address-range analysis (access_of, i2v_tune.cpp) reads their views (x, g, r, dst, the node's vectors) from `se`
struct Launch {
    Kind kind;
    I2VConvParams conv; I2VPoolParams pool; I2VAddMaskParams am; I2VGConvParams gc; I2VDwConvParams dc; I2VSeParams se;
    I2VAttnGemm ag; I2VSoftmaxRows sm; int sm_rows_per_clip = 0;    // L_AGEMM / L_SOFTMAX (clips are filled in at run time)
    int T = 1;                     // frames per clip of the launch's iteration space (conv launches: conv.Tg)
    bool src_is_input = false;     // conv: src pointer patched with the caller's x
    bool img_accumulate = false;   // L_IMGGRAD of a second convolution reading the input (two-pathway stems): gx += ...
    float* ms_ptr = nullptr; size_t ms_floats_per_frame = 0;   // L_MEMSET
    float* se_vec = nullptr; size_t se_vec_floats = 0;   // L_SE_*: the node's per-frame vectors (one block, Node::se_off, se_floats)
    double se_bytes_per_frame = 0; // L_SE_*: algorithmic bytes
    bool ms_gx = false;            // L_MEMSET of the caller's gradient output (skipped when accumulating)
    double alg_flops_per_frame = 0; // L_IMGGRAD: algorithmic (not class-padded) flops
    // conv launches: the autotuner's tile configuration (conv.cfg encoding) per batch bucket b = clips in (max >> (b + 1), max >> b];
    // 0: not tuned (conv.cfg as planned).  Every configuration computes the same bits, so the choice never shows in a result.
    int cfg_b[4] = {0, 0, 0, 0};
    // Fused pair (k_conv_fused): this 3x3 launch and the NEXT launch of its list, the pointwise convolution over its output, may run as
    // one kernel that never stores the intermediate.  fuse_ok: k_conv_fusable's bits, 0 when anything else reads the intermediate
    // (mark_fusable); fuse_b[bucket]: what the autotuner measured -- 0 two launches, 1 fused (plain staging), 2 fused (halo staging).
    int fuse_ok = 0;
    int fuse_b[4] = {0, 0, 0, 0};
    // Fused fast-pathway block (k_fastblock, round 6): this launch and the next fb_ok - 1 launches of its list -- forward 3: conv1, conv2,
    // conv3; 4: conv1, conv2, the projection shortcut, conv3; backward 2: the input gradients of conv3 and conv2 -- may run as ONE kernel
    // that never stores the intermediates.  0 when anything else reads an intermediate (mark_fastblocks); fb_b[bucket]: what the
    // autotuner measured (0: separate launches, 1: fused).
    int node = -1;                 // conv launches: the graph node they belong to
    int fb_ok = 0;
    int fb_b[4] = {0, 0, 0, 0};
    // Shortcut pair (k_conv_scpair): this 1x1 launch's output is nothing but the plain addend of the pointwise launch sc_ok entries
    // further down its list, it is independent of what lies between, and nothing else touches that memory (mark_fusable).  Where
    // sc_b[bucket] is set (1 without the autotuner; with it, where the pair measured faster than the two launches) the executor passes
    // over this launch and runs the pair as ONE kernel in its consumer's place: the intermediate is never stored.
    int sc_ok = 0;
    int sc_b[4] = {0, 0, 0, 0};
    bool sc_private = false;       // nothing but the consumer ever touches the intermediate's memory (a tensor's own view, not scratch that is overwritten later)
    // Launch overlap (mark_overlap, round 6): a convolution launch that does not depend on its predecessors back to launch ov_after
    // (-1: on nothing in its list) may run on the net's SIDE stream, issued right after launch ov_after, while the main stream goes on;
    // ov_join is the first later launch that touches what it writes or reads (list size: none in this list) and waits for it.
    // ov_after == -2: runs in place.  No launch changes, so no result changes.
    int ov_after = -2, ov_join = -1;
};
inline int cfg_bucket(int clips, int max_clips) {
    int b = 0;
    while (b < 3 && (max_clips >> (b + 1)) >= clips && (max_clips >> (b + 1)) >= 1) ++b;
    return b;
}

struct Addend { const float* p; int64_t nstride; int stride, H, W; };

// Address-range analysis: what the plan-time passes that fuse, move or hoist launches ask about memory.  A range is [first, second) in
// BYTES; a null operand has none and meets nothing.  extent: `frames` frames `stride` bytes apart, the last one `plane` bytes long (a
// view of a wider buffer ends with its own channels, not with the frame stride).
typedef std::pair<const char*, const char*> Range;
inline Range extent(const void* p, int64_t frames, int64_t stride, int64_t plane) {
    const char* c = (const char*)p;
    return c ? Range(c, c + (frames > 0 ? (frames - 1) * stride : 0) + std::max<int64_t>(plane, 1)) : Range(nullptr, nullptr);
}
inline bool meets(const Range& a, const Range& b) { return a.first && b.first && a.first < b.second && b.first < a.second; }
// What ONE launch reads and writes at the planned clip count (access_of, i2v_tune.cpp: the only place that lists the operands of each
// Kind).  barrier: not analysed (attention launches address whole matrices) -- reads, writes and conflicts with everything.
struct Access { std::vector<Range> r, w; bool barrier = false; };
inline int reads(const Access& a, const Range& x) {         // through how many operands (a consumer reads its producer's output through ONE)
    int c = a.barrier ? 1 : 0;
    for (const Range& q : a.r) c += meets(q, x) ? 1 : 0;
    return c;
}
inline bool writes(const Access& a, const Range& x) {
    for (const Range& q : a.w) if (meets(q, x)) return true;
    return a.barrier;
}
inline bool covers(const Access& a, const Range& x) {       // one output overwrites ALL of x: what x held is dead
    for (const Range& q : a.w) if (x.first && q.first <= x.first && q.second >= x.second) return true;
    return false;
}
inline bool conflict(const Access& a, const Access& b) {    // one writes what the other reads or writes: they may neither swap nor overlap
    if (a.barrier || b.barrier) return true;
    for (const Range& x : a.w) if (reads(b, x) || writes(b, x)) return true;
    for (const Range& x : b.w) if (reads(a, x)) return true;
    return false;
}

// A range that a planned group never stores (record_unstored): reading it back would hand out stale arena contents.
// group: 0 the intermediate of a fused 3x3 -> pointwise pair, 1 an intermediate of a fused fast-pathway block, 2 the output of a shortcut
// that runs inside a shortcut pair; remake: the launch of Net::fwd that reproduces a group-2 range on demand, -1: none (refused)
struct Unstored { Range bytes; int group; int remake; };

struct Net {
    std::vector<Buffer> bufs; std::vector<Tensor> tens; std::vector<Node> nodes;
    int input = -1; std::vector<int> hooks; int maxN = 0; bool planned = false;
    float* arena = nullptr; size_t arena_floats = 0; std::vector<void*> dev_allocs;
    std::vector<Launch> fwd, bwd;
    int frames = 0;
    int Tin() const { return bufs[tens[input].buf].T; }     // frames per clip of the input
    size_t weight_bytes = 0;
    std::vector<float*> hook_tmp;  // per hook: separate gradient buffer when the hooked tensor is also consumed
    size_t in_stage_off = 0; bool stage_input = false;   // quad-row stems read up to 64 bytes around a view: the caller's frames are
                                                         // copied into the arena (slack on both sides) before the forward pass
    // launch overlap (mark_overlap / run_list): the side stream, its event pool, and per list (0 forward, 1 backward) the hoisted
    // launches to issue right after main launch p (index p + 1; index 0: at the start of the list)
    i2v_stream_t side = nullptr; std::vector<void*> ov_ev; size_t ov_used = 0;
    std::vector<std::vector<int>> ov_at[2]; int ov_max_frames = 0;
    std::vector<Unstored> unstored;         // what i2v_net_read_tensor cannot simply copy out (record_unstored, at the end of the plan)
};

// `chain`: the launch follows the previous timed launch back to back on the same stream (same launch list), so its
// start IS that launch's stop event -- one event record per launch instead of two (the records cost ~2 us of stream
// time each, 4 % of the headline bench when every launch carried a pair).
struct TimedLaunch { void* start; void* stop; int kind; double flops; int Cd, K, HWg, frames, pw; void* chain_from; double bytes; int count = 1; };

}  // namespace eng

struct i2v_ctx {
    int device; std::vector<eng::Net*> nets; std::mutex nets_mu;     // the table: created / destroyed under the lock, ids of destroyed nets are handed out again
    // nets may be executed from several threads on several streams (clip lanes): entries are handed out under a lock,
    // live in a deque (stable addresses) and chain to an explicit event, never to "the previous entry"
    int timing = 0;          // 0 off, 1 one event pair per launch, 2 one per SEGMENT (run of consecutive launches of one kind)
    std::deque<eng::TimedLaunch> timed; size_t timed_used = 0; std::mutex timing_mu;
};

namespace eng {
#pragma GCC visibility push(hidden)

inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

inline Net* get_net(i2v_handle h, int id) {
    if (!h || id < 0 || id >= (int)h->nets.size() || !h->nets[id]) { fail("bad net id %d", id); return nullptr; }
    return h->nets[id];
}

template <typename T>
int upload(Net& n, const std::vector<T>& host, T** dev) {
    size_t bytes = host.size() * sizeof(T);
    void* d = be_malloc(bytes ? bytes : 16);
    if (!d) return fail("device allocation of %zu bytes failed", bytes);
    n.dev_allocs.push_back(d);
    n.weight_bytes += bytes;
    if (bytes) CHECK_BE(be_h2d(d, host.data(), bytes));
    *dev = (T*)d;
    return 0;
}

// i2v_pack.cpp: the operands of a convolution node, uploaded -- forward, input gradient per stride-parity class, image gradient
bool math_bf16x3();
int pack_fwd(Net& n, Node& nd);
int pack_bwd(Net& n, Node& nd);
int pack_img(Net& n, Node& nd);
bool gconv_enabled();               // grouped nodes run on k_gconv in this plan (else: the dense route)
int pack_gconv(Net& n, Node& nd);
bool dwconv_enabled();              // depthwise nodes run on k_dwconv in this plan (else: the dense route)
int pack_dwconv(Net& n, Node& nd);

// i2v_plan.cpp: one pass over the nodes from arena offset `off` for N frames.  Dry: nothing is emitted, *end is where the temporaries
// end.  Real (the arena allocated): fills n.fwd, n.bwd and n.hook_tmp.  False with *err set when the graph cannot be planned.
struct View { float* p; int64_t nstride; int C, H, W; int T = 1; };
View view_of(Net& n, int t, bool grad);
bool plan_pass(Net& n, bool dry, size_t off, size_t N, size_t* end, std::string* err);

// i2v_tune.cpp: what may run fused or on the side stream, and which tile configuration each convolution launch runs -- the first two
// decided from access_of's read and write sets of every launch (`clips`: the planned clip count)
Access access_of(const Launch& l, int64_t clips);
Range conv_dst(const Launch& l, int64_t clips);        // the output of a convolution launch, as access_of lists it
void mark_fusable(Net& n);
void mark_overlap(Net& n);
int autotune(Net& n);
void record_unstored(Net& n);       // Net::unstored from the finished marks and the autotuner's choices

// i2v_run.cpp: one launch (or fused group) of a planned list, as the executor and the autotuner's probes issue it
I2VConvParams conv_prep(const Launch& l, const float* x, float* gx, int accumulate);
int conv_run(const Launch& l, int frames, const float* x, float* gx, int accumulate, i2v_stream_t s);
bool fused_fits(const Launch& a, const Launch& b, int frames);
int fused_run(const Launch& a, const Launch& b, int frames, const float* x, int halo, i2v_stream_t s);
int fast_run(const std::vector<Launch>& L, size_t li, int frames, const float* x, i2v_stream_t s);
bool sc_pair_ok(const Launch& a, const Launch& b);            // the structural rule on the prepped parameters of two launches of one list
bool sc_fits(const Launch& a, const Launch& b, int frames);
int sc_run(const Launch& a, const Launch& b, int frames, i2v_stream_t s);
extern long long g_overlap_launches;        // launches issued on a side stream (mark_overlap): a relaxed counter, diagnostics only

#pragma GCC visibility pop
}  // namespace eng
