// Depthwise 7 x 7 convolution (pad 3, stride 1) on token-major tensors for gfx950 -- the first layer of a ConvNeXt block, timm's
// `nn.Conv2d(C, C, 7, padding=3, groups=C)`, on the (frame, row, column, channel) layout the transformer stack keeps its streams in --
// forward and input gradient, ONE launch per block and pass (I2VCnDwParams, i2v_params.h).
//
// The layer moves 8 bytes per output element for 98 flops: it is bound by memory.  Channels are contiguous, so lanes run over channels:
//   * a lane owns `vec` channels (4 where C % 4 == 0 and the arrays are 16-byte aligned: every access is a 16-byte one; else 1) of a RUN
//     of I2V_CNDW_RUN = 8 consecutive output positions of one row; consecutive lanes own consecutive channel groups, then the next run,
//     then the next row: every load and store of a wave is a set of contiguous 16 C-byte pieces;
//   * the lane keeps its 8 accumulators in registers and walks the 7 filter rows: per filter row it loads that row's 7 weights (a
//     coalesced row of the [49][C] filter each) and the 8 + 6 source values under the run, then slides the 7-wide window over them in
//     registers.  That is 7 x 14 source loads for 8 outputs, 12.25 per output where the naive form loads 49, and every output still
//     is one chain in row-major tap order, because the accumulators persist across the filter rows;
//   * a position outside the plane is a zero operand, not a skipped tap: planes smaller than the filter need nothing special.
// No LDS, no atomics, no read-modify-write; every store is a vector store of a value this lane alone owns.
// Arithmetic: acc = fma(w[a][b], x[h + a - 3][w + b - 3], acc) from 0.f over a = 0 .. 6 outer, b = 0 .. 6 inner, then + b[c], then
// + add (-ffp-contract=off: every fma is written, nothing else is contracted).  The order depends on neither the frame count, the block
// size nor the run; i2v_convnext_host.h performs the same operations in the same order.
// The input gradient is the same kernel on the mirrored filter with the output's gradient as source (stride 1: no parity classes).
#include "i2v_be.h"

long long g_stat_cndw = 0;

typedef float cn_f4 __attribute__((ext_vector_type(4)));

template <int V> struct CnT;
template <> struct CnT<1> {
    typedef float T;
    static __device__ __forceinline__ T zero() { return 0.f; }
    static __device__ __forceinline__ T fma(T w, T x, T a) { return __builtin_fmaf(w, x, a); }
};
template <> struct CnT<4> {
    typedef cn_f4 T;
    static __device__ __forceinline__ T zero() { return cn_f4{0.f, 0.f, 0.f, 0.f}; }
    static __device__ __forceinline__ T fma(T w, T x, T a) {
        return cn_f4{__builtin_fmaf(w.x, x.x, a.x), __builtin_fmaf(w.y, x.y, a.y), __builtin_fmaf(w.z, x.z, a.z), __builtin_fmaf(w.w, x.w, a.w)};
    }
};

template <int V>
__global__ void __launch_bounds__(256) convnext_dw_kernel(const I2VCnDwParams p) {
    typedef typename CnT<V>::T T;
    constexpr int R = I2V_CNDW_RUN;
    const unsigned e = blockIdx.x * 256u + threadIdx.x;
    if (e >= (unsigned)p.H * (unsigned)p.runs * (unsigned)p.lanes) return;
    const unsigned t = fastdiv(e, p.dv_l_m, p.dv_l_s);
    const int c0 = (int)(e - t * (unsigned)p.lanes) * V;
    const int h = (int)fastdiv(t, p.dv_r_m, p.dv_r_s);
    const int w0 = (int)(t - (unsigned)h * (unsigned)p.runs) * R;
    const int n = blockIdx.y, H = p.H, W = p.W, C = p.C;
    const float* xn = p.x + (int64_t)n * H * W * C + c0;
    const float* wc = p.w + c0;
    T acc[R];
#pragma unroll
    for (int j = 0; j < R; ++j) acc[j] = CnT<V>::zero();
#pragma unroll 1      // (one filter row's weights and window live at a time: unrolled, the scheduler hoists all seven rows' loads and spills)
    for (int a = 0; a < 7; ++a) {
        const int hs = h + a - 3;
        const bool rowok = hs >= 0 && hs < H;
        T wr[7], win[R + 6];
#pragma unroll
        for (int b = 0; b < 7; ++b) wr[b] = *(const T*)(wc + (a * 7 + b) * C);
        const float* row = xn + (int64_t)(rowok ? hs : 0) * W * C;
#pragma unroll
        for (int j = 0; j < R + 6; ++j) {
            const int ws = w0 + j - 3;
            win[j] = CnT<V>::zero();
            if (rowok && ws >= 0 && ws < W) win[j] = *(const T*)(row + (int64_t)ws * C);
        }
#pragma unroll
        for (int j = 0; j < R; ++j)
#pragma unroll
            for (int b = 0; b < 7; ++b) acc[j] = CnT<V>::fma(wr[b], win[j + b], acc[j]);
    }
    const int64_t o0 = (((int64_t)n * H + h) * W + w0) * C + c0;
    T bias = CnT<V>::zero();
    if (p.b) bias = *(const T*)(p.b + c0);
#pragma unroll
    for (int j = 0; j < R; ++j) {
        if (w0 + j < W) {
            T v = acc[j];
            if (p.b) v = v + bias;
            if (p.add) v = v + *(const T*)(p.add + o0 + (int64_t)j * C);
            *(T*)(p.y + o0 + (int64_t)j * C) = v;
        }
    }
}

static bool cndw_al16(const void* q) { return ((uintptr_t)q & 15) == 0; }
static int cndw_vec(const I2VCnDwParams& p) {
    return p.C % 4 == 0 && cndw_al16(p.x) && cndw_al16(p.w) && cndw_al16(p.y) && (!p.b || cndw_al16(p.b)) && (!p.add || cndw_al16(p.add)) ? 4 : 1;
}

int k_convnext_dw_plan(I2VCnDwParams* p) {
    if (!p->x || !p->w || !p->y || p->H < 1 || p->W < 1 || p->C < 1) return 1;
    p->runs = (p->W + I2V_CNDW_RUN - 1) / I2V_CNDW_RUN;
    p->vec = cndw_vec(*p);
    p->lanes = p->C / p->vec;
    if ((int64_t)p->H * p->runs * p->lanes >= (1ll << 31)) return 1;
    fastdiv_magic((unsigned)p->lanes, &p->dv_l_m, &p->dv_l_s);
    fastdiv_magic((unsigned)p->runs, &p->dv_r_m, &p->dv_r_s);
    return 0;
}

int k_convnext_dw(const I2VCnDwParams& p, i2v_stream_t st) {
    hipStream_t s = (hipStream_t)st;
    I2VCnDwParams q = p;
    if (k_convnext_dw_plan(&q) != 0 || q.runs != p.runs || q.vec != p.vec || q.lanes != p.lanes || q.dv_l_m != p.dv_l_m || q.dv_l_s != p.dv_l_s ||
        q.dv_r_m != p.dv_r_m || q.dv_r_s != p.dv_r_s)
        return hip_fail(hipErrorInvalidValue, "k_convnext_dw: launch not planned (k_convnext_dw_plan)");
    if (p.N < 0) return hip_fail(hipErrorInvalidValue, "k_convnext_dw: negative frame count");
    if (p.N == 0) return 0;
    if ((int64_t)p.N * p.H * p.W * p.C >= (1ll << 31)) return hip_fail(hipErrorInvalidValue, "k_convnext_dw: more than 2^31 elements");
    const int64_t items = (int64_t)p.H * p.runs * p.lanes;
    const dim3 grid((unsigned)((items + 255) / 256), (unsigned)p.N);
    if (grid.x > 65535u || grid.y > 65535u) return hip_fail(hipErrorInvalidValue, "k_convnext_dw: a grid dimension over 65535");
    __atomic_fetch_add(&g_stat_cndw, 1, __ATOMIC_RELAXED);
    if (p.vec == 4) hipLaunchKernelGGL((convnext_dw_kernel<4>), grid, dim3(256), 0, s, p);
    else hipLaunchKernelGGL((convnext_dw_kernel<1>), grid, dim3(256), 0, s, p);
    LAUNCH_CHECK("convnext_dw_kernel");
    return 0;
}
