/* libi2v_hip.so -- the launches of the I3D non-local block's core (csrc/i2v_kernels.hip: the three product forms between frame-major
 * activation views and a dense per-clip matrix with their K-split, the row softmax and its backward) and the gated add that sits next
 * to them in a net's launch list, reachable on their own with arbitrary descriptors: tests and tools.  No planner calls these entries
 * and they change no launch.
 *
 * Same conventions as i2v_hip.h: every function returns 0 on success and non-zero on error with the text in `i2v_last_error()`; tensors
 * are caller-owned fp32 pointers of the library's memory space (device pointers in libi2v_hip.so, host pointers in the host
 * simulation); work is enqueued on `stream` (a hipStream_t as void*, 0 = default) and nothing synchronises the host.
 */
#ifndef I2V_NL_LAUNCH_H
#define I2V_NL_LAUNCH_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* A channel-major operand over a frame-major activation view: element (clip b, channel c, position i), i < T * HW, lives at
 *   p + (b * T + i / HW) * nstride + c * HW + i % HW          (nstride: floats between frames, >= channels * HW) */
typedef struct { const float* p; int64_t nstride; int32_t T, HW; } i2v_nl_act;

/* One product per clip, every output element one k-ordered fmaf chain:
 *   form 1  D[i][j] = scale * sum_c A[c][i] * B[c][j]     D dense [clips][M][N];  M = A.T * A.HW, N = B.T * B.HW
 *   form 2  C[c][i] = sum_j A[c][j] * Din[i][j]           C an activation view of c_T * c_HW = M positions;  N = A.T * A.HW
 *   form 3  C[c][j] = sum_i A[c][i] * Din[i][j]           C an activation view of c_T * c_HW = N positions;  M = A.T * A.HW
 * Cc channels.  Forms 2 / 3: `accumulate` adds to C instead of writing it; ksplit > 1 cuts the reduction into ksplit segments of
 * ceil(ceil(K / ksplit) / 32) * 32 rows whose sums go to part[clips][ksplit][Cc][columns] and are added in segment order (form 1
 * ignores it).  Operands are read 16 bytes at a time where their base is 16-byte aligned and HW and nstride (Din: N) are multiples of
 * 4, element by element otherwise -- the launch decides, the caller need not.
 * No rows, no columns or clips <= 0: nothing to do, 0.  Refused: a null descriptor, a form outside 1..3, a null operand the form
 * reads or writes, T <= 0 or HW <= 0 of a view the form uses, a count that is not its view's T * HW, form 1 without channels,
 * ksplit > 1 without part. */
typedef struct {
    int32_t form, clips, Cc, M, N;
    i2v_nl_act A, B;                                      /* B: form 1 only */
    float* C; int64_t c_nstride; int32_t c_T, c_HW;       /* forms 2 / 3: the output view */
    float* D; const float* Din;                           /* the dense matrix: output of form 1 / input of forms 2, 3 */
    float scale; int32_t accumulate;
    int32_t ksplit; float* part;
} i2v_nl_gemm_desc;

int i2v_nl_gemm_f32(const i2v_nl_gemm_desc* desc, void* stream);

/* Row softmax over `rows` dense rows of N floats, in place: mode 0  X = softmax(X);  mode 1  X = P o (X - rowsum(X o P)), the
 * backward over dP with the probabilities P.  rows <= 0: nothing to do, 0.  Refused: X null, a mode outside 0 / 1, mode 1 without P,
 * N <= 0. */
int i2v_nl_softmax_rows_f32(float* X, const float* P, int64_t rows, int N, int mode, void* stream);

/* out = gain' * gate(((0 + a[0]) + a[1]) + a[2]) over N frames of C channels of HW elements; operand x's element (n, c, i) lives at
 * x + n * x_nstride + c * HW + i.  Null addends are left out.  gate (1-bit rows, one per channel, gate_stride 32-bit words each:
 * bit n * HW + i) or else mask (a float view: kept where mask > 0) zeroes the sum; neither: no gating.  gain != 0 multiplies the
 * result.  N <= 0: nothing to do, 0.  Refused: a null descriptor, out null, C <= 0 or HW <= 0, gate rows shorter than N * HW bits. */
typedef struct {
    float* out; int64_t out_nstride;
    const float* a[3]; int64_t a_nstride[3];
    const float* mask; int64_t mask_nstride;
    const uint32_t* gate; int32_t gate_stride;
    int32_t N, C, HW;
    float gain;
} i2v_nl_addmask_desc;

int i2v_nl_addmask_f32(const i2v_nl_addmask_desc* desc, void* stream);

#ifdef __cplusplus
}
#endif
#endif
