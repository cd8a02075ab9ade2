"""The BEiT biased global attention launches (csrc/i2v_beit.hip) on the base shape -- 128 frames, 197 tokens, 12 heads of width 64 --
forward and input gradient, next to three yardsticks:

  * eager PyTorch on the same GPU and tensors: the attention core of tests/beit_reference.py (`attn_core`: q scaled, q k^T, the bias
    added, softmax, product with v) in float32 and its autograd backward to qkv;
  * the composed route of the same library, which is what the planner runs under I2V_BEIT_ATTN=0: forward `i2v_xf_gemm_f32`
    (S = scale q k^T, batched over frames and heads) + `i2v_beit_bias_add_f32` + `i2v_xf_softmax_f32` + `i2v_xf_gemm_f32` (P v), with P
    kept; backward a gemm (dP = dout v^T), `i2v_xf_softmax_bwd_f32` and three gemms (dq = dS k, dk = dS^T q, dv = P^T dout);
  * the floor: the larger of the byte floor -- qkv read and out written once forward; qkv and dout read and dqkv written once backward,
    the bias once per call -- at the measured 4.7 TB/s of DESIGN.md section 4, and the arithmetic floor of the products (2 forward, 5
    backward) at the 157.3 TFLOP/s of the fp32 MFMA.  The kernel does more: the backward forms S and dP three times (12 products).

    python tools/beit_attention_bench.py [--frames 128] [--reps 30] [--shape base|large]

Times CALLS: one HIP event pair around each side's calls (the ctypes calls and their launches; outputs are made before), the median of
`reps` warm calls after 5 warm-up calls, with the fastest and slowest call as the spread.  Prints one JSON line."""
import argparse
import ctypes as C
import json

from bench_util import timed
#: label -> (T, H, dh)
SHAPES = {"base": (197, 12, 64), "large": (197, 16, 64)}
FLOOR_TBS, FLOOR_TFLOPS = 4.7, 157.3


def one(label, Fr, reps):
    import torch
    from i2v_amd import attacks
    from i2v_amd import lib as _lib
    from tests.beit_reference import attn_core
    T, H, dh = SHAPES[label]
    eng = attacks.get_engine("cuda:0")
    capi, st = eng.capi, eng.stream()
    P = lambda t: t.data_ptr()      # noqa: E731
    gen = torch.Generator().manual_seed(T * 100 + H)
    Cn, scale = H * dh, dh ** -0.5
    qkv, bias = torch.randn(Fr, T, 3 * Cn, generator=gen).cuda(), torch.randn(H, T, T, generator=gen).cuda()
    dout = torch.randn(Fr, T, Cn, generator=gen).cuda()
    out, dqkv = torch.empty_like(dout), torch.empty_like(qkv)

    def fwd():
        _lib.check(capi, capi.i2v_beit_attention_f32(P(qkv), P(bias), Fr, T, H, dh, scale, P(out), st))

    def bwd():
        _lib.check(capi, capi.i2v_beit_attention_bwd_f32(P(qkv), P(bias), P(dout), Fr, T, H, dh, scale, P(dqkv), st))

    # the composed route: batch = frames * heads, outer = frame, inner = head; the score rows and the bias are padded to a multiple of 4
    # floats (ld), which the softmax launches need
    ld = (T + 3) // 4 * 4
    S, dS = torch.zeros(Fr, H, T, ld, device="cuda"), torch.zeros(Fr, H, T, ld, device="cuda")
    biasp = torch.zeros(H, T, ld, device="cuda")
    biasp[:, :, :T] = bias
    out_c, dqkv_c = torch.empty_like(dout), torch.empty_like(qkv)
    rows, qs, os_, ps = Fr * H * T, 3 * Cn * T, T * Cn, T * ld      # rows of S; per-frame strides of qkv and out; per-head stride of S
    k_, v_ = 4 * Cn, 8 * Cn                                         # bytes from q to k and to v inside a qkv row

    def gemm(A, a_bo, a_bi, a_sm, a_sk, B, b_bo, b_sk, b_sn, Cp, c_bo, c_bi, c_sm, M, N, K, alpha=1.0):
        d = _lib.XfGemmDesc(A, a_bo, a_bi, a_sm, a_sk, B, b_bo, dh, b_sk, b_sn, Cp, c_bo, c_bi, c_sm, None, None, None, None, M, N, K, Fr * H, H,
                            alpha, 0)
        _lib.check(capi, capi.i2v_xf_gemm_f32(C.byref(d), st))

    def comp_fwd():
        gemm(P(qkv), qs, dh, 3 * Cn, 1, P(qkv) + k_, qs, 1, 3 * Cn, P(S), H * ps, ps, ld, T, T, dh, scale)         # S = scale q k^T
        _lib.check(capi, capi.i2v_beit_bias_add_f32(P(S), P(biasp), Fr, H * ps, st))
        _lib.check(capi, capi.i2v_xf_softmax_f32(P(S), rows, T, ld, st))
        gemm(P(S), H * ps, ps, ld, 1, P(qkv) + v_, qs, 3 * Cn, 1, P(out_c), os_, dh, Cn, T, dh, T)                 # out = P v

    def comp_bwd():
        gemm(P(dout), os_, dh, Cn, 1, P(qkv) + v_, qs, 1, 3 * Cn, P(dS), H * ps, ps, ld, T, T, dh)                 # dP = dout v^T
        _lib.check(capi, capi.i2v_xf_softmax_bwd_f32(P(dS), P(S), rows, T, ld, scale, st))
        gemm(P(dS), H * ps, ps, ld, 1, P(qkv) + k_, qs, 3 * Cn, 1, P(dqkv_c), qs, dh, 3 * Cn, T, dh, T)            # dq = dS k
        gemm(P(dS), H * ps, ps, 1, ld, P(qkv), qs, 3 * Cn, 1, P(dqkv_c) + k_, qs, dh, 3 * Cn, T, dh, T)            # dk = dS^T q
        gemm(P(S), H * ps, ps, 1, ld, P(dout), os_, Cn, 1, P(dqkv_c) + v_, qs, dh, 3 * Cn, T, dh, T)               # dv = P^T dout

    fwd(), bwd(), comp_fwd(), comp_bwd()
    torch.cuda.synchronize()
    rel = lambda a, b: float((a - b).norm() / b.norm())      # noqa: E731
    agree = {"out": rel(out_c, out), "dqkv": rel(dqkv_c, dqkv)}
    assert max(agree.values()) < 1e-5, agree                               # the two sides compute the same thing
    xr = qkv.clone().requires_grad_(True)
    with torch.no_grad():
        eager_f = timed(lambda: attn_core(xr, bias, H), reps, 5)
    y = attn_core(xr, bias, H)
    eager_b = timed(lambda: torch.autograd.grad(y, xr, dout, retain_graph=True), reps, 5)
    del y
    row = {"shape": label, "frames": Fr, "T": T, "heads": H, "dh": dh, "composition_agrees_to": agree}
    prod = Fr * H * T * T * dh
    for name, fn, comp, floats, flop, eg in (("forward", fwd, comp_fwd, Fr * (qs + os_) + H * T * T, 4 * prod, eager_f),
                                             ("input_gradient", bwd, comp_bwd, Fr * (2 * qs + os_) + H * T * T, 10 * prod, eager_b)):
        ms, lo, hi = timed(fn, reps, 5)
        cms, clo, chi = timed(comp, reps, 5)
        bfl, afl = floats * 4 / (FLOOR_TBS * 1e12) * 1e3, flop / (FLOOR_TFLOPS * 1e12) * 1e3
        row[name] = {"call_ms": round(ms, 4), "fastest_slowest_ms": [round(lo, 4), round(hi, 4)], "byte_floor_ms": round(bfl, 4),
                     "arithmetic_floor_ms": round(afl, 4), "bound_by": "bytes" if bfl >= afl else "arithmetic",
                     "share_of_floor": round(max(bfl, afl) / ms, 3), "mfma_TFLOP/s": round(flop / ms / 1e9, 2),
                     "composed_ms": round(cms, 4), "composed_fastest_slowest_ms": [round(clo, 4), round(chi, 4)],
                     "composed_over_kernel": round(cms / ms, 2), "eager_ms": round(eg[0], 4), "eager_over_kernel": round(eg[0] / ms, 2)}
    print(json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=128)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--shape", choices=sorted(SHAPES), default="base")
    a = ap.parse_args()
    one(a.shape, a.frames, a.reps)


if __name__ == "__main__":
    main()
