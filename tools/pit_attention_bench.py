"""The PiT streaming attention launches (csrc/i2v_pit.hip) on the six stage shapes of pit_s_224 and pit_b_224 at 128 frames, forward and
input gradient, next to three yardsticks:

  * eager PyTorch on the same GPU and tensors: the attention core of tests/pit_reference.py (`attn_core`: q k^T, the scale, softmax,
    product with v) in float32 and its autograd backward to qkv;
  * the composed route of the same library, which is what the planner runs under I2V_PIT_ATTN=0: forward `i2v_xf_gemm_f32`
    (S = scale q k^T, batched over frames and heads) + `i2v_xf_softmax_f32` + `i2v_xf_gemm_f32` (P v), with P kept; backward a gemm
    (dP = dout v^T), `i2v_xf_softmax_bwd_f32` and three gemms (dq = dS k, dk = dS^T q, dv = P^T dout).  Checked to agree with the kernel
    before either is timed;
  * the arithmetic floor of the algorithm's products -- 4 F H T^2 dh flops forward, 10 F H T^2 dh backward -- at the 157.3 TFLOP/s of
    the fp32 MFMA.  The kernel does more: its backward forms S and dP twice (7 products for 5).

    python tools/pit_attention_bench.py [--frames 128] [--reps 30] [--shape s0|s1|s2|b0|b1|b2|all|b2c]   (b2c: the 64-token control of b2, not part of `all`)

Times CALLS: one HIP event pair around each side's calls (the ctypes calls and their launches; outputs are made before), the median of
`reps` warm calls after 5 warm-up calls, with the fastest and slowest call as the spread.  Prints one JSON line per shape."""
import argparse
import ctypes as C
import json

from bench_util import timed
#: label -> (T, H, dh): the three stages of pit_s_224 and of pit_b_224
SHAPES = {"s0": (730, 3, 48), "s1": (197, 6, 48), "s2": (50, 12, 48), "b0": (962, 4, 64), "b1": (257, 8, 64), "b2": (65, 16, 64)}
#: a control for the one shape the kernel loses backward: `pit_b`'s stage 2 with one token fewer, which is exactly one tile of 64
CONTROLS = {"b2c": (64, 16, 64)}
FLOOR_TBS, FLOOR_TFLOPS = 4.7, 157.3


def one(label, Fr, reps):
    import torch
    from i2v_amd import attacks
    from i2v_amd import lib as _lib
    from tests.pit_reference import attn_core
    T, H, dh = {**SHAPES, **CONTROLS}[label]
    eng = attacks.get_engine("cuda:0")
    capi, st = eng.capi, eng.stream()
    P = lambda t: t.data_ptr()      # noqa: E731
    gen = torch.Generator().manual_seed(T * 100 + H)
    Cn, scale = H * dh, dh ** -0.5
    qkv = torch.randn(Fr, T, 3 * Cn, generator=gen).cuda()
    dout = torch.randn(Fr, T, Cn, generator=gen).cuda()
    out, dqkv = torch.empty_like(dout), torch.empty_like(qkv)
    lse, delta = torch.empty(Fr, H, T, device="cuda"), torch.empty(Fr, H, T, device="cuda")

    def fwd():
        _lib.check(capi, capi.i2v_pit_attention_f32(P(qkv), Fr, T, H, dh, scale, P(out), P(lse), st))

    def bwd():
        _lib.check(capi, capi.i2v_pit_attention_bwd_f32(P(qkv), P(out), P(lse), P(dout), Fr, T, H, dh, scale, P(delta), P(dqkv), st))

    # the composed route: batch = frames * heads, outer = frame, inner = head; the score rows are padded to a multiple of 4 floats (ld),
    # which the softmax launches need
    ld = (T + 3) // 4 * 4
    S, dS = torch.zeros(Fr, H, T, ld, device="cuda"), torch.zeros(Fr, H, T, ld, device="cuda")
    out_c, dqkv_c = torch.empty_like(dout), torch.empty_like(qkv)
    rows, qs, os_, ps = Fr * H * T, 3 * Cn * T, T * Cn, T * ld      # rows of S; per-frame strides of qkv and out; per-head stride of S
    k_, v_ = 4 * Cn, 8 * Cn                                         # bytes from q to k and to v inside a qkv row

    def gemm(A, a_bo, a_bi, a_sm, a_sk, B, b_bo, b_sk, b_sn, Cp, c_bo, c_bi, c_sm, M, N, K, alpha=1.0):
        d = _lib.XfGemmDesc(A, a_bo, a_bi, a_sm, a_sk, B, b_bo, dh, b_sk, b_sn, Cp, c_bo, c_bi, c_sm, None, None, None, None, M, N, K, Fr * H, H,
                            alpha, 0)
        _lib.check(capi, capi.i2v_xf_gemm_f32(C.byref(d), st))

    def comp_fwd():
        gemm(P(qkv), qs, dh, 3 * Cn, 1, P(qkv) + k_, qs, 1, 3 * Cn, P(S), H * ps, ps, ld, T, T, dh, scale)         # S = scale q k^T
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
        eager_f = timed(lambda: attn_core(xr, H), reps, 5)
    y = attn_core(xr, H)
    eager_b = timed(lambda: torch.autograd.grad(y, xr, dout, retain_graph=True), reps, 5)
    del y
    row = {"shape": label, "frames": Fr, "T": T, "heads": H, "dh": dh, "composition_agrees_to": agree}
    prod = Fr * H * T * T * dh
    for name, fn, comp, floats, flop, eg in (("forward", fwd, comp_fwd, Fr * (qs + os_ + H * T), 4 * prod, eager_f),
                                             ("input_gradient", bwd, comp_bwd, Fr * (2 * qs + 2 * os_ + 3 * H * T), 10 * prod, eager_b)):
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
    ap.add_argument("--shape", choices=sorted(SHAPES) + sorted(CONTROLS) + ["all"], default="all")
    a = ap.parse_args()
    for label in (SHAPES if a.shape == "all" else [a.shape]):
        one(label, a.frames, a.reps)


if __name__ == "__main__":
    main()
