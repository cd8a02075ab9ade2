"""The Twins sub-sampled attention launches (csrc/i2v_twins.hip) on the four PCPVT and the four SVT-small stage shapes at 128 frames,
forward and input gradient, next to three yardsticks:

  * eager PyTorch on the same GPU and tensors: the GSA core of tests/twins_reference.py (`gsa_core`: q k^T, softmax, product with v) in
    float32 and its autograd backward to q and kv;
  * the same problem composed from the shared launches, which is what the planner would run without the new kernel: forward
    `i2v_xf_gemm_f32` (S = scale q k^T, batched over frames and heads) + `i2v_xf_softmax_f32` + `i2v_xf_gemm_f32` (P v), with P kept;
    backward a gemm (dP = dout v^T), `i2v_xf_softmax_bwd_f32` and three gemms (dq = dS k, dk = dS^T q, dv = P^T dout);
  * the floor: the larger of the byte floor -- q read and out written once, kv read once forward; q, dout, kv read and dq, dkv written
    once backward -- at the measured 4.7 TB/s of DESIGN.md section 4, and the arithmetic floor of the products (2 forward, 5 backward)
    at the 157.3 TFLOP/s of the fp32 MFMA.  The kernel does more: the backward forms S and dP in both of its launches (8 products).

    python tools/twins_attention_bench.py [--frames 128] [--reps 30]          # one child process per shape, stopping at the first failure
    python tools/twins_attention_bench.py --shape pcpvt0 [--frames 128]        # one shape, in this process

Times CALLS: one HIP event pair around each side's calls (the ctypes calls and their launches; outputs are made before), the median of
`reps` warm calls after 5 warm-up calls, with the fastest and slowest call as the spread.  Prints one JSON line per shape."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

from bench_util import timed
#: label -> (Tq, Tk, H, dh): stages 0 .. 3 of the three PCPVT models (head width 64) and of twins_svt_small (head width 32)
SHAPES = {"pcpvt0": (3136, 49, 1, 64), "pcpvt1": (784, 49, 2, 64), "pcpvt2": (196, 49, 5, 64), "pcpvt3": (49, 49, 8, 64),
          "svt0": (3136, 49, 2, 32), "svt1": (784, 49, 4, 32), "svt2": (196, 49, 8, 32), "svt3": (49, 49, 16, 32)}
FLOOR_TBS, FLOOR_TFLOPS = 4.7, 157.3
CHILD_SECONDS = 150


def one(label, Fr, reps):
    import torch
    from i2v_amd import attacks
    from i2v_amd import lib as _lib
    from tests.twins_reference import gsa_core
    Tq, Tk, H, dh = SHAPES[label]
    eng = attacks.get_engine("cuda:0")
    capi, st = eng.capi, eng.stream()
    P = lambda t: t.data_ptr()      # noqa: E731
    gen = torch.Generator().manual_seed(Tq * 100 + H)
    Cn, scale = H * dh, dh ** -0.5
    q, kv = torch.randn(Fr, Tq, Cn, generator=gen).cuda(), torch.randn(Fr, Tk, 2 * Cn, generator=gen).cuda()
    dout = torch.randn(Fr, Tq, Cn, generator=gen).cuda()
    out, dq, dkv = torch.empty_like(q), torch.empty_like(q), torch.empty_like(kv)

    def fwd():
        _lib.check(capi, capi.i2v_twins_attention_f32(P(q), P(kv), Fr, Tq, Tk, H, dh, scale, P(out), st))

    def bwd():
        _lib.check(capi, capi.i2v_twins_attention_bwd_f32(P(q), P(kv), P(dout), Fr, Tq, Tk, H, dh, scale, P(dq), P(dkv), st))

    # the composition from the shared launches: batch = frames * heads, outer = frame, inner = head; the score rows are padded to a
    # multiple of 4 floats (ld), which the softmax launches need
    ld = (Tk + 3) // 4 * 4
    S, dS = torch.zeros(Fr, H, Tq, ld, device="cuda"), torch.zeros(Fr, H, Tq, ld, device="cuda")
    out_c, dq_c, dkv_c = torch.empty_like(q), torch.empty_like(q), torch.empty_like(kv)
    rows = Fr * H * Tq
    tok, key, sq = Tq * Cn, Tk * 2 * Cn, Tq * ld      # per-frame strides of q / out and of kv; per-head stride of S
    v_ = 4 * Cn                                        # bytes from k to v inside a kv row

    def gemm(A, a_bo, a_bi, a_sm, a_sk, B, b_bo, b_sk, b_sn, Cp, c_bo, c_bi, c_sm, M, N, K, alpha=1.0):
        d = _lib.XfGemmDesc(A, a_bo, a_bi, a_sm, a_sk, B, b_bo, dh, b_sk, b_sn, Cp, c_bo, c_bi, c_sm, None, None, None, None, M, N, K, Fr * H, H,
                            alpha, 0)
        _lib.check(capi, capi.i2v_xf_gemm_f32(C.byref(d), st))

    def comp_fwd():
        gemm(P(q), tok, dh, Cn, 1, P(kv), key, 1, 2 * Cn, P(S), H * sq, sq, ld, Tq, Tk, dh, scale)                # S = scale q k^T
        _lib.check(capi, capi.i2v_xf_softmax_f32(P(S), rows, Tk, ld, st))
        gemm(P(S), H * sq, sq, ld, 1, P(kv) + v_, key, 2 * Cn, 1, P(out_c), tok, dh, Cn, Tq, dh, Tk)              # out = P v

    def comp_bwd():
        gemm(P(dout), tok, dh, Cn, 1, P(kv) + v_, key, 1, 2 * Cn, P(dS), H * sq, sq, ld, Tq, Tk, dh)              # dP = dout v^T
        _lib.check(capi, capi.i2v_xf_softmax_bwd_f32(P(dS), P(S), rows, Tk, ld, scale, st))
        gemm(P(dS), H * sq, sq, ld, 1, P(kv), key, 2 * Cn, 1, P(dq_c), tok, dh, Cn, Tq, dh, Tk)                   # dq = dS k
        gemm(P(dS), H * sq, sq, 1, ld, P(q), tok, Cn, 1, P(dkv_c), key, dh, 2 * Cn, Tk, dh, Tq)                   # dk = dS^T q
        gemm(P(S), H * sq, sq, 1, ld, P(dout), tok, Cn, 1, P(dkv_c) + v_, key, dh, 2 * Cn, Tk, dh, Tq)            # dv = P^T dout

    fwd(), bwd(), comp_fwd(), comp_bwd()
    torch.cuda.synchronize()
    rel = lambda a, b: float((a - b).norm() / b.norm())      # noqa: E731
    agree = {"out": rel(out_c, out), "dq": rel(dq_c, dq), "dkv": rel(dkv_c, dkv)}
    assert max(agree.values()) < 1e-5, agree                               # the two sides compute the same thing
    qr, kr = q.clone().requires_grad_(True), kv.clone().requires_grad_(True)
    with torch.no_grad():
        eager_f = timed(lambda: gsa_core(qr, kr, H), reps, 5)
    y = gsa_core(qr, kr, H)
    eager_b = timed(lambda: torch.autograd.grad(y, (qr, kr), dout, retain_graph=True), reps, 5)
    del y
    row = {"shape": label, "frames": Fr, "Tq": Tq, "Tk": Tk, "heads": H, "dh": dh, "composition_agrees_to": agree}
    prod = Fr * H * Tq * Tk * dh
    for name, fn, comp, floats, flop, eg in (("forward", fwd, comp_fwd, Fr * (2 * tok + key), 4 * prod, eager_f),
                                             ("input_gradient", bwd, comp_bwd, Fr * (3 * tok + 2 * key), 10 * prod, eager_b)):
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
    ap.add_argument("--shape", choices=sorted(SHAPES))
    a = ap.parse_args()
    if a.shape:
        return one(a.shape, a.frames, a.reps)
    for label in SHAPES:                                                   # a fresh process per shape; a failure ends the run
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--shape", label, "--frames", str(a.frames), "--reps", str(a.reps)],
                               timeout=CHILD_SECONDS)
        except subprocess.TimeoutExpired:
            sys.exit(f"{label}: no result within {CHILD_SECONDS} s; stopping")
        if r.returncode != 0:
            sys.exit(f"{label}: exit status {r.returncode}; stopping")


if __name__ == "__main__":
    main()
