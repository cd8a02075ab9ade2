"""The XCiT cross-covariance attention launches (csrc/i2v_xcit.hip) on the four model shapes at 128 frames, forward and input gradient,
next to two yardsticks:

  * eager PyTorch on the same GPU and tensors: the XCA core of tests/xcit_reference.py (`xca_core`: normalise q and k over the tokens,
    the dh x dh product, softmax, product with v) in float32 and its autograd backward to qkv;
  * the byte floor: q, k and v read once and out written once forward (4 F T C floats), qkv and dout read once and dqkv written once
    backward (7 F T C floats), at the measured 4.7 TB/s of DESIGN.md section 4.  The kernel reads more: dout twice and q, k, v once each
    backward.

    python tools/xcit_attention_bench.py [--frames 128] [--reps 20]          # one child process per shape, stopping at the first failure
    python tools/xcit_attention_bench.py --shape small [--frames 128]         # one shape, in this process

Times CALLS: one HIP event pair around each C entry (the ctypes call and its launch; outputs are made before), the median of `reps` warm
calls after 3 warm-up calls.  Prints one JSON line per shape."""
import argparse
import json
import os
import subprocess
import sys

from bench_util import timed
#: label -> (T, H, dh): tiny (nano has dh 32), small, medium, large
SHAPES = {"tiny": (196, 4, 48), "small": (196, 8, 48), "medium": (196, 8, 64), "large": (196, 16, 48)}
FLOOR_TBS = 4.7
CHILD_SECONDS = 120


def one(label, Fr, reps):
    import torch
    from i2v_amd import attacks
    from i2v_amd import lib as _lib
    from tests.xcit_reference import xca_core
    T, H, dh = SHAPES[label]
    eng = attacks.get_engine("cuda:0")
    capi, st = eng.capi, eng.stream()
    P = lambda t: t.data_ptr()      # noqa: E731
    gen = torch.Generator().manual_seed(T * 100 + H)
    C = H * dh
    qkv, dout = torch.randn(Fr, T, 3 * C, generator=gen).cuda(), torch.randn(Fr, T, C, generator=gen).cuda()
    temp = (0.5 + 3.5 * torch.rand(H, generator=gen)).cuda()
    gram, probs = torch.zeros(Fr, H, dh + 2, dh, device="cuda"), torch.zeros(Fr, H, dh, dh, device="cuda")
    out, dqkv = torch.empty_like(dout), torch.empty_like(qkv)

    def fwd():
        _lib.check(capi, capi.i2v_xcit_attention_f32(P(qkv), Fr, T, H, dh, P(temp), P(gram), P(probs), P(out), st))

    def bwd():
        _lib.check(capi, capi.i2v_xcit_attention_bwd_f32(P(qkv), P(gram), P(probs), P(dout), Fr, T, H, dh, P(temp), P(dqkv), st))
    qr = qkv.clone().requires_grad_(True)
    with torch.no_grad():
        eager_f = timed(lambda: xca_core(qr, H, temp), reps, 3)[0]
    y, _ = xca_core(qr, H, temp)
    eager_b = timed(lambda: torch.autograd.grad(y, qr, dout, retain_graph=True), reps, 3)[0]
    del y
    row = {"shape": label, "frames": Fr, "T": T, "heads": H, "dh": dh, "workgroups": Fr * H}
    for name, fn, floats, flop, eg in (("forward", fwd, 4 * Fr * T * C, 4 * Fr * H * T * dh * dh, eager_f),
                                       ("input_gradient", bwd, 7 * Fr * T * C, 8 * Fr * H * T * dh * dh, eager_b)):
        ms = timed(fn, reps, 3)[0]
        floor = floats * 4 / (FLOOR_TBS * 1e12) * 1e3
        row[name] = {"call_ms": round(ms, 4), "byte_floor_ms": round(floor, 4), "share_of_byte_floor": round(floor / ms, 3),
                     "algorithmic_TB/s": round(floats * 4 / ms / 1e9, 3), "mfma_TFLOP/s": round(flop / ms / 1e9, 2), "eager_ms": round(eg, 4),
                     "eager_over_kernel": round(eg / ms, 2)}
    print(json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=128)
    ap.add_argument("--reps", type=int, default=20)
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
