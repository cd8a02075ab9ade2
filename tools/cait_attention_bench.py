"""The CaiT talking-heads attention launches (csrc/i2v_cait.hip) on the two full-size shapes at 128 frames, forward and input gradient,
next to three yardsticks:

  * eager PyTorch on the same GPU and tensors: the `TalkingHeadAttn` core of tests/cait_reference.py in float32 and its autograd
    backward to qkv;
  * `i2v_vit_attention_f32` / `_bwd_f32` on the same (F, T, H, dh): plain multi-head attention on the shared GEMM and softmax launches,
    which shows what the two head mixes (and the fused tile) cost;
  * the arithmetic floor of the fp32 MFMA products -- 4 F H T^2 dh FLOP forward (q k^T, P' v), 8 F H T^2 dh backward (dout v^T, dS k,
    dS^T q, P'^T dout) -- at the 157.3 TFLOP/s fp32 MFMA peak.  The head mixes (4 F T^2 H^2 FLOP forward, 6 backward) run on the vector
    ALUs and are not in that floor.

    python tools/cait_attention_bench.py [--frames 128] [--reps 20]

Times CALLS: one HIP event pair around each C entry (the ctypes call and its launches; outputs and scratch are made before), the median
of `reps` warm calls after 3 warm-up calls.  Prints one JSON line per shape."""
import argparse
import json

from bench_util import timed
#: name -> (T, H, dh)
SHAPES = (("cait_xxs24_224 / cait_xxs36_224", 196, 4, 48), ("cait_s24_224", 196, 8, 48))
PEAK_TFLOPS = 157.3


def main():
    import torch
    from i2v_amd import attacks
    from i2v_amd import lib as _lib
    from tests.cait_reference import talking_heads
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=128)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    eng = attacks.get_engine("cuda:0")
    capi, st = eng.capi, eng.stream()
    P = lambda t: t.data_ptr()      # noqa: E731
    Fr = a.frames
    for name, T, H, dh in SHAPES:
        gen = torch.Generator().manual_seed(T * 100 + H)
        R = lambda *shape: torch.randn(*shape, generator=gen).cuda()      # noqa: E731
        C, ld, scale = H * dh, (T + 3) // 4 * 4, dh ** -0.5
        qkv, dout = R(Fr, T, 3 * C), R(Fr, T, C)
        wl, bl, ww, bw = (torch.eye(H) + 0.25 * torch.randn(H, H, generator=gen)).cuda(), 0.5 * R(H), (torch.eye(H) + 0.25 * torch.randn(H, H, generator=gen)).cuda(), 0.02 * R(H)
        probs, ds, pm = (torch.zeros(Fr, H, T, ld, device="cuda") for _ in range(3))
        out, dqkv = torch.empty_like(dout), torch.empty_like(qkv)
        flop_f, flop_b = 4 * Fr * H * T * T * dh, 8 * Fr * H * T * T * dh

        def fwd():
            _lib.check(capi, capi.i2v_cait_attention_f32(P(qkv), Fr, T, H, dh, scale, P(wl), P(bl), P(ww), P(bw), P(probs), P(out), st))

        def bwd():
            _lib.check(capi, capi.i2v_cait_attention_bwd_f32(P(qkv), P(probs), P(dout), Fr, T, H, dh, scale, P(wl), P(ww), P(bw), P(ds), P(pm),
                                                             P(dqkv), st))

        def vit_fwd():
            _lib.check(capi, capi.i2v_vit_attention_f32(P(qkv), Fr, T, H, dh, scale, P(probs), P(out), st))

        def vit_bwd():
            _lib.check(capi, capi.i2v_vit_attention_bwd_f32(P(qkv), P(probs), P(dout), Fr, T, H, dh, scale, P(ds), P(dqkv), st))
        qr = qkv.clone().requires_grad_(True)
        with torch.no_grad():
            eager_f = timed(lambda: talking_heads(qr, H, scale, wl, bl, ww, bw), a.reps, 3)[0]
        y, _ = talking_heads(qr, H, scale, wl, bl, ww, bw)
        eager_b = timed(lambda: torch.autograd.grad(y, qr, dout, retain_graph=True), a.reps, 3)[0]
        del y
        vit_f = timed(vit_fwd, a.reps, 3)[0]
        vit_b = timed(vit_bwd, a.reps, 3)[0]
        row = {"name": name, "frames": Fr, "T": T, "heads": H, "dh": dh, "lds_bytes": H * 16 * ((T + 15) // 16 * 16 + 4) * 4,
               "workgroups": Fr * -(-T // 16)}
        for label, fn, flop, eg, vt in (("forward", fwd, flop_f, eager_f, vit_f), ("input_gradient", bwd, flop_b, eager_b, vit_b)):
            ms = timed(fn, a.reps, 3)[0]
            row[label] = {"call_ms": round(ms, 4), "mfma_TFLOP/s": round(flop / ms / 1e9, 2), "flop_floor_ms": round(flop / PEAK_TFLOPS / 1e9, 4),
                          "share_of_flop_floor": round(flop / PEAK_TFLOPS / 1e9 / ms, 3), "eager_ms": round(eg, 4),
                          "eager_over_kernel": round(eg / ms, 2), "vit_attention_ms": round(vt, 4), "kernel_over_vit_attention": round(ms / vt, 2)}
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
