"""The ConViT gated positional attention launches (csrc/i2v_convit.hip) on the three model shapes at 128 frames, forward and input
gradient, next to four yardsticks:

  * eager PyTorch on the same GPU and tensors: the GPSA core of tests/convit_reference.py (`blend_attention`: softmax, blend with the
    precomputed table, product with v) in float32 and its autograd backward to qkv;
  * `i2v_vit_attention_f32` / `_bwd_f32` on the same qkv: plain multi-head attention on the shared GEMM and softmax launches -- the price
    of the blend (and of the fused tile) over plain attention;
  * the kernel's own `table = null` mode: the same launch without the blend;
  * the arithmetic floor of the fp32 MFMA products -- 4 F H T^2 dh FLOP forward (q k^T, P v), 8 F H T^2 dh backward (dout v^T, dS k,
    dS^T q, P^T dout) -- at the 157.3 TFLOP/s fp32 MFMA peak.

    python tools/convit_attention_bench.py [--frames 128] [--reps 20]

Times CALLS: one HIP event pair around each C entry (the ctypes call and its launches; outputs and scratch are made before), the median
of `reps` warm calls after 3 warm-up calls.  Prints one JSON line per shape."""
import argparse
import json

from bench_util import timed
#: name -> (T, H, dh)
SHAPES = (("convit_tiny", 196, 4, 48), ("convit_small", 196, 9, 48), ("convit_base", 196, 16, 48))
PEAK_TFLOPS = 157.3


def main():
    import torch
    from i2v_amd import attacks
    from i2v_amd import lib as _lib
    from tests.convit_reference import blend_attention
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=128)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    eng = attacks.get_engine("cuda:0")
    capi, st = eng.capi, eng.stream()
    P = lambda t: None if t is None else t.data_ptr()      # noqa: E731
    Fr = a.frames
    for name, T, H, dh in SHAPES:
        gen = torch.Generator().manual_seed(T * 100 + H)
        R = lambda *shape: torch.randn(*shape, generator=gen).cuda()      # noqa: E731
        C, ld, scale = H * dh, (T + 3) // 4 * 4, dh ** -0.5
        qkv, dout = R(Fr, T, 3 * C), R(Fr, T, C)
        c = (0.1 + 0.8 * torch.rand(H, generator=gen)).cuda()
        table = (torch.rand(H, T, ld, generator=gen) * (2.0 / T)).cuda()
        probs, ds = (torch.zeros(Fr, H, T, ld, device="cuda") for _ in range(2))
        out, dqkv = torch.empty_like(dout), torch.empty_like(qkv)
        flop_f, flop_b = 4 * Fr * H * T * T * dh, 8 * Fr * H * T * T * dh

        def fwd(cc=c, tt=table):
            _lib.check(capi, capi.i2v_convit_attention_f32(P(qkv), Fr, T, H, dh, scale, P(cc), P(tt), P(probs), P(out), st))

        def bwd(cc=c, tt=table):
            _lib.check(capi, capi.i2v_convit_attention_bwd_f32(P(qkv), P(probs), P(dout), Fr, T, H, dh, scale, P(cc), P(tt), P(ds), P(dqkv), st))

        def vit_fwd():
            _lib.check(capi, capi.i2v_vit_attention_f32(P(qkv), Fr, T, H, dh, scale, P(probs), P(out), st))

        def vit_bwd():
            _lib.check(capi, capi.i2v_vit_attention_bwd_f32(P(qkv), P(probs), P(dout), Fr, T, H, dh, scale, P(ds), P(dqkv), st))
        qr = qkv.clone().requires_grad_(True)
        tab = table[:, :, :T].contiguous()
        with torch.no_grad():
            eager_f = timed(lambda: blend_attention(qr, H, scale, c, tab), a.reps, 3)[0]
        y, _ = blend_attention(qr, H, scale, c, tab)
        eager_b = timed(lambda: torch.autograd.grad(y, qr, dout, retain_graph=True), a.reps, 3)[0]
        del y
        vit_f = timed(vit_fwd, a.reps, 3)[0]
        vit_b = timed(vit_bwd, a.reps, 3)[0]
        null_f = timed(lambda: fwd(None, None), a.reps, 3)[0]
        null_b = timed(lambda: bwd(None, None), a.reps, 3)[0]
        row = {"name": name, "frames": Fr, "T": T, "heads": H, "dh": dh, "lds_bytes": 16 * ((T + 15) // 16 * 16 + 4) * 4,
               "workgroups": Fr * H * -(-T // 16)}
        for label, fn, flop, eg, vt, nl in (("forward", fwd, flop_f, eager_f, vit_f, null_f), ("input_gradient", bwd, flop_b, eager_b, vit_b, null_b)):
            ms = timed(fn, a.reps, 3)[0]
            row[label] = {"call_ms": round(ms, 4), "mfma_TFLOP/s": round(flop / ms / 1e9, 2), "flop_floor_ms": round(flop / PEAK_TFLOPS / 1e9, 4),
                          "share_of_flop_floor": round(flop / PEAK_TFLOPS / 1e9 / ms, 3), "eager_ms": round(eg, 4),
                          "eager_over_kernel": round(eg / ms, 2), "vit_attention_ms": round(vt, 4), "kernel_over_vit_attention": round(ms / vt, 2),
                          "table_null_ms": round(nl, 4), "kernel_over_table_null": round(ms / nl, 2)}
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
