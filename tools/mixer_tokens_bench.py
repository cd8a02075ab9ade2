"""The MLP-Mixer / ResMLP token-mixing launch (csrc/i2v_mixer.hip) on the token shapes of the served names at 128 frames, forward and
input gradient, next to two yardsticks:

  * eager PyTorch on the same token-major tensors: `W2 @ gelu(W1 @ z + b1[:, None]) + b2[:, None] + r` (for ResMLP the one product
    with its three per-channel arrays) and its autograd backward to z;
  * the arithmetic floor -- 4 F C S Sh FLOP forward (2 F C S S without a hidden layer), the three products 6 F C S Sh backward (one,
    2 F C S S) at the 157.3 TFLOP/s fp32 MFMA peak -- beside the byte floor (read the tile, write it; the backward reads z and g) at
    4.7 to 5.0 TB/s.

    python tools/mixer_tokens_bench.py [--frames 128] [--reps 20] [--tiles 0,32,64]

Times CALLS: one HIP event pair around each C entry (the ctypes call and the launch; outputs and transposed weights are made before),
the median of `reps` calls after 3 warm-up calls.  `--tiles`: the channel tiles to time per shape -- 0 is the planned one; a tile
that does not fit the LDS for a shape is skipped.  Prints one JSON line per shape and tile."""
import argparse
import json

from bench_util import timed
#: name -> (S, Sh, C): the distinct token shapes of graphs.MIXER_MODELS
SHAPES = (("mixer_s32_224", 49, 256, 512), ("mixer_s16_224", 196, 256, 512), ("mixer_b32_224", 49, 384, 768), ("mixer_b16_224", 196, 384, 768),
          ("mixer_l32_224", 49, 512, 1024), ("mixer_l16_224", 196, 512, 1024), ("resmlp_*_224", 196, 0, 384))
PEAK_TFLOPS = 157.3
FLOOR_TBS = (4.7, 5.0)
LDS = 160 * 1024


def main():
    import torch
    import torch.nn.functional as F
    from i2v_amd import attacks
    from i2v_amd import lib as _lib
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=128)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--tiles", default="0,32,64")
    a = ap.parse_args()
    eng = attacks.get_engine("cuda:0")
    capi, st = eng.capi, eng.stream()
    P = lambda t: None if t is None else t.data_ptr()      # noqa: E731
    Fr = a.frames
    for name, S, Sh, Cn in SHAPES:
        gen = torch.Generator().manual_seed(S * 1000 + Cn)
        R = lambda *shape: torch.randn(*shape, generator=gen).cuda()      # noqa: E731
        z, r, g = R(Fr, S, Cn), R(Fr, S, Cn), R(Fr, S, Cn)
        if Sh:
            w1, b1, w2, b2 = R(Sh, S) * S ** -0.5, R(Sh), R(S, Sh) * Sh ** -0.5, R(S)
            sc = sh = osc = None
            w2t, w1t = w2.t().contiguous(), w1.t().contiguous()
        else:
            w1, b1, w2, b2 = R(S, S) * S ** -0.5, R(S), None, None
            sc, sh, osc = R(Cn), R(Cn), R(Cn)
            w2t, w1t = w1.t().contiguous(), None
        out, dz = torch.empty_like(z), torch.empty_like(z)
        K = Sh if Sh else S
        flop_f, flop_b = (4 if Sh else 2) * Fr * Cn * S * K, (6 if Sh else 2) * Fr * Cn * S * K
        bytes_f, bytes_b = 3 * z.numel() * 4, (3 if Sh else 2) * z.numel() * 4      # forward: z, residual, out; backward: (z,) g, dz
        # eager: the same tensors, token-major
        zr = z.clone().requires_grad_(True)

        def eager():
            t = zr if sc is None else sc * zr + sh
            u = w1 @ t + b1[:, None]
            if Sh:
                u = w2 @ F.gelu(u) + b2[:, None]
            return r + (u if osc is None else osc * u)
        with torch.no_grad():
            eager_f = timed(eager, a.reps, 3)[0]
        y = eager()
        eager_b = timed(lambda: torch.autograd.grad(y, zr, g, retain_graph=True), a.reps, 3)[0]
        for tile in [int(t) for t in a.tiles.split(",")]:
            ct = tile or 32
            if (S + Sh) * ct * 4 > LDS:
                continue

            def fwd():
                _lib.check(capi, capi.i2v_mixer_tokens_f32(P(z), P(r), P(out), Fr, S, Sh, Cn, P(w1), P(b1), P(w2), P(b2), P(sc), P(sh), P(osc),
                                                           tile, st))

            def bwd():
                _lib.check(capi, capi.i2v_mixer_tokens_bwd_f32(P(z) if Sh else None, P(g), None, P(dz), Fr, S, Sh, Cn, P(w1) if Sh else None,
                                                               P(b1) if Sh else None, P(w2t), P(w1t), P(sc), P(sh), P(osc), tile, st))
            row = {"name": name, "S": S, "Sh": Sh, "C": Cn, "frames": Fr, "tile": tile, "channel_tile": ct, "lds_bytes": (S + Sh) * ct * 4,
                   "workgroups": Fr * -(-Cn // ct)}
            for label, fn, flop, nbytes, eg in (("forward", fwd, flop_f, bytes_f, eager_f), ("input_gradient", bwd, flop_b, bytes_b, eager_b)):
                ms = timed(fn, a.reps, 3)[0]
                row[label] = {"call_ms": round(ms, 4), "TFLOP/s": round(flop / ms / 1e9, 2), "flop_floor_ms": round(flop / PEAK_TFLOPS / 1e9, 4),
                              "share_of_flop_floor": round(flop / PEAK_TFLOPS / 1e9 / ms, 3),
                              "byte_floor_ms": [round(nbytes / t / 1e9, 4) for t in FLOOR_TBS], "eager_ms": round(eg, 4),
                              "eager_over_kernel": round(eg / ms, 2)}
            print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
