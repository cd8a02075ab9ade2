"""Window attention against the do-nothing alternative: on the stage-0 and stage-1 shapes of swin_base at 128
frames, the dedicated kernels (`i2v_swin_window_attention_f32` / `_bwd_f32`, shifted block: bias, mask and window addressing included)
and the ViT attention entries called with frames = number of windows (`i2v_vit_attention_f32` / `_bwd_f32`: three and five batched
GEMMs and a softmax pass, no bias, no mask, windows handed over contiguous).  Prints host-timed milliseconds per call.

For the device times the design quotes, run it under the profiler and reduce the per-dispatch trace with this same file:

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o swin_attn -- python tools/swin_attention_bench.py
    python tools/swin_attention_bench.py --reduce OUT/.../swin_attn_kernel_trace.csv

The reduction relies on the launch order below: per shape, per route, one warm-up call and REPS timed ones, a call being 1, 1, 3 and 5
kernels (the Swin forward and backward; the ViT forward's two GEMMs and softmax; the ViT backward's four GEMMs and softmax backward).
The two shapes launch kernels of the same names, so only the per-dispatch trace can tell them apart, not the profiler's stats file."""
import csv
import ctypes as C
import json
import sys
import time

import bench_util  # noqa: F401 (puts the repository on sys.path)

REPS = 5
SHAPES = ((128, 56, 4), (128, 28, 8))           # frames, grid, heads: stage 0 and stage 1 of swin_base
ROUTES = (("swin forward", 1, ("swin_attn_fwd",)), ("swin backward", 1, ("swin_attn_bwd",)),
          ("vit-route forward", 3, ("vit_gemm", "vit_softmax_kernel")), ("vit-route backward", 5, ("vit_gemm", "vit_softmax_bwd")))


def reduce_trace(path):
    """Device microseconds per call (mean and minimum over the REPS timed calls, the warm-up call left out) per shape and route."""
    rows = [r for r in csv.DictReader(open(path)) if any(m in r["Kernel_Name"] for m in ("swin_attn_", "vit_gemm", "vit_softmax"))]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    i, out = 0, []
    for F, g, heads in SHAPES:
        per_shape = {}
        for route, n, marks in ROUTES:
            chunk = rows[i:i + (REPS + 1) * n]
            i += (REPS + 1) * n
            assert len(chunk) == (REPS + 1) * n and all(any(m in r["Kernel_Name"] for m in marks) for r in chunk), (route, len(chunk))
            us = [sum(int(r["End_Timestamp"]) - int(r["Start_Timestamp"]) for r in chunk[k * n:(k + 1) * n]) / 1e3 for k in range(REPS + 1)]
            per_shape[route] = {"kernels_per_call": n, "mean_us": round(sum(us[1:]) / REPS, 1), "min_us": round(min(us[1:]), 1)}
        new = per_shape["swin forward"]["mean_us"] + per_shape["swin backward"]["mean_us"]
        old = per_shape["vit-route forward"]["mean_us"] + per_shape["vit-route backward"]["mean_us"]
        out.append({"frames": F, "grid": g, "heads": heads, "problems": F * (g // 7) ** 2 * heads, "routes": per_shape,
                    "swin_us": round(new, 1), "vit_route_us": round(old, 1), "vit_route_over_swin": round(old / new, 3)})
    assert i == len(rows), (i, len(rows))
    print(json.dumps(out, indent=1))


def p(t):
    return C.c_void_p(t.data_ptr())


def main(reps=REPS):
    if len(sys.argv) == 3 and sys.argv[1] == "--reduce":
        return reduce_trace(sys.argv[2])
    import torch
    from i2v_amd import attacks
    from i2v_amd import lib as _lib
    eng = attacks.get_engine("cuda:0")
    capi, st = eng.capi, eng.stream()
    for F, g, heads in SHAPES:
        dh, ws, T = 32, 7, 49
        Cw, nwin = heads * dh, F * (g // ws) ** 2
        qkv = torch.randn(F, g * g, 3 * Cw, device="cuda")
        dout = torch.randn(F, g * g, Cw, device="cuda")
        table = 0.5 * torch.randn(169, heads, device="cuda")
        out, dqkv = torch.empty_like(dout), torch.empty_like(qkv)
        ld = capi.i2v_vit_probs_ld(T)
        probs = torch.empty(nwin, heads, T, ld, device="cuda")
        dprobs = torch.empty_like(probs)
        calls = {
            "swin forward": lambda: capi.i2v_swin_window_attention_f32(p(qkv), F, g, g, ws, 3, heads, dh, p(table), p(out), st),
            "swin backward": lambda: capi.i2v_swin_window_attention_bwd_f32(p(qkv), p(dout), F, g, g, ws, 3, heads, dh, p(table), p(dqkv), st),
            "vit-route forward": lambda: capi.i2v_vit_attention_f32(p(qkv), nwin, T, heads, dh, dh ** -0.5, p(probs), p(out), st),
            "vit-route backward": lambda: capi.i2v_vit_attention_bwd_f32(p(qkv), p(probs), p(dout), nwin, T, heads, dh, dh ** -0.5,
                                                                         p(dprobs), p(dqkv), st),
        }
        for name, fn in calls.items():
            _lib.check(capi, fn())                                  # warm-up
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(reps):
                _lib.check(capi, fn())
            torch.cuda.synchronize()
            print(f"grid {g} heads {heads} ({nwin * heads} problems): {name} {1e3 * (time.perf_counter() - t0) / reps:.3f} ms", flush=True)


if __name__ == "__main__":
    main()
