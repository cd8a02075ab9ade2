"""The ConvNeXt blocks' token-major depthwise 7 x 7 launch (csrc/i2v_convnext.hip) on the four stage shapes of `convnext_tiny` at 128
frames, forward and input gradient (the same kernel on the mirrored filter, plus the residual gradient it adds), next to eager PyTorch's
`F.conv2d(groups=C)` in channels-last format on the same device.

    python tools/convnext_dw_bench.py [--frames 128] [--reps 20]
    python tools/convnext_dw_bench.py kernels KERNEL_TRACE_CSV [--frames 128]      # kernel time from a profiler trace of the run above

The first form times CALLS: one HIP event pair around each `Engine.convnext_dw` call (an output allocation, the ctypes call, the
launch), the median of `reps` calls after 3 warm-up calls; for the launches of a few tens of microseconds the host's enqueue latency is
inside the window.  The second form reads the `kernel_trace.csv` that `rocprofv3 --kernel-trace --output-format csv` writes for such a
run and gives the median KERNEL time per shape and pass (the dispatches of `convnext_dw_kernel` are told apart by their grid; per shape
the forward calls come first).  Algorithmic bytes per pass:
one read and one write of the tensor plus the filter (the backward's residual gradient is a second read, counted).  The byte floor uses the
4.7 to 5.0 TB/s of DESIGN.md section 4.  Prints one JSON line per shape."""
import argparse
import json
import statistics
import sys

from bench_util import timed
SHAPES = ((96, 56), (192, 28), (384, 14), (768, 7))
FLOOR_TBS = (4.7, 5.0)


def kernels(path, frames):
    import csv
    rows = [r for r in csv.DictReader(open(path)) if "convnext_dw_kernel" in r.get("Kernel_Name", "")]
    for Cc, g in SHAPES:
        gx = -(-(g * -(-g // 8) * (Cc // 4)) // 256)                   # blocks of 256 items: rows x runs of 8 x channel groups of 4
        # the trace gives grids in work-items: x = blocks * 256, y = frames
        mine = [r for r in rows if int(r["Grid_Size_X"]) == gx * 256 and int(r["Grid_Size_Y"]) == frames]
        mine.sort(key=lambda r: int(r["Start_Timestamp"]))
        ns = [int(r["End_Timestamp"]) - int(r["Start_Timestamp"]) for r in mine]
        half = len(ns) // 2
        tensor, filt = frames * g * g * Cc * 4, 49 * Cc * 4
        row = {"C": Cc, "plane": g, "frames": frames, "dispatches": len(ns)}
        for name, part, nbytes in (("forward", ns[:half], 2 * tensor + filt), ("input_gradient", ns[half:], 3 * tensor + filt)):
            us = statistics.median(part) / 1e3
            gbs = nbytes / us / 1e3
            row[name] = {"kernel_us": round(us, 2), "GB/s": round(gbs, 1), "share_of_floor": [round(gbs / (t * 1e3), 3) for t in FLOOR_TBS]}
        print(json.dumps(row))


def main():
    if len(sys.argv) >= 3 and sys.argv[1] == "kernels":
        return kernels(sys.argv[2], int(sys.argv[4]) if len(sys.argv) > 4 else 128)
    import torch
    import torch.nn.functional as F
    from i2v_amd import attacks
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=128)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    eng = attacks.get_engine("cuda:0")
    for Cc, g in SHAPES:
        gen = torch.Generator().manual_seed(Cc)
        x = torch.randn(a.frames, g, g, Cc, generator=gen).cuda()
        w = (torch.randn(49, Cc, generator=gen) / 7).cuda()
        b = torch.randn(Cc, generator=gen).cuda()
        res = torch.randn(a.frames, g, g, Cc, generator=gen).cuda()
        wm = w.flip(0).contiguous()
        tensor, filt = x.numel() * 4, w.numel() * 4
        row = {"C": Cc, "plane": g, "frames": a.frames}
        for name, fn, nbytes in (("forward", lambda: eng.convnext_dw(x, w, b), 2 * tensor + filt),
                                 ("input_gradient", lambda: eng.convnext_dw(x, wm, None, res), 3 * tensor + filt)):
            ms = timed(fn, a.reps, 3)[0]
            gbs = nbytes / ms / 1e6
            row[name] = {"call_ms": round(ms, 4), "GB/s": round(gbs, 1), "floor_ms": [round(nbytes / t / 1e9, 4) for t in FLOOR_TBS],
                         "share_of_floor": [round(gbs / (t * 1e3), 3) for t in FLOOR_TBS]}
        # eager: NCHW-shaped tensors in channels-last memory format are the same bytes as the token-major tensor
        xe = x.permute(0, 3, 1, 2).requires_grad_(True)
        we = w.t().reshape(Cc, 1, 7, 7).contiguous()
        assert xe.is_contiguous(memory_format=torch.channels_last)
        row["eager_forward_ms"] = round(timed(lambda: F.conv2d(xe.detach(), we, b, padding=3, groups=Cc), a.reps, 3)[0], 4)
        y = F.conv2d(xe, we, b, padding=3, groups=Cc)
        dy = res.permute(0, 3, 1, 2)
        row["eager_input_gradient_ms"] = round(timed(lambda: torch.autograd.grad(y, xe, dy, retain_graph=True), a.reps, 3)[0], 4)
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
