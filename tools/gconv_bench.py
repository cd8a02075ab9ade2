"""The grouped-convolution kernel against the dense route on the conv2 shapes of resnext50_32x4d -- every stage's
stride-1 member and, from stage 2 on, its stride-2 entry: seven shapes -- at `--frames` frames (default 128), forward and input gradient.

    python tools/gconv_bench.py [--frames 128] [--reps 5]
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o gconv -- python tools/gconv_bench.py     # device times per kernel

Each shape is the net "3-channel stem 3x3 -> grouped conv -> hook" planned twice, with I2V_GCONV unset (one `gconv_kernel` launch per
pass) and with I2V_GCONV=0 (block-diagonal weight through the dense kernels: one forward launch, one input-gradient launch per stride
parity).  Times are the engine's own per-launch event pairs (`I2V_TIMING_DUMP`), the stem's launches left out; the best of `--reps`.
TFLOP/s and GB/s count the node's real products and its algorithmic bytes on both routes.  Prints one JSON line per shape."""
import argparse
import ctypes as C
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "image-to-video-i2v-attack_amd")]

SHAPES = ((128, 56, 1), (256, 56, 2), (256, 28, 1), (512, 28, 2), (512, 14, 1), (1024, 14, 2), (1024, 7, 1))     # channels, input plane, stride


def timed(eng, net, x, gx, reps, dump):
    """Best (forward ms, backward ms, GFLOP, MB) of the grouped node's launches: every kind-0 / kind-5 line but the stem's (K = 27)."""
    import torch
    best = None
    for _ in range(reps + 1):
        open(dump, "w").close()
        eng.capi.i2v_timing_enable(eng.h, 1)
        net.forward(x)
        net.backward(gx)
        torch.cuda.synchronize()
        out = (C.c_double * (8 * 8))()
        eng.capi.i2v_timing_collect_ex(eng.h, out, 8, 8)
        eng.capi.i2v_timing_enable(eng.h, 0)
        rows = [ln.split() for ln in open(dump)]
        fwd = [r for r in rows if r[0] == "0" and r[2] != "27"]
        bwd = [r for r in rows if r[0] == "5"]
        cur = (sum(float(r[6]) for r in fwd), sum(float(r[6]) for r in bwd), sum(float(r[7]) for r in fwd), sum(float(r[8]) for r in fwd + bwd))
        if best is None or cur[0] + cur[1] < best[0] + best[1]:
            best = cur
    return best


def main():
    import torch
    from i2v_amd import attacks, weights
    from tests.resnet_family_reference import node_alone_graph
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=128)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    dump = os.path.join(tempfile.mkdtemp(), "launches.txt")
    os.environ["I2V_TIMING_DUMP"] = dump
    os.environ["I2V_AUTOTUNE"] = os.environ.get("I2V_AUTOTUNE", "1")
    eng = attacks.get_engine("cuda:0")
    for ch, plane, stride in SHAPES:
        g = node_alone_graph(ch, 32, plane, stride)
        sd = weights.synthetic_state_dict(g, 0)
        x = torch.randn(a.frames, 3, plane, plane, device="cuda:0")
        gx = torch.empty_like(x)
        res = {"C": ch, "group_width": ch // 32, "plane": plane, "stride": stride, "frames": a.frames}
        for route in ("kernel", "dense"):
            os.environ.pop("I2V_GCONV", None)
            if route == "dense":
                os.environ["I2V_GCONV"] = "0"
            net = eng.build_net(g, sd, [g.hooks[1]], a.frames)
            f, b, gflop, mb = timed(eng, net, x, gx, a.reps, dump)
            net.close()
            res[route] = {"fwd_ms": round(f, 4), "bwd_ms": round(b, 4), "tflops": round(2 * gflop / (f + b), 2), "gb_per_s": round(mb / (f + b), 1)}
        res["kernel_wins"] = sum(res["kernel"][k] for k in ("fwd_ms", "bwd_ms")) < sum(res["dense"][k] for k in ("fwd_ms", "bwd_ms"))
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
