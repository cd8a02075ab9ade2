"""The depthwise-convolution kernel against the dense route on the 17 depthwise nodes of mnasnet1_0 at 224 x 224
-- 12 distinct shapes, each listed with the number of nodes that have it -- at `--frames` frames (default 128), forward and input
gradient.

    python tools/dwconv_bench.py [--frames 128] [--reps 5]
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o dwconv -- python tools/dwconv_bench.py     # device times per kernel

Each shape is the net "1x1 lift of the 3-channel input -> depthwise conv -> hook" planned twice, with I2V_DWCONV unset (one
`dwconv_kernel` launch per pass) and with I2V_DWCONV=0 (block-diagonal weight through the dense kernels: one forward launch, one
input-gradient launch per stride parity).  Times are the engine's own per-launch event pairs (`I2V_TIMING_DUMP`), the lift's launches
left out; the best of `--reps`.  TFLOP/s count the node's real products (2 C k k Ho Wo per frame and pass), GB/s its algorithmic
bytes (per pass: 4 bytes per source and per destination element plus one gate bit per element of the gated plane) on both routes;
`floor` is the kernel route's share of the byte floor at 4.7 and at 5.0 TB/s.  One JSON line per shape."""
import argparse
import ctypes as C
import json
import os
import sys
import tempfile
from collections import Counter

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "image-to-video-i2v-attack_amd")]


def shapes():
    """(channels, k, input plane, stride) -> number of mnasnet1_0 nodes with that shape, in network order."""
    from i2v_amd import graphs
    g = graphs.build("mnasnet1_0", (224, 224))
    return Counter((nd.cin, nd.kh, g.tensors[nd.src].H, nd.stride) for nd in g.nodes if nd.op == "conv" and nd.groups > 1)


def timed(eng, net, x, gx, reps, dump):
    """Best (forward ms, backward ms) of the depthwise node's launches: every kind-0 / kind-5 line but the lift's (K = 3)."""
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
        fwd = [r for r in rows if r[0] == "0" and r[2] != "3"]
        bwd = [r for r in rows if r[0] == "5"]
        cur = (sum(float(r[6]) for r in fwd), sum(float(r[6]) for r in bwd))
        if best is None or cur[0] + cur[1] < best[0] + best[1]:
            best = cur
    return best


def main():
    import torch
    from i2v_amd import attacks, weights
    from tests.mnasnet_reference import node_alone_graph
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=128)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    dump = os.path.join(tempfile.mkdtemp(), "launches.txt")
    os.environ["I2V_TIMING_DUMP"] = dump
    os.environ["I2V_AUTOTUNE"] = os.environ.get("I2V_AUTOTUNE", "1")
    eng = attacks.get_engine("cuda:0")
    for (ch, k, plane, stride), count in shapes().items():
        g = node_alone_graph(ch, k, plane, stride)
        sd = weights.synthetic_state_dict(g, 0)
        x = torch.randn(a.frames, 3, plane, plane, device="cuda:0")
        gx = torch.empty_like(x)
        out = (plane + 2 * (k // 2) - k) // stride + 1
        n_in, n_out = a.frames * ch * plane * plane, a.frames * ch * out * out
        gflop = 2.0 * n_out * k * k / 1e9                                      # per pass
        mb = (4.0 * (n_in + n_out) + n_out / 8.0 + 4.0 * (n_in + n_out) + n_in / 8.0) / 1e6      # forward + input gradient
        res = {"C": ch, "k": k, "plane": plane, "stride": stride, "frames": a.frames, "nodes": count}
        for route in ("kernel", "dense"):
            os.environ.pop("I2V_DWCONV", None)
            if route == "dense":
                os.environ["I2V_DWCONV"] = "0"
            net = eng.build_net(g, sd, [g.hooks[1]], a.frames)
            f, b = timed(eng, net, x, gx, a.reps, dump)
            net.close()
            res[route] = {"fwd_ms": round(f, 4), "bwd_ms": round(b, 4), "tflops": round(2 * gflop / (f + b), 3), "gb_per_s": round(mb / (f + b), 1)}
        os.environ.pop("I2V_DWCONV", None)
        res["floor"] = {"at_4.7_TB_s": round(res["kernel"]["gb_per_s"] / 4700, 3), "at_5.0_TB_s": round(res["kernel"]["gb_per_s"] / 5000, 3)}
        res["dense_over_kernel"] = round((res["dense"]["fwd_ms"] + res["dense"]["bwd_ms"]) / (res["kernel"]["fwd_ms"] + res["kernel"]["bwd_ms"]), 2)
        res["kernel_wins"] = res["dense_over_kernel"] > 1
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
