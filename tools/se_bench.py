"""The squeeze-and-excitation node on the four stage shapes of seresnet50 at 224 x 224 -- 256 x 56^2, 512 x 28^2,
1024 x 14^2, 2048 x 7^2, squeezed widths 16, 32, 64, 128 -- at `--frames` frames (default 128), forward plus input gradient.

    python tools/se_bench.py [--frames 128] [--reps 5] [--step-timeout 300]

Every shape runs in a child process of its own under `timeout -k 10 <step-timeout>`; the first child that fails ends the run with its
exit status (nothing more is started on the device).  Each shape is the net "3x3 stem -> 1x1 convolution (linear) -> SE node with the
stem output as residual -> hook" (tests/seresnet_reference.py).  Times are the engine's own per-launch event pairs
(`I2V_TIMING_DUMP`: the SE launches carry 20 + stage + 3 x backward in the `pw` field), the best of `--reps`, for each of the six
launches: ms, GB/s of the launch's algorithmic bytes (what the engine's timing records count: every plane, vector and matrix once) and
its share of the byte floor at 4.7 and at 5.0 TB/s.  Alongside: the float32 eager-PyTorch run of the reference
module on the same device -- mean, two 1x1 convolutions, sigmoid, scale, add, ReLU, and autograd's backward to the module's input --
timed with device events, best of `--reps`.  One JSON line per shape."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "image-to-video-i2v-attack_amd")]

SHAPES = ((256, 16, 56), (512, 32, 28), (1024, 64, 14), (2048, 128, 7))        # (C, rd, plane): layer1 .. layer4 of seresnet50
LAUNCHES = ("fwd_squeeze", "fwd_excite", "fwd_scale", "bwd_squeeze", "bwd_excite", "bwd_scale")


def engine_times(ch, rd, plane, frames, reps):
    import torch
    from i2v_amd import attacks, weights
    from tests.seresnet_reference import node_alone_graph
    dump = os.path.join(tempfile.mkdtemp(), "launches.txt")
    os.environ["I2V_TIMING_DUMP"] = dump
    eng = attacks.get_engine("cuda:0")
    g = node_alone_graph(ch, rd, plane, True, True)
    net = eng.build_net(g, weights.synthetic_state_dict(g, 0), [g.hooks[1]], frames)
    x = torch.randn(frames, 3, plane, plane, device="cuda:0")
    gx = torch.empty_like(x)
    best = {}
    for _ in range(reps + 1):
        open(dump, "w").close()
        eng.capi.i2v_timing_enable(eng.h, 1)
        net.forward(x)
        net.backward(gx)
        torch.cuda.synchronize()
        out = (C.c_double * (8 * 8))()
        eng.capi.i2v_timing_collect_ex(eng.h, out, 8, 8)
        eng.capi.i2v_timing_enable(eng.h, 0)
        for r in (ln.split() for ln in open(dump)):
            if 20 <= int(r[5]) <= 25:
                name = LAUNCHES[int(r[5]) - 20]
                ms, mb = float(r[6]), float(r[8])
                if name not in best or ms < best[name][0]:
                    best[name] = (ms, mb)
    net.close()
    assert set(best) == set(LAUNCHES), sorted(best)
    return best


def eager_times(ch, rd, plane, frames, reps):
    """(forward ms, backward ms) of the reference module in eager PyTorch, float32, on the device."""
    import torch
    import torch.nn.functional as F
    dev = "cuda:0"
    w1, b1 = torch.randn(rd, ch, 1, 1, device=dev) * 0.05, torch.zeros(rd, device=dev)
    w2, b2 = torch.randn(ch, rd, 1, 1, device=dev) * 0.05, torch.zeros(ch, device=dev)
    x = torch.randn(frames, ch, plane, plane, device=dev, requires_grad=True)
    r = torch.randn(frames, ch, plane, plane, device=dev)
    gy = torch.randn(frames, ch, plane, plane, device=dev)
    best = None
    for _ in range(reps + 1):
        e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        e[0].record()
        s = torch.sigmoid(F.conv2d(F.relu(F.conv2d(x.mean((2, 3), keepdim=True), w1, b1)), w2, b2))
        y = F.relu(x * s + r)
        e[1].record()
        g, = torch.autograd.grad(y, x, gy)
        e[2].record()
        torch.cuda.synchronize()
        cur = (e[0].elapsed_time(e[1]), e[1].elapsed_time(e[2]))
        if best is None or sum(cur) < sum(best):
            best = cur
    return best


def one_shape(ch, rd, plane, frames, reps):
    eng = engine_times(ch, rd, plane, frames, reps)
    ef, eb = eager_times(ch, rd, plane, frames, reps)
    res = {"C": ch, "rd": rd, "plane": plane, "frames": frames, "launches": {}}
    for name in LAUNCHES:
        ms, mb = eng[name]
        gbs = mb / ms if ms > 0 else 0.0          # MB / ms = GB/s
        res["launches"][name] = {"ms": round(ms, 4), "gb_per_s": round(gbs, 1), "floor_at_4.7_TB_s": round(gbs / 4700, 3), "floor_at_5.0_TB_s": round(gbs / 5000, 3)}
    tot = sum(eng[n][0] for n in LAUNCHES)
    res["engine_ms"] = round(tot, 4)
    res["engine_gb_per_s"] = round(sum(eng[n][1] for n in LAUNCHES) / tot, 1)
    res["eager_fp32"] = {"fwd_ms": round(ef, 4), "bwd_ms": round(eb, 4)}
    res["eager_over_engine"] = round((ef + eb) / tot, 2)
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=128)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--step-timeout", type=int, default=300)
    ap.add_argument("--shape", type=int, default=-1, help="(internal) run this one shape in this process")
    a = ap.parse_args()
    if a.shape >= 0:
        one_shape(*SHAPES[a.shape], a.frames, a.reps)
        return 0
    for i in range(len(SHAPES)):            # one device step per shape, each under its own time limit; stop at the first failure
        rc = subprocess.run(["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__), "--shape", str(i),
                             "--frames", str(a.frames), "--reps", str(a.reps)]).returncode
        if rc != 0:
            print(f"shape {SHAPES[i]} ended with status {rc}: stopping", file=sys.stderr)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
