"""The quality launch pair (csrc/i2v_quality.hip: the tile launch and the per-frame fold) at 128 frames of 224 x 224, in both modes
(8-bit frames, normalised fp32 clips), next to two yardsticks:

  * the byte floor at 4.7 TB/s: both operands read once plus the scratch partials and the 24 bytes a frame that come out;
  * eager PyTorch on the same GPU: the same formula composed of `F.conv2d` calls with the separable 11-tap window over the five moment
    maps, in float32 (checked to agree with the kernel first, to 1e-4: eager's fp32 moments are not the kernel's double ones).

    python tools/quality_bench.py run [--frames 128] [--hw 224] [--reps 30]
    rocprofv3 --kernel-trace --stats -d DIR -o quality -- python tools/quality_bench.py run     # profiler kernel time
    python tools/quality_bench.py stats DIR/.../quality_results.db [--frames 128]    # the table from that run (or its kernel stats csv)

`run` times CALLS between HIP event pairs (median, fastest, slowest of `reps` warm calls) and prints one JSON line per mode; under the
profiler the same calls give the kernel times, which `stats` reads: the two kernels of each mode per call against the byte floor, and
everything else (eager's kernels and the input generators) summed."""
import argparse
import json

from bench_util import kernel_rows, timed

FLOOR_TBS = 4.7
WARM = 5
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def floor_ms(mode, frames, hw, tiles):
    per_elem = 1 if mode == "u8" else 4
    return (2 * frames * 3 * hw * hw * per_elem + frames * tiles * 24 * 2 + frames * 24) / (FLOOR_TBS * 1e12) * 1e3


def eager_ssim(la, lb, g):
    """Mean SSIM per frame of levels (n, 3, h, w), float32, separable window `g` (11,): 10 conv2d calls and the formula."""
    import torch.nn.functional as F

    def filt(x):
        n, c, h, w = x.shape
        x = x.reshape(n * c, 1, h, w)
        return F.conv2d(F.conv2d(x, g.view(1, 1, 1, 11)), g.view(1, 1, 11, 1)).reshape(n, c, h - 10, w - 10)
    va, vb = la - 127.5, lb - 127.5
    ma, mb = filt(va), filt(vb)
    saa, sbb, sab = filt(va * va) - ma * ma, filt(vb * vb) - mb * mb, filt(va * vb) - ma * mb
    Ma, Mb = ma + 127.5, mb + 127.5
    c1, c2 = (0.01 * 255) ** 2, (0.03 * 255) ** 2
    return (((2 * Ma * Mb + c1) * (2 * sab + c2)) / ((Ma * Ma + Mb * Mb + c1) * (saa + sbb + c2))).mean(dim=(1, 2, 3))


def one(mode, frames, hw, reps):
    import torch
    from i2v_amd import attacks
    eng = attacks.get_engine("cuda:0")
    gen = torch.Generator().manual_seed(11)
    a8 = torch.randint(0, 256, (frames, hw, hw, 3), generator=gen, dtype=torch.uint8)
    b8 = (a8.int() + torch.randint(-16, 17, a8.shape, generator=gen, dtype=torch.int32)).clamp(0, 255).to(torch.uint8)
    a8, b8 = a8.cuda(), b8.cuda()
    if mode == "u8":
        a, b = a8, b8
        la, lb = (t.permute(0, 3, 1, 2).float().contiguous() for t in (a8, b8))
    else:
        a, b = eng.clip_from_u8(a8[None]), eng.clip_from_u8(b8[None])                    # one clip of `frames` frames
        mean, std = (torch.tensor(v, device="cuda").view(1, 3, 1, 1, 1) for v in (MEAN, STD))
        la, lb = ((255 * (t * std + mean))[0].transpose(0, 1).contiguous() for t in (a, b))
    k = torch.arange(11, dtype=torch.float64) - 5
    g = torch.exp(-k * k / 4.5)
    g = (g / g.sum()).float().cuda()
    got = eng.clip_quality(a, b)
    torch.cuda.synchronize()
    agree = float((got[:, 2].float() - eager_ssim(la, lb, g)).abs().max())
    assert agree < 1e-4, agree
    tr, tc = eng.clip_quality_tile()
    tiles = (-(-(hw - 10) // tr)) * (-(-(hw - 10) // tc))
    nbytes = int(eng.capi.i2v_clip_quality_scratch_bytes(frames, hw, hw))
    out = torch.empty(frames, 3, dtype=torch.float64, device="cuda")
    scratch = torch.empty(nbytes // 8, dtype=torch.float64, device="cuda")
    P, st = (lambda t: t.data_ptr()), eng.stream()
    if mode == "u8":
        fn = lambda: eng.capi.i2v_clip_quality_u8(P(a), P(b), P(out), frames, hw, hw, P(scratch), nbytes, st)      # noqa: E731
    else:
        fn = lambda: eng.capi.i2v_clip_quality_f32(P(a), P(b), P(out), 1, frames, hw, hw, P(scratch), nbytes, st)      # noqa: E731
    ms, lo, hi = timed(fn, reps, WARM)
    assert torch.equal(out, got)
    with torch.no_grad():
        eg = timed(lambda: eager_ssim(la, lb, g), reps, WARM)
    fl = floor_ms(mode, frames, hw, tiles)
    print(json.dumps({"mode": mode, "frames": frames, "hw": hw, "tile": [tr, tc], "tiles_per_frame": tiles, "eager_agrees_to": agree,
                      "call_ms": round(ms, 4), "fastest_slowest_ms": [round(lo, 4), round(hi, 4)], "byte_floor_ms": round(fl, 4),
                      "share_of_floor": round(fl / ms, 3), "eager_ms": round(eg[0], 4), "eager_fastest_slowest_ms": [round(eg[1], 4), round(eg[2], 4)],
                      "eager_over_kernel": round(eg[0] / ms, 2)}), flush=True)


def stats(path, frames, hw):
    """The profiler's kernel stats of one `run`: the tile kernel of each mode and the frame kernel per call against the byte floor, and
    everything else (eager's kernels, the loader's, the input generators) summed."""
    ours, rest = {}, 0.0
    for name, calls, total in kernel_rows(path):
        if "ql_tile_kernel" in name or "ql_frame_kernel" in name:
            ours[name] = (calls, total / calls / 1e6)
        else:
            rest += total
    frame_ms = sum(ms for name, (_, ms) in ours.items() if "ql_frame_kernel" in name)
    for name, (calls, ms) in sorted(ours.items()):
        row = {"kernel": name, "calls": calls, "kernel_ms": round(ms, 4)}
        if "ql_tile_kernel" in name:
            mode = "u8" if ("Lb1" in name or "<true>" in name) else "f32"
            fl = floor_ms(mode, frames, hw, (-(-(hw - 10) // 16)) * (-(-(hw - 10) // 32)))
            row.update({"mode": mode, "pair_ms": round(ms + frame_ms, 4), "byte_floor_ms": round(fl, 4), "share_of_floor": round(fl / (ms + frame_ms), 3)})
        print(json.dumps(row))
    print(json.dumps({"other_kernels_total_ms": round(rest / 1e6, 3), "note": "eager's kernels, the loader's and the input generators, all calls"}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=("run", "stats"))
    ap.add_argument("path", nargs="?")
    ap.add_argument("--frames", type=int, default=128)
    ap.add_argument("--hw", type=int, default=224)
    ap.add_argument("--reps", type=int, default=30)
    a = ap.parse_args()
    if a.mode == "stats":
        return stats(a.path, a.frames, a.hw)
    for mode in ("u8", "f32"):
        one(mode, a.frames, a.hw, a.reps)


if __name__ == "__main__":
    main()
