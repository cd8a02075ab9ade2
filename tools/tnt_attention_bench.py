"""The TNT batched short-sequence attention launches (csrc/i2v_tnt.hip) on the inner shapes of tnt_s_patch16_224 and tnt_b_patch16_224
at 128 frames (25 088 sequences of 16 tokens, 4 heads of width 6 / 10), forward and input gradient, next to two yardsticks:

  * the byte floor at 4.7 TB/s: forward qkv read once and out written once; backward qkv and dout read and dqkv written;
  * eager PyTorch on the same GPU: softmax(scale q k^T) v on contiguous (S, H, 16, dh) tensors in float32 and its autograd backward to
    q, k and v (checked to agree with the kernel first).
There is no composed route to compare: the shared `xf_attention` launches do not accept this shape without change -- their batched GEMM
counts frames x heads in one grid dimension and refuses a batch over 65 535 (here 100 352).

    python tools/tnt_attention_bench.py run [--frames 128] [--reps 30] [--shape s|b|all]
    rocprofv3 --kernel-trace --stats -d DIR -o tnt -- python tools/tnt_attention_bench.py run     # profiler kernel time
    python tools/tnt_attention_bench.py stats DIR/.../tnt_results.db [--frames 128]    # the table from that run (or its kernel stats csv)

`run` times CALLS between HIP event pairs (median, fastest, slowest of `reps` warm calls) and prints one JSON line per shape; under
the profiler the same calls give the kernel times, which `stats` reads: per kernel its calls and average, the kernel against its byte
floor, and eager's kernels summed per call."""
import argparse
import json

from bench_util import kernel_rows, timed
#: label -> (heads, dh): the inner attention of tnt_s and tnt_b; 16 tokens, 196 sequences a frame
SHAPES = {"s": (4, 6), "b": (4, 10)}
FLOOR_TBS = 4.7
WARM = 5


def floors(frames, H, dh):
    """(forward, backward) byte floor in ms."""
    S, C = frames * 196, H * dh
    return tuple(S * 16 * C * n * 4 / (FLOOR_TBS * 1e12) * 1e3 for n in (4, 7))


def one(label, frames, reps):
    import torch
    from i2v_amd import attacks
    H, dh = SHAPES[label]
    S, T, Cn = frames * 196, 16, H * dh
    eng = attacks.get_engine("cuda:0")
    gen = torch.Generator().manual_seed(100 + dh)
    qkv = torch.randn(S, T, 3 * Cn, generator=gen).cuda()
    dout = torch.randn(S, T, Cn, generator=gen).cuda()
    out = eng.tnt_attention(qkv, H)
    dqkv = eng.tnt_attention_bwd(qkv, dout, H)
    torch.cuda.synchronize()
    q, k, v = (t.contiguous().requires_grad_(True) for t in qkv.reshape(S, T, 3, H, dh).permute(2, 0, 3, 1, 4).unbind(0))
    g = dout.reshape(S, T, H, dh).transpose(1, 2).contiguous()
    core = lambda: ((q @ k.transpose(-2, -1)) * dh ** -0.5).softmax(dim=-1) @ v      # noqa: E731
    y = core()
    gq, gk, gv = torch.autograd.grad(y, (q, k, v), g, retain_graph=True)
    rel = lambda a, b: float((a - b).norm() / b.norm())      # noqa: E731
    split = lambda t, i: t.reshape(S, T, 3, H, dh)[:, :, i].transpose(1, 2)      # noqa: E731
    agree = {"out": rel(out.reshape(S, T, H, dh).transpose(1, 2), y.detach()), "dq": rel(split(dqkv, 0), gq), "dk": rel(split(dqkv, 1), gk),
             "dv": rel(split(dqkv, 2), gv)}
    assert max(agree.values()) < 1e-4, agree
    with torch.no_grad():
        eager_f = timed(core, reps, WARM)
    eager_b = timed(lambda: torch.autograd.grad(y, (q, k, v), g, retain_graph=True), reps, WARM)
    row = {"shape": label, "frames": frames, "sequences": S, "T": T, "heads": H, "dh": dh, "sequences_per_workgroup": eng.tnt_attention_group(T, H, dh),
           "eager_agrees_to": agree}
    P = lambda t: t.data_ptr()      # noqa: E731
    capi, st, scale = eng.capi, eng.stream(), dh ** -0.5
    ff, fb = floors(frames, H, dh)
    for name, fn, bfl, eg in (("forward", lambda: capi.i2v_tnt_attention_f32(P(qkv), S, T, H, dh, scale, P(out), st), ff, eager_f),
                              ("input_gradient", lambda: capi.i2v_tnt_attention_bwd_f32(P(qkv), P(dout), S, T, H, dh, scale, P(dqkv), st), fb, eager_b)):
        ms, lo, hi = timed(fn, reps, WARM)
        row[name] = {"call_ms": round(ms, 4), "fastest_slowest_ms": [round(lo, 4), round(hi, 4)], "byte_floor_ms": round(bfl, 4),
                     "share_of_floor": round(bfl / ms, 3), "eager_ms": round(eg[0], 4), "eager_fastest_slowest_ms": [round(eg[1], 4), round(eg[2], 4)],
                     "eager_over_kernel": round(eg[0] / ms, 2)}
    print(json.dumps(row), flush=True)


def stats(path, frames, reps):
    """The profiler's kernel stats of one `run --shape all`: the two TNT kernels per head width, and everything else (eager's kernels and
    the input generators) summed per timed call."""
    rows = kernel_rows(path)
    ours, rest = {}, 0.0
    for name, calls, total in rows:
        if "tnt_attn" in name:
            ours[name] = (calls, total / calls / 1e6)
        else:
            rest += total
    for label, (H, dh) in SHAPES.items():
        ff, fb = floors(frames, H, dh)
        for kind, floor in (("tnt_attn_kernel", ff), ("tnt_attn_bwd_kernel", fb)):
            for name, (calls, ms) in ours.items():
                if kind + f"ILi{dh}E" in name.replace(" ", "") or (kind + "<" + str(dh) + ">") in name:
                    print(json.dumps({"shape": label, "kernel": kind, "calls": calls, "kernel_ms": round(ms, 4), "byte_floor_ms": round(floor, 4),
                                      "share_of_floor": round(floor / ms, 3)}))
    print(json.dumps({"other_kernels_total_ms": round(rest / 1e6, 3), "note": "eager's kernels and the input generators, all calls"}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=("run", "stats"))
    ap.add_argument("path", nargs="?")
    ap.add_argument("--frames", type=int, default=128)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--shape", choices=sorted(SHAPES) + ["all"], default="all")
    a = ap.parse_args()
    if a.mode == "stats":
        return stats(a.path, a.frames, a.reps)
    for label in (SHAPES if a.shape == "all" else [a.shape]):
        one(label, a.frames, a.reps)


if __name__ == "__main__":
    main()
