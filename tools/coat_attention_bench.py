"""The CoaT factorized attention launches and dwmix (csrc/i2v_coat.hip) on the stage shapes of coat_lite_tiny and coat_lite_small at 128
frames, forward and input gradient, next to two yardsticks (there is no composed route: the shared softmax is row-wise):

  * eager PyTorch on the same GPU and tensors: the core of tests/coat_reference.py (`factor_core`: softmax of k over the tokens,
    Ks^T v, q G, q o E) in float32 and its autograd backward to qkv and E; for dwmix `coat_reference.crpe` (three grouped conv2d calls on
    a channel-major copy of v) and its autograd backward;
  * the byte floor at 4.7 TB/s: forward k and v read by the reduce, q and E read and out written by the apply (G and the statistics are
    small); backward q and dout read by the reduce, qkv, E and dout read and dqkv and dE written by the apply.  dwmix: v read, E written.

    python tools/coat_attention_bench.py [--frames 128] [--reps 30] [--shape t0|t1|t2|t3|s2|s3|all]

Times CALLS: one HIP event pair around each side's calls (the ctypes calls and their launches; outputs are made before), the median of
`reps` warm calls after 5 warm-up calls, with the fastest and slowest call as the spread.  A direction's two launches (reduce, apply)
are timed together, as the entry runs them.  Prints one JSON line per shape."""
import argparse
import json

from bench_util import timed
#: label -> (grid, heads, dh): the four stages of coat_lite_tiny, and stages 2 and 3 of coat_lite_mini / coat_lite_small
SHAPES = {"t0": (56, 8, 8), "t1": (28, 8, 16), "t2": (14, 8, 32), "t3": (7, 8, 40), "s2": (14, 8, 40), "s3": (7, 8, 64)}
FLOOR_TBS = 4.7


def one(label, Fr, reps):
    import torch
    from i2v_amd import attacks
    from tests import coat_reference as cr
    g, H, dh = SHAPES[label]
    T, Cn = 1 + g * g, H * dh
    eng = attacks.get_engine("cuda:0")
    gen = torch.Generator().manual_seed(T * 100 + dh)
    qkv = torch.randn(Fr, T, 3 * Cn, generator=gen).cuda()
    dout = torch.randn(Fr, T, Cn, generator=gen).cuda()
    n = [w * dh for w in (2, 3, 3)]
    filt = [(torch.randn(n[i], 1, K, K, generator=gen) / K).cuda() for i, K in enumerate((3, 5, 7))]
    bias = [0.02 * torch.randn(n[i], generator=gen).cuda() for i in range(3)]
    packed = tuple(w.reshape(-1, w.shape[-1] ** 2).t().contiguous() for w in filt)
    bcat = torch.cat(bias).contiguous()
    E = eng.coat_dwmix(qkv, packed, bcat, g, 1, False, 2 * Cn, Cn)
    out, gram, kstat = eng.coat_attention(qkv, E, H)
    dqkv, dE = eng.coat_attention_bwd(qkv, E, gram, kstat, dout, H)
    torch.cuda.synchronize()
    # the eager core on the same tensors; checked to agree first
    xr, Er = qkv.clone().requires_grad_(True), E.clone().requires_grad_(True)
    y = cr.factor_core(xr, Er, H)
    gq, gE = torch.autograd.grad(y, (xr, Er), dout, retain_graph=True)
    rel = lambda a, b: float((a - b).norm() / b.norm())      # noqa: E731
    vr = qkv[:, :, 2 * Cn:].clone().requires_grad_(True)
    agree = {"out": rel(out, y.detach()), "dq": rel(dqkv[:, :, :Cn], gq[:, :, :Cn]), "dv": rel(dqkv[:, :, 2 * Cn:], gq[:, :, 2 * Cn:]), "dE": rel(dE, gE)}
    assert max(agree.values()) < 1e-4, agree
    with torch.no_grad():
        eager_f = timed(lambda: cr.factor_core(xr, Er, H), reps, 5)
    eager_b = timed(lambda: torch.autograd.grad(y, (xr, Er), dout, retain_graph=True), reps, 5)
    del y

    def crpe_eager(v):
        plane = v[:, 1:].transpose(1, 2).reshape(Fr, Cn, g, g)
        parts, at = [], 0
        for w, b in zip(filt, bias):
            parts.append(torch.nn.functional.conv2d(plane[:, at:at + w.shape[0]], w, b, padding=w.shape[-1] // 2, groups=w.shape[0]))
            at += w.shape[0]
        return torch.cat(parts, dim=1).flatten(2).transpose(1, 2)
    with torch.no_grad():
        eager_dw = timed(lambda: crpe_eager(vr), reps, 5)
    ye = crpe_eager(vr)
    eager_dwb = timed(lambda: torch.autograd.grad(ye, vr, dout[:, 1:], retain_graph=True), reps, 5)
    del ye
    row = {"shape": label, "frames": Fr, "T": T, "heads": H, "dh": dh, "eager_agrees_to": agree}
    qs, os_ = Fr * T * 3 * Cn, Fr * T * Cn
    P = lambda t: t.data_ptr()      # noqa: E731
    capi, st, scale = eng.capi, eng.stream(), dh ** -0.5
    dgram = torch.empty_like(gram)
    cases = (("forward", lambda: capi.i2v_coat_factor_attention_f32(P(qkv), P(E), Fr, T, H, dh, scale, P(gram), P(kstat), P(out), st),
              qs + 2 * os_, eager_f),
             ("input_gradient", lambda: capi.i2v_coat_factor_attention_bwd_f32(P(qkv), P(E), P(gram), P(kstat), P(dout), Fr, T, H, dh, scale,
                                                                                P(dgram), P(dqkv), P(dE), st),
              (qs // 3 + os_) + (qs + 2 * os_) + (qs + os_), eager_b),
             ("dwmix", lambda: eng.coat_dwmix(qkv, packed, bcat, g, 1, False, 2 * Cn, Cn), 2 * os_, eager_dw),
             ("dwmix_input_gradient", lambda: eng.coat_dwmix(dE, packed, None, g, 1, False, bwd=True, into=dqkv, into_col=2 * Cn), 3 * os_, eager_dwb))
    for name, fn, floats, eg in cases:
        ms, lo, hi = timed(fn, reps, 5)
        bfl = floats * 4 / (FLOOR_TBS * 1e12) * 1e3
        row[name] = {"call_ms": round(ms, 4), "fastest_slowest_ms": [round(lo, 4), round(hi, 4)], "byte_floor_ms": round(bfl, 4),
                     "share_of_floor": round(bfl / ms, 3), "eager_ms": round(eg[0], 4), "eager_fastest_slowest_ms": [round(eg[1], 4), round(eg[2], 4)],
                     "eager_over_kernel": round(eg[0] / ms, 2)}
    print(json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=128)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--shape", choices=sorted(SHAPES) + ["all"], default="all")
    a = ap.parse_args()
    for label in (SHAPES if a.shape == "all" else [a.shape]):
        one(label, a.frames, a.reps)


if __name__ == "__main__":
    main()
