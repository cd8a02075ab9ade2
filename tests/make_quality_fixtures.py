"""Writes tests/golden/quality_fp32_cpu_errors.json: per case of tests/quality_cases.CASES the error of the float32 CPU run of the
reference (`quality_cases.reference(..., dtype=torch.float32)`) against its float64 run -- `ssim`: the largest absolute error of a
frame's SSIM; `sse`: the largest relative error of a frame's SSE (0 where the SSE is 0).  The tests bound the device and its host twin
by max(2e-6, 4 x that error).  Run from the repository root: `python -m tests.make_quality_fixtures`."""
import json

import torch

from tests import quality_cases as qc


def errors(case):
    a, b = qc.operands(case)
    want, got = qc.reference(case, a, b), qc.reference(case, a, b, dtype=torch.float32)
    sse = want[:, 0]
    rel = torch.where(sse > 0, (got[:, 0] - sse).abs() / sse.clamp_min(1e-300), torch.zeros_like(sse))
    return {"ssim": float((got[:, 2] - want[:, 2]).abs().max()), "sse": float(rel.max())}


def main():
    torch.set_num_threads(1)
    out = {c.name: errors(c) for c in qc.CASES}
    with open(qc.FP32_PATH, "w") as fh:
        json.dump(out, fh, indent=1, sort_keys=True)
        fh.write("\n")
    for k, v in out.items():
        print(k, v)


if __name__ == "__main__":
    main()
