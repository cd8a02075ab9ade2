"""TEST INFRASTRUCTURE: writes the committed fixture of the window-attention kernel tests.
  tests/golden/swin_kernel_fp32_cpu_errors.json   per window case of tests/swin_cases.py and per output (out, dq, dk, dv): the error of
                                                  the case's reference evaluated in float32 by plain torch on the CPU against its
                                                  float64 evaluation, measured as the output's bound is (`swin_cases.error`: the worst
                                                  (frame, window, head) block).  The device test derives its bound from it:
                                                  max(floor, 4 * this); nothing in it comes from the code under test.
Run from the repository root: python tests/make_swin_kernel_fixtures.py"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, os.path.join(ROOT, "image-to-video-i2v-attack_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)
ERRS = os.path.join(HERE, "golden", "swin_kernel_fp32_cpu_errors.json")


def compute(ids=None):
    import torch
    from tests import swin_cases as sc
    threads = torch.get_num_threads()
    torch.set_num_threads(1)            # one thread: torch's float32 reductions then split the same way on every host
    try:
        return {c.id: {k: float("%.3g" % v) for k, v in sc.fp32_errors(c).items()} for c in sc.WIN_CASES if ids is None or c.id in ids}
    finally:
        torch.set_num_threads(threads)


def load():
    with open(ERRS) as f:
        return json.load(f)


if __name__ == "__main__":
    doc = compute()
    with open(ERRS, "w") as f:
        f.write("{\n" + ",\n".join(json.dumps(k) + ": " + json.dumps(v) for k, v in doc.items()) + "\n}\n")
    print(ERRS, os.path.getsize(ERRS), "bytes,", len(doc), "cases")
