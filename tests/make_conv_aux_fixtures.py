"""TEST INFRASTRUCTURE: writes the committed fixture of the grouped / depthwise / squeeze-and-excitation kernel tests.
  tests/golden/conv_aux_fp32_cpu_errors.json   per case of tests/conv_aux_cases.py and per value output (convolutions: y, dx; SE: m, h,
                                               s, y, t, dmh, dx): the error of the case's reference evaluated in float32 on the CPU against
                                               its float64 evaluation, measured as the output's bound is (`conv_aux_cases.error`: the
                                               worst (frame, channel) plane).  Convolutions: the larger of plain float32 torch and the
                                               float32 fma chain of csrc/i2v_params.h on the operands of the library's own packers (the
                                               host simulation exports them).  The tests derive their bounds from it: max(floor, 4 *
                                               this); nothing in it comes from the code under test.
Run from the repository root: python tests/make_conv_aux_fixtures.py"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, os.path.join(ROOT, "image-to-video-i2v-attack_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)
ERRS = os.path.join(HERE, "golden", "conv_aux_fp32_cpu_errors.json")


def compute(ids=None):
    import torch
    from tests import conv_aux_cases as cc
    threads = torch.get_num_threads()
    torch.set_num_threads(1)            # one thread: torch's float32 reductions then split the same way on every host
    try:
        return {c.id: {k: float("%.3g" % v) for k, v in cc.fp32_errors(c).items()} for c in cc.CASES if ids is None or c.id in ids}
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
