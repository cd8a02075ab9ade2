"""TEST INFRASTRUCTURE: writes the committed fixture of the non-local-block launch tests.
  tests/golden/nl_fp32_cpu_errors.json   per case of tests/nl_cases.py and per `tensor` output: the error of the case's reference
                                         evaluated in float32 by plain torch on the CPU against its float64 evaluation, normalised as
                                         the output's bound is (`nl_cases.error`).  The device and host-simulation tests derive their
                                         bound from it: max(floor, 4 * this); nothing in it comes from the code under test.
Run from the repository root: python tests/make_nl_fixtures.py"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, os.path.join(ROOT, "image-to-video-i2v-attack_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)
ERRS = os.path.join(HERE, "golden", "nl_fp32_cpu_errors.json")


def compute():
    import torch
    from tests import nl_cases as nc
    torch.set_num_threads(1)            # one thread: torch's float32 reductions then split the same way on every host
    return {c.id: {k: float("%.3g" % v) for k, v in nc.fp32_errors(c).items()} for c in nc.CASES}


def load():
    with open(ERRS) as f:
        return json.load(f)


if __name__ == "__main__":
    doc = compute()
    with open(ERRS, "w") as f:
        f.write("{\n" + ",\n".join(json.dumps(k) + ": " + json.dumps(v) for k, v in doc.items()) + "\n}\n")
    print(ERRS, os.path.getsize(ERRS), "bytes,", len(doc), "cases")
