"""TEST INFRASTRUCTURE: writes the committed fixture of the talking-heads / gated positional attention edge tests.
  tests/golden/attn_edge_fp32_cpu_errors.json   per attention case of tests/attn_edge_cases.py and per output (probs, out, dq, dk, dv):
                                                e32, the larger of two errors against the float64 reference, both measured as the
                                                output's bound is (`attn_edge_cases.error`: the worst slice, normalised by its (frame,
                                                head) plane) -- the reference evaluated in float32 by plain torch on the CPU, and the
                                                scalar host twin (csrc/i2v_cait_host.h, csrc/i2v_convit_host.h) through the host
                                                simulation.  The tests derive their bound from it: max(floor, 4 * this); nothing in it
                                                comes from the device.
Run from the repository root: python tests/make_attn_edge_fixtures.py"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, os.path.join(ROOT, "image-to-video-i2v-attack_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)
ERRS = os.path.join(HERE, "golden", "attn_edge_fp32_cpu_errors.json")


def compute(ids=None, parts=False):
    """{case id: {output: e32}}; `parts`: {case id: {output: (float32 torch, host twin)}} instead."""
    import torch
    from tests import attn_edge_cases as ac
    from tests.hostsim_util import hostsim_engine
    eng = hostsim_engine()
    threads = torch.get_num_threads()
    torch.set_num_threads(1)            # one thread: torch's float32 reductions then split the same way on every host
    try:
        out = {}
        for c in ac.ATTN_CASES:
            if ids is not None and c.id not in ids:
                continue
            t32, twin, ref = ac.fp32_errors(c), ac.run(eng, c), ac.reference(c)
            both = {k: (v, ac.error(twin[k], ref[k][1])) for k, v in t32.items()}
            out[c.id] = both if parts else {k: float("%.3g" % max(v)) for k, v in both.items()}
        return out
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
