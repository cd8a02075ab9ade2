"""Writes swin_fp32_cpu_errors.json: the relative L2 error of an fp32 CPU run of the Swin restatement (tests/swin_reference.py) against
its float64 run, on the inputs of tests/test_gpu_swin.py's full-size test (2 frames, synthetic weights of seed 0, hooks d = 1..4 and the
input gradient with all four hook gradients flowing).  The GPU test's bounds are the larger of the ViT bounds and 4 x these figures.
Run from the repository root: python tests/golden/make_swin_fp32_cpu_errors.py"""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "image-to-video-i2v-attack_amd")]
from i2v_amd import graphs, weights                     # noqa: E402
from tests.swin_reference import SwinReference          # noqa: E402

NAMES = ("swin_tiny_patch4_window7_224", "swin_base_patch4_window7_224")


def rand(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


def rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def main():
    out = {}
    for name in NAMES:
        spec = graphs.build(name)
        sd = weights.synthetic_state_dict(spec, 0)
        x = rand(2, 3, 224, 224, seed=22)
        stages = [spec.hook_for(d) for d in (1, 2, 3, 4)]
        hg = [rand(2, spec.hook_dim(s), seed=30 + i) for i, s in enumerate(stages)]
        r64, r32 = SwinReference(spec, sd, stages, torch.float64), SwinReference(spec, sd, stages, torch.float32)
        f64, f32 = r64.forward(x), r32.forward(x)
        g64, g32 = r64.backward(hg), r32.backward(hg)
        out[name] = {"hooks": [rel(a, b) for a, b in zip(f32, f64)], "grad": rel(g32, g64),
                     "hook_std": [float(f.std()) for f in f64]}
        print(name, out[name], flush=True)
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "swin_fp32_cpu_errors.json"), "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
