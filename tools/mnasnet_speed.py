"""Speed of a 10-step I2V attack at `--depth 3` on b x 32 x 224^2 clips for an MNASNet surrogate, in adversarial frames/s (the counterpart
of tools/resnext_speed.py).

    python tools/mnasnet_speed.py engine [--arch mnasnet1_0] [--clips 4] [--steps 10] [--reps 2]   # the product class on the HIP path
    python tools/mnasnet_speed.py eager  [--arch ...]                                                 # the same loop in eager PyTorch fp32
    python tools/mnasnet_speed.py shares KERNEL_STATS_CSV                                             # kernel-time shares from a profiler stats file

Run each side in a process of its own, under its own time limit.  Synthetic weights (seed 0); the first call of each side warms up and is
not timed; best of `--reps`.  Prints one JSON line.  `shares` reads the `kernel_stats.csv` of `rocprofv3 --kernel-trace --stats
--output-format csv -- python tools/mnasnet_speed.py engine` and groups the device time: depthwise conv (`dwconv_kernel`), the other
convolutions (`conv_*`), the rest."""
import argparse
import csv
import json
import os
import sys

import bench_util  # noqa: F401 (puts the repository on sys.path)
from family_speed import clips, eager_attack, time_calls

ARCHS = ("mnasnet1_0", "mnasnet0_5", "mnasnet0_75", "mnasnet1_3")


def shares(path):
    tot = {"depthwise conv": [0, 0], "other convolutions": [0, 0], "the rest": [0, 0]}
    for r in csv.DictReader(open(path)):
        fam = "depthwise conv" if "dwconv_kernel" in r["Name"] else "other convolutions" if "conv_" in r["Name"] else "the rest"
        tot[fam][0] += int(float(r["TotalDurationNs"]))
        tot[fam][1] += int(r["Calls"])
    whole = sum(v[0] for v in tot.values())
    print(json.dumps({"file": os.path.basename(path), "device_ms": round(whole / 1e6, 2),
                      "shares": {k: {"ms": round(v[0] / 1e6, 2), "launches": v[1], "share": round(v[0] / whole, 4)} for k, v in tot.items()}}))


def main():
    if len(sys.argv) == 3 and sys.argv[1] == "shares":
        return shares(sys.argv[2])
    import torch
    from i2v_amd import attacks, graphs, weights
    from tests.mnasnet_reference import FamilyRef
    ap = argparse.ArgumentParser()
    ap.add_argument("side", choices=("engine", "eager"))
    ap.add_argument("--arch", default="mnasnet1_0", choices=ARCHS)
    ap.add_argument("--depth", type=int, default=3)
    ap.add_argument("--clips", type=int, default=4)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--reps", type=int, default=2)
    a = ap.parse_args()
    vid = clips(a.clips, 32)
    if a.side == "engine":
        atk = attacks.ImageGuidedFMDirection_Adam([a.arch], depth=a.depth, step_size=0.005, steps=a.steps, weight_seed=0)
        labels, names = torch.zeros(a.clips, dtype=torch.long), [f"c{i}" for i in range(a.clips)]
        call = lambda: atk(vid, labels, names)                                                    # noqa: E731
    else:
        g = graphs.build(a.arch)
        ref = FamilyRef(g, weights.synthetic_state_dict(g, 0), [g.hooks[a.depth]], torch.float32)
        ref.sd = {k: v.cuda() for k, v in ref.sd.items()}
        vd = vid.cuda()
        call = lambda: eager_attack(vd, lambda t: ref.features(t)[0].reshape(t.shape[0], -1), a.steps)      # noqa: E731
    times = time_calls(call, a.reps)
    print(json.dumps({"side": a.side, "arch": a.arch, "depth": a.depth, "clips": a.clips, "frames": 32, "steps": a.steps,
                      "seconds": [round(t, 4) for t in times], "adv_frames_per_s": round(a.clips * 32 / min(times), 2)}))


if __name__ == "__main__":
    main()
