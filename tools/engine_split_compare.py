#!/usr/bin/env python3
"""Developer tool: is a rebuilt engine (csrc/i2v_engine.cpp and its sibling units) the same engine?  Three subcommands.

    I2V_AUTOTUNE=0 I2V_LIB=<library> python tools/engine_split_compare.py plan OUT.json
        plans the headline ResNet-101 net (depth 3, 128 frames) and the SlowFast ILAF net (one 32-frame clip), runs one forward +
        backward in timing mode 1 and records workspace_bytes(), fusion_info() and every I2V_TIMING_DUMP line without its ms column
        (kind Cd K HWg frames pw, GFLOP, MB).  I2V_AUTOTUNE=0 makes the plan deterministic.  With a third argument, the path of a
        host-simulation library (tests/hostsim/libi2v_hostsim.so), the same on the CPU with the tiny graphs of the tests.
    python tools/engine_split_compare.py diff A.json B.json
        the two records must be identical; exit status 1 and the first differences otherwise.
    python tools/engine_split_compare.py npy DIR_A DIR_B
        two `bench.py --dump-outputs` directories: every array named in the manifests must be equal (numpy.array_equal)."""
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "image-to-video-i2v-attack_amd"), ROOT]


def plan(out_path, hostsim=None):
    import torch
    from i2v_amd import graphs, lib, weights
    from i2v_amd.engine import Engine
    if hostsim:
        import ctypes
        eng, dev = Engine("cpu", capi=lib.bind(ctypes.CDLL(hostsim))), "cpu"
        g_img, g_vid = graphs.build_tiny("resnet", (64, 64)), graphs.build_video_tiny("slowfast_resnet50")
        nets = {"tiny_resnet_depth3_8": (g_img, [g_img.hooks[3]], 8, (8, 3, 64, 64)),
                "tiny_slowfast_ilaf_8": (g_vid, graphs.video_hooks(g_vid, "slowfast_resnet50"), 8, (8, 3, 32, 32))}
    else:
        eng, dev = Engine("cuda:0"), "cuda"
        g_img, g_vid = graphs.build("resnet"), graphs.build_video("slowfast_resnet50")
        nets = {"resnet101_depth3_128": (g_img, [g_img.hooks[3]], 128, (128, 3, 224, 224)),
                "slowfast_ilaf_32": (g_vid, graphs.video_hooks(g_vid, "slowfast_resnet50"), 32, (32, 3, 224, 224))}
    record = {}
    for name, (g, hooks, frames, shape) in nets.items():
        net = eng.build_net(g, weights.synthetic_state_dict(g, 0), hooks, frames)
        x = torch.randn(*shape, generator=torch.Generator().manual_seed(0)).to(dev)
        gx = torch.zeros_like(x)
        with tempfile.TemporaryDirectory() as tmp:
            os.environ["I2V_TIMING_DUMP"] = dump = os.path.join(tmp, "dump.txt")
            eng.timing_enable(1)
            net.forward(x)
            net.backward(gx)
            kinds = eng.timing_collect()
            eng.timing_enable(False)
            lines = [ln.split() for ln in open(dump)]
        record[name] = {"workspace_bytes": net.workspace_bytes(), "fusion_info": net.fusion_info(), "dump_lines": len(lines),
                        "launches": [ln[:6] + ln[7:] for ln in lines],          # without the ms column
                        "by_kind": {k: {f: v[f] for f in ("flops", "launches", "bytes", "lowi_bytes", "lowi_launches", "lowi_flops")}
                                    for k, v in kinds.items()}}
        net.close()
    with open(out_path, "w") as fh:
        json.dump(record, fh, indent=1)
    print({k: (v["workspace_bytes"], v["fusion_info"], v["dump_lines"]) for k, v in record.items()})


def diff(a_path, b_path):
    a, b = json.load(open(a_path)), json.load(open(b_path))
    bad = 0
    for name in sorted(set(a) | set(b)):
        ra, rb = a.get(name, {}), b.get(name, {})
        for key in sorted(set(ra) | set(rb)):
            if ra.get(key) != rb.get(key):
                bad += 1
                print(f"DIFFERENT {name}.{key}")
                if key == "launches":
                    for i, (la, lb) in enumerate(zip(ra[key], rb[key])):
                        if la != lb:
                            print(f"  line {i}: {la} != {lb}")
                            break
        print(f"{name}: workspace {ra.get('workspace_bytes')} fusion {ra.get('fusion_info')} dump lines {ra.get('dump_lines')}")
    print("plans identical" if not bad else f"{bad} differences")
    return 1 if bad else 0


def npy(dir_a, dir_b):
    import numpy as np
    ma, mb = json.load(open(os.path.join(dir_a, "manifest.json"))), json.load(open(os.path.join(dir_b, "manifest.json")))
    bad = 0 if ma == mb else 1
    if bad:
        print("manifests differ")
    for name in sorted(set(ma) & set(mb)):
        same = np.array_equal(np.load(os.path.join(dir_a, name + ".npy")), np.load(os.path.join(dir_b, name + ".npy")))
        bad += 0 if same else 1
        print(f"{name}: {'equal' if same else 'DIFFERENT'}")
    print(f"{len(ma)} arrays, {'all equal' if not bad else str(bad) + ' problems'}: {dir_a} vs {dir_b}")
    return 1 if bad else 0


if __name__ == "__main__":
    cmd, args = sys.argv[1], sys.argv[2:]
    sys.exit({"plan": plan, "diff": diff, "npy": npy}[cmd](*args) or 0)
