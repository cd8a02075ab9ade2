"""TEST INFRASTRUCTURE: writes the two committed fixtures of the MNASNet tests.
  tests/golden/torchvision_mnasnet_keys.json   state_dict key -> shape of the four names up to `layers.13`, from torchvision 0.10.1's
                                               RULE restated below (not from i2v_amd.graphs): convolution weights with their shapes,
                                               BatchNorms as prefix -> channels (`expand_keys` reads it back)
  tests/golden/mnasnet_fp32_cpu_errors.json    relative L2 error of the float32 CPU run of tests/mnasnet_reference.py against its
                                               float64 run, per case: what the device tests derive their bound from
Run from the repository root: python tests/make_mnasnet_fixtures.py [keys|errors]"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, os.path.join(ROOT, "image-to-video-i2v-attack_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)
KEYS = os.path.join(HERE, "golden", "torchvision_mnasnet_keys.json")
ERRS = os.path.join(HERE, "golden", "mnasnet_fp32_cpu_errors.json")

#: torchvision.models.mnasnet: name -> alpha
TV = {"mnasnet0_5": 0.5, "mnasnet0_75": 0.75, "mnasnet1_0": 1.0, "mnasnet1_3": 1.3}
#: `MNASNet.__init__`: the `_stack(in, out, kernel, stride, expansion, repeats)` calls of layers.8 .. layers.13
STACKS = ((3, 2, 3, 3), (5, 2, 3, 3), (5, 2, 6, 3), (3, 1, 6, 2), (5, 2, 6, 4), (3, 1, 6, 1))


def round_to_multiple_of(val, divisor, round_up_bias=0.9):
    """torchvision's `_round_to_multiple_of`."""
    assert 0.0 < round_up_bias < 1.0
    new_val = max(divisor, int(val + divisor / 2) // divisor * divisor)
    return new_val if new_val >= round_up_bias * val else new_val + divisor


def depths_of(alpha):
    """`_get_depths` (`_version` 2: the stem widths scale with alpha too)."""
    return [round_to_multiple_of(d * alpha, 8) for d in (32, 16, 24, 40, 80, 96, 192, 320)]


def torchvision_layers(alpha):
    """Every convolution up to layers.13 as (weight key, BatchNorm prefix, cout, cin per group, k, stride, relu, adds the identity)."""
    d = depths_of(alpha)
    out = [("layers.0.weight", "layers.1", d[0], 3, 3, 2, True, False),
           ("layers.3.weight", "layers.4", d[0], 1, 3, 1, True, False),
           ("layers.6.weight", "layers.7", d[1], d[0], 1, 1, False, False)]
    cin = d[1]
    for si, (k, stride, exp, repeats) in enumerate(STACKS):
        cout = d[si + 2]
        for b in range(repeats):
            s = stride if b == 0 else 1
            mid, p = cin * exp, f"layers.{si + 8}.{b}.layers"
            out += [(f"{p}.0.weight", f"{p}.1", mid, cin, 1, 1, True, False),
                    (f"{p}.3.weight", f"{p}.4", mid, 1, k, s, True, False),
                    (f"{p}.6.weight", f"{p}.7", cout, mid, 1, 1, False, cin == cout and s == 1)]
            cin = cout
    return out


def torchvision_keys(alpha):
    out = {}
    for key, bn, cout, cing, k, _, _, _ in torchvision_layers(alpha):
        out[key] = [cout, cing, k, k]
        for s in ("weight", "bias", "running_mean", "running_var"):
            out[f"{bn}.{s}"] = [cout]
    return out


def compact_keys(alpha):
    lay = torchvision_layers(alpha)
    return {"convs": {l[0]: [l[2], l[3], l[4], l[4]] for l in lay}, "bns": {l[1]: l[2] for l in lay}}


def expand_keys(doc):
    out = {k: list(v) for k, v in doc["convs"].items()}
    for prefix, c in doc["bns"].items():
        for s in ("weight", "bias", "running_mean", "running_var"):
            out[f"{prefix}.{s}"] = [c]
    return out


def reference_macs(alpha, hw=224):
    """Multiply-adds per frame up to layers.13 from the same rule: a depthwise layer costs C k k Ho Wo."""
    total, size = 0, hw
    for _, _, cout, cing, k, s, _, _ in torchvision_layers(alpha):
        size = (size + 2 * (k // 2) - k) // s + 1
        total += size * size * cout * cing * k * k
    return total


def hook_shapes(alpha, hw=224):
    """depth -> (C, H, W) of layers.8 / .9 / .11 / .13."""
    d = depths_of(alpha)
    out, size = {}, (hw + 2 - 3) // 2 + 1
    for si, (k, stride, _, _) in enumerate(STACKS):
        size = (size + 2 * (k // 2) - k) // stride + 1
        if si + 8 in (8, 9, 11, 13):
            out[{8: 1, 9: 2, 11: 3, 13: 4}[si + 8]] = (d[si + 2], size, size)
    return out


def write_keys():
    try:                                    # checked once against torchvision itself where it imports; the tests do not depend on it
        import torchvision
        for name, alpha in TV.items():
            sd = getattr(torchvision.models, name)().state_dict()
            want = torchvision_keys(alpha)
            for k, shp in want.items():
                assert list(sd[k].shape) == shp, (name, k, tuple(sd[k].shape), shp)
            extra = [k for k in sd if k not in want and not k.endswith("num_batches_tracked") and not k.startswith(("layers.14", "layers.15", "classifier."))]
            assert not extra, (name, extra[:3])
        print("checked against torchvision", torchvision.__version__)
    except ImportError:
        print("torchvision does not import here: the rule above is unchecked against it")
    doc = {name: compact_keys(alpha) for name, alpha in TV.items()}
    for name, alpha in TV.items():
        assert expand_keys(doc[name]) == torchvision_keys(alpha), name
    with open(KEYS, "w") as f:
        f.write("{\n" + ",\n".join(json.dumps(k) + ":" + json.dumps(v, separators=(",", ":")) for k, v in doc.items()) + "\n}\n")
    print(KEYS, os.path.getsize(KEYS))


#: the whole-net cases of the device tests: tag -> (builder name, tiny, frame size, frames)
NET_CASES = {"mnasnet_tiny": ("mnasnet_tiny", True, 64, 3), "mnasnet1_0": ("mnasnet1_0", False, 224, 2), "mnasnet0_5": ("mnasnet0_5", False, 224, 2)}


def write_errors():
    import torch
    from i2v_amd import graphs, weights
    from tests import mnasnet_reference as mr
    torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))
    doc = {}
    for case in mr.NODE_CASES:
        C, k, plane, stride, frames = case
        g = mr.node_alone_graph(C, k, plane, stride)
        sd = weights.synthetic_state_dict(g, 7)
        x, hg = mr.case_inputs(mr.case_id(case), g, frames, [g.hooks[1]])
        doc[mr.case_id(case)] = mr.fp32_cpu_errors(g, sd, [g.hooks[1]], x, hg)[0]
        print(mr.case_id(case), doc[mr.case_id(case)], flush=True)
    for tag, (name, tiny, hw, frames) in NET_CASES.items():
        g = (graphs.build_tiny if tiny else graphs.build)(name, (hw, hw))
        hooks = [g.hooks[d] for d in (1, 2, 3, 4)]
        sd = weights.synthetic_state_dict(g, 7)
        x, hg = mr.case_inputs(tag, g, frames, hooks)
        doc[tag] = mr.fp32_cpu_errors(g, sd, hooks, x, hg)[0]
        print(tag, doc[tag], flush=True)
    with open(ERRS, "w") as f:
        f.write("{\n" + ",\n".join(json.dumps(k) + ": " + json.dumps(v) for k, v in doc.items()) + "\n}\n")


if __name__ == "__main__":
    what = sys.argv[1:] or ["keys", "errors"]
    if "keys" in what:
        write_keys()
    if "errors" in what:
        write_errors()
