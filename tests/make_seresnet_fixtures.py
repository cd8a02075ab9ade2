"""TEST INFRASTRUCTURE: writes the two committed fixtures of the SE-ResNet tests.
  tests/golden/timm_seresnet_keys.json         state_dict key -> shape of the eight names up to `layer4`, from timm 0.5.0's RULE restated
                                               below (not from i2v_amd.graphs): convolution weights with their shapes, BatchNorms as
                                               prefix -> channels, SE modules as prefix -> (C, rd) (`expand_keys` reads it back)
  tests/golden/seresnet_fp32_cpu_errors.json   relative L2 error of the float32 CPU run of tests/seresnet_reference.py against its
                                               float64 run, per case: what the tests derive their bound from (never a device figure)
The rule is checked against timm wherever timm imports; where it does not, it is unchecked against it.
Run from the repository root: python tests/make_seresnet_fixtures.py [keys|errors]"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, os.path.join(ROOT, "image-to-video-i2v-attack_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)
KEYS = os.path.join(HERE, "golden", "timm_seresnet_keys.json")
ERRS = os.path.join(HERE, "golden", "seresnet_fp32_cpu_errors.json")

#: timm.models.resnet: name -> (block, layers, cardinality, base_width), all with block_args=dict(attn_layer='se')
TIMM = {"seresnet18": ("basic", (2, 2, 2, 2), 1, 64), "seresnet34": ("basic", (3, 4, 6, 3), 1, 64),
        "seresnet50": ("bottleneck", (3, 4, 6, 3), 1, 64), "seresnet101": ("bottleneck", (3, 4, 23, 3), 1, 64),
        "seresnet152": ("bottleneck", (3, 8, 36, 3), 1, 64), "seresnext50_32x4d": ("bottleneck", (3, 4, 6, 3), 32, 4),
        "seresnext101_32x4d": ("bottleneck", (3, 4, 23, 3), 32, 4), "seresnext101_32x8d": ("bottleneck", (3, 4, 23, 3), 32, 8)}


def make_divisible(v, divisor=8, min_value=None, round_limit=0.9):
    """timm's `make_divisible`."""
    min_value = min_value or divisor
    new_v = max(min_value, int(v + divisor / 2) // divisor * divisor)
    if new_v < round_limit * v:
        new_v += divisor
    return new_v


def se_rd(C):
    """`SEModule(C)`: rd_ratio 1/16, rd_divisor 8, `make_divisible(C * rd_ratio, rd_divisor, round_limit=0.)`."""
    return make_divisible(C / 16, 8, round_limit=0.0)


def timm_layers(name):
    """Every module up to layer4, in forward order: ("conv", weight key, BN prefix, cout, cin per group, k, stride, relu) and
    ("se", prefix, C, rd).  The stride sits on the 3x3 (conv2 of a bottleneck, conv1 of a basic block); the SE module follows the block's
    last BatchNorm; a projection shortcut `downsample.0 / .1` wherever the stride or the width changes."""
    block, layers, card, base = TIMM[name]
    exp = 4 if block == "bottleneck" else 1
    out = [("conv", "conv1.weight", "bn1", 64, 3, 7, 2, True)]
    inplanes = 64
    for li, nb in enumerate(layers):
        planes = 64 * 2 ** li
        for b in range(nb):
            s = 2 if (b == 0 and li > 0) else 1
            p = f"layer{li + 1}.{b}"
            if block == "bottleneck":
                w = int(planes * base / 64) * card
                out += [("conv", f"{p}.conv1.weight", f"{p}.bn1", w, inplanes, 1, 1, True),
                        ("conv", f"{p}.conv2.weight", f"{p}.bn2", w, w // card, 3, s, True),
                        ("conv", f"{p}.conv3.weight", f"{p}.bn3", planes * 4, w, 1, 1, False)]
            else:
                out += [("conv", f"{p}.conv1.weight", f"{p}.bn1", planes, inplanes, 3, s, True),
                        ("conv", f"{p}.conv2.weight", f"{p}.bn2", planes, planes, 3, 1, False)]
            out.append(("se", f"{p}.se", planes * exp, se_rd(planes * exp)))
            if s != 1 or inplanes != planes * exp:
                out.append(("conv", f"{p}.downsample.0.weight", f"{p}.downsample.1", planes * exp, inplanes, 1, s, False))
            inplanes = planes * exp
    return out


def timm_keys(name):
    out = {}
    for l in timm_layers(name):
        if l[0] == "conv":
            _, key, bn, cout, cing, k, _, _ = l
            out[key] = [cout, cing, k, k]
            for s in ("weight", "bias", "running_mean", "running_var"):
                out[f"{bn}.{s}"] = [cout]
        else:
            _, p, C, rd = l
            out[f"{p}.fc1.weight"], out[f"{p}.fc1.bias"] = [rd, C, 1, 1], [rd]
            out[f"{p}.fc2.weight"], out[f"{p}.fc2.bias"] = [C, rd, 1, 1], [C]
    return out


def compact_keys(name):
    lay = timm_layers(name)
    return {"convs": {l[1]: [l[3], l[4], l[5], l[5]] for l in lay if l[0] == "conv"}, "bns": {l[2]: l[3] for l in lay if l[0] == "conv"},
            "se": {l[1]: [l[2], l[3]] for l in lay if l[0] == "se"}}


def expand_keys(doc):
    out = {k: list(v) for k, v in doc["convs"].items()}
    for prefix, c in doc["bns"].items():
        for s in ("weight", "bias", "running_mean", "running_var"):
            out[f"{prefix}.{s}"] = [c]
    for p, (C, rd) in doc["se"].items():
        out[f"{p}.fc1.weight"], out[f"{p}.fc1.bias"] = [rd, C, 1, 1], [rd]
        out[f"{p}.fc2.weight"], out[f"{p}.fc2.bias"] = [C, rd, 1, 1], [C]
    return out


def _plane_after(size, k, s):
    return (size + 2 * (k // 2) - k) // s + 1


def reference_macs(name, hw=224):
    """Multiply-adds per frame up to layer4 from the same rule: convolutions by their real (grouped) products, an SE module 2 C rd."""
    block = TIMM[name][0]
    total = 0
    size = _plane_after(hw, 7, 2)
    total += size * size * 64 * 3 * 49
    size = _plane_after(size, 3, 2)                      # the 3x3 / 2 max-pool
    for l in timm_layers(name)[1:]:
        if l[0] == "se":
            total += 2 * l[2] * l[3]
            continue
        _, key, _, cout, cing, k, s, _ = l
        if "downsample" in key:                          # reads the block's input: the plane the block's strided 3x3 produced
            total += size * size * cout * cing
            continue
        strided = key.endswith("conv2.weight") if block == "bottleneck" else key.endswith("conv1.weight")
        if strided:
            size = _plane_after(size, k, s)
        total += size * size * cout * cing * k * k
    return total


def hook_shapes(name, hw=224):
    """depth -> (C, H, W) of layer{d}[-1]."""
    exp = 4 if TIMM[name][0] == "bottleneck" else 1
    size = _plane_after(_plane_after(hw, 7, 2), 3, 2)
    out = {}
    for d in (1, 2, 3, 4):
        if d > 1:
            size = _plane_after(size, 3, 2)
        out[d] = (64 * 2 ** (d - 1) * exp, size, size)
    return out


def write_keys():
    try:                                    # checked against timm itself where it imports; the tests do not depend on it
        import timm
        for name in TIMM:
            sd = timm.create_model(name, pretrained=False).state_dict()
            want = timm_keys(name)
            for k, shp in want.items():
                assert list(sd[k].shape) == shp, (name, k, tuple(sd[k].shape), shp)
            extra = [k for k in sd if k not in want and not k.endswith("num_batches_tracked") and not k.startswith("fc.")]
            assert not extra, (name, extra[:3])
        print("checked against timm", timm.__version__)
    except ImportError:
        print("timm does not import here: the rule above is unchecked against it")
    doc = {name: compact_keys(name) for name in TIMM}
    for name in TIMM:
        assert expand_keys(doc[name]) == timm_keys(name), name
    with open(KEYS, "w") as f:
        f.write("{\n" + ",\n".join(json.dumps(k) + ":" + json.dumps(v, separators=(",", ":")) for k, v in doc.items()) + "\n}\n")
    print(KEYS, os.path.getsize(KEYS))


#: the whole-net cases: tag -> (builder name, tiny, frame size, frames)
NET_CASES = {"seresnet_tiny": ("seresnet_tiny", True, 64, 3), "seresnext_tiny": ("seresnext_tiny", True, 64, 3),
             "seresnet50": ("seresnet50", False, 224, 2), "seresnext50_32x4d": ("seresnext50_32x4d", False, 224, 2)}


def node_case(case):
    """(tag, graph, weights, hooks, frames) of a node case."""
    from i2v_amd import weights
    from tests import seresnet_reference as sr
    C, rd, plane, residual, relu, frames = case
    g = sr.node_alone_graph(C, rd, plane, residual, relu)
    return sr.case_id(case), g, weights.synthetic_state_dict(g, 7), [g.hooks[1]], frames


def net_case(tag):
    from i2v_amd import graphs, weights
    name, tiny, hw, frames = NET_CASES[tag]
    g = (graphs.build_tiny if tiny else graphs.build)(name, (hw, hw))
    return tag, g, weights.synthetic_state_dict(g, 7), [g.hooks[d] for d in (1, 2, 3, 4)], frames


def write_errors():
    import torch
    from tests import seresnet_reference as sr
    torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))
    doc = {}
    for tag, g, sd, hooks, frames in [node_case(c) for c in sr.NODE_CASES] + [net_case(t) for t in NET_CASES]:
        x, hg = sr.case_inputs(tag, g, frames, hooks)
        doc[tag] = sr.fp32_cpu_errors(g, sd, hooks, x, hg)
        print(tag, doc[tag], flush=True)
    with open(ERRS, "w") as f:
        f.write("{\n" + ",\n".join(json.dumps(k) + ": " + json.dumps(v) for k, v in doc.items()) + "\n}\n")


if __name__ == "__main__":
    what = sys.argv[1:] or ["keys", "errors"]
    if "keys" in what:
        write_keys()
    if "errors" in what:
        write_errors()
