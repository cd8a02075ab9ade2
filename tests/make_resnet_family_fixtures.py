"""TEST INFRASTRUCTURE: writes the two committed fixtures of the ResNet-family tests.
  tests/golden/torchvision_resnet_family_keys.json   state_dict key -> shape of every new name, from torchvision's RULE restated below
                                                     (not from i2v_amd.graphs): names and shapes only, one entry per run of equal blocks
                                                     (`expand_keys` reads it back)
  tests/golden/resnet_family_fp32_cpu_errors.json    relative L2 error of the float32 CPU run of tests/resnet_family_reference.py against
                                                     its float64 run, per case: what the device tests derive their bound from
Run from the repository root: python tests/make_resnet_family_fixtures.py [keys|errors]"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, os.path.join(ROOT, "image-to-video-i2v-attack_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)
KEYS = os.path.join(HERE, "golden", "torchvision_resnet_family_keys.json")
ERRS = os.path.join(HERE, "golden", "resnet_family_fp32_cpu_errors.json")

#: torchvision.models.resnet: name -> (block, layers, groups, width_per_group)
TV = {"resnet18": ("BasicBlock", (2, 2, 2, 2), 1, 64), "resnet34": ("BasicBlock", (3, 4, 6, 3), 1, 64),
      "resnet152": ("Bottleneck", (3, 8, 36, 3), 1, 64), "wide_resnet50_2": ("Bottleneck", (3, 4, 6, 3), 1, 128),
      "wide_resnet101_2": ("Bottleneck", (3, 4, 23, 3), 1, 128), "resnext50_32x4d": ("Bottleneck", (3, 4, 6, 3), 32, 4),
      "resnext101_32x8d": ("Bottleneck", (3, 4, 23, 3), 32, 8)}


def torchvision_keys(block, layers, groups, width_per_group):
    """`ResNet.__init__` / `_make_layer` / the two block classes, as shapes: conv1, bn1, layer1..4 (fc is behind the last hook)."""
    out = {"conv1.weight": [64, 3, 7, 7]}

    def bn(prefix, c):
        for s in ("weight", "bias", "running_mean", "running_var"):
            out[f"{prefix}.{s}"] = [c]
    bn("bn1", 64)
    expansion = 4 if block == "Bottleneck" else 1
    inplanes = 64
    for li, blocks in enumerate(layers):
        planes, stride = 64 * 2 ** li, (1 if li == 0 else 2)
        for b in range(blocks):
            p, s = f"layer{li + 1}.{b}", (stride if b == 0 else 1)
            if block == "Bottleneck":
                width = int(planes * (width_per_group / 64.0)) * groups
                out[f"{p}.conv1.weight"] = [width, inplanes, 1, 1]
                bn(f"{p}.bn1", width)
                out[f"{p}.conv2.weight"] = [width, width // groups, 3, 3]
                bn(f"{p}.bn2", width)
                out[f"{p}.conv3.weight"] = [planes * 4, width, 1, 1]
                bn(f"{p}.bn3", planes * 4)
            else:
                out[f"{p}.conv1.weight"] = [planes, inplanes, 3, 3]
                bn(f"{p}.bn1", planes)
                out[f"{p}.conv2.weight"] = [planes, planes, 3, 3]
                bn(f"{p}.bn2", planes)
            if b == 0 and (s != 1 or inplanes != planes * expansion):
                out[f"{p}.downsample.0.weight"] = [planes * expansion, inplanes, 1, 1]
                bn(f"{p}.downsample.1", planes * expansion)
            inplanes = planes * expansion
    return out


def compact_keys(keys, layers):
    """The same names and shapes, written once per run of equal blocks: per stage the first block and, where there are more, the
    second (every later block of a torchvision stage has the second one's shapes; `expand_keys` asserts nothing, it only repeats).
    BatchNorm's four vectors are one entry, `<prefix>.*`."""
    def fold(d):
        out = {}
        for k, shp in d.items():
            if k.endswith(".running_var"):
                out[k[:-len("running_var")] + "*"] = shp
            elif not k.endswith((".running_mean", ".bias")) and not (k.endswith(".weight") and len(shp) == 1):
                out[k] = shp
        return out
    doc = {"stem": fold({k: v for k, v in keys.items() if not k.startswith("layer")}), "layers": []}
    for li, blocks in enumerate(layers):
        def block(b):
            p = f"layer{li + 1}.{b}."
            return fold({k[len(p):]: v for k, v in keys.items() if k.startswith(p)})
        doc["layers"].append({"blocks": blocks, "first": block(0), "rest": block(1) if blocks > 1 else {}})
    return doc


def expand_keys(doc):
    """The fixture's compact form back into state_dict key -> shape."""
    def unfold(prefix, d, out):
        for k, shp in d.items():
            if k.endswith(".*"):
                for s in ("weight", "bias", "running_mean", "running_var"):
                    out[prefix + k[:-1] + s] = shp
            else:
                out[prefix + k] = shp
    out = {}
    unfold("", doc["stem"], out)
    for li, layer in enumerate(doc["layers"]):
        for b in range(layer["blocks"]):
            unfold(f"layer{li + 1}.{b}.", layer["first"] if b == 0 else layer["rest"], out)
    return out


def reference_macs(block, layers, groups, width_per_group, hw=224):
    """Multiply-adds per frame up to layer4, from the same rule (stem 7x7 / 2 / pad 3, max-pool 3 / 2 / pad 1)."""
    keys = torchvision_keys(block, layers, groups, width_per_group)
    size = (hw + 6 - 7) // 2 + 1
    total = size * size * 64 * 3 * 49
    size = (size + 2 - 3) // 2 + 1
    for li, blocks in enumerate(layers):
        for b in range(blocks):
            p = f"layer{li + 1}.{b}"
            s = 2 if (li > 0 and b == 0) else 1
            out_size = (size + 2 - 3) // s + 1
            for name in ("conv1", "conv2", "conv3", "downsample.0"):
                k = f"{p}.{name}.weight"
                if k not in keys:
                    continue
                co, ci, kh, kw = keys[k]
                at_in = name == "conv1" and block == "Bottleneck"       # the bottleneck's conv1 runs before the stride
                total += (size if at_in else out_size) ** 2 * co * ci * kh * kw
            size = out_size
    return total


def write_keys():
    doc = {name: torchvision_keys(*spec) for name, spec in TV.items()}
    try:                                    # checked once against torchvision itself where it imports; the tests do not depend on it
        import torchvision
        for name in TV:
            sd = getattr(torchvision.models, name)().state_dict()
            for k, shp in doc[name].items():
                assert list(sd[k].shape) == shp, (name, k, tuple(sd[k].shape), shp)
            extra = [k for k in sd if k not in doc[name] and not k.endswith("num_batches_tracked") and not k.startswith("fc.")]
            assert not extra, (name, extra[:3])
        print("checked against torchvision", torchvision.__version__)
    except ImportError:
        print("torchvision does not import here: the rule above is unchecked against it")
    compact = {name: compact_keys(doc[name], TV[name][1]) for name in TV}
    for name in TV:
        assert expand_keys(compact[name]) == doc[name], name
    with open(KEYS, "w") as f:
        f.write("{\n" + ",\n".join(json.dumps(k) + ":" + json.dumps(v, separators=(",", ":")) for k, v in compact.items()) + "\n}\n")
    print(KEYS, os.path.getsize(KEYS))


def write_errors():
    import torch
    from i2v_amd import graphs, weights
    from tests import resnet_family_reference as rf
    torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))
    doc = {}
    for case in rf.NODE_CASES:
        C, groups, plane, stride, frames = case
        g = rf.node_alone_graph(C, groups, plane, stride)
        sd = weights.synthetic_state_dict(g, 7)
        x, hg = rf.case_inputs(rf.case_id(case), g, frames, [g.hooks[1]])
        doc[rf.case_id(case)] = rf.fp32_cpu_errors(g, sd, [g.hooks[1]], x, hg)[0]
        print(rf.case_id(case), doc[rf.case_id(case)], flush=True)
    for name, builder, hw, frames in (("resnext_tiny", graphs.build_tiny, 64, 3), ("resnet_basic_tiny", graphs.build_tiny, 64, 3),
                                      ("resnext50_32x4d", graphs.build, 224, 2), ("resnet18", graphs.build, 224, 2)):
        g = builder(name, (hw, hw))
        hooks = [g.hooks[d] for d in (1, 2, 3, 4)]
        sd = weights.synthetic_state_dict(g, 7)
        x, hg = rf.case_inputs(name, g, frames, hooks)
        doc[name] = rf.fp32_cpu_errors(g, sd, hooks, x, hg)[0]
        print(name, doc[name], flush=True)
    with open(ERRS, "w") as f:
        f.write("{\n" + ",\n".join(json.dumps(k) + ": " + json.dumps(v) for k, v in doc.items()) + "\n}\n")


if __name__ == "__main__":
    what = sys.argv[1:] or ["keys", "errors"]
    if "keys" in what:
        write_keys()
    if "errors" in what:
        write_errors()
