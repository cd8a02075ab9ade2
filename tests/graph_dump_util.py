"""TEST INFRASTRUCTURE: a graph of `i2v_amd.graphs` as plain lists, for node-for-node comparisons against a committed dump
(`tests/golden/cnn_graphs_before_resnet_family.json`: the seven CNN names as they were built before the ResNet family was added)."""
import dataclasses
import hashlib
import json
import os

EXISTING_NAMES = ("resnet", "resnet50", "vgg", "alexnet", "squeezenet", "densenet121", "densenet161")
DUMP_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cnn_graphs_before_resnet_family.json")
#: fields added to the IR after the dump was taken; a graph of an existing name must hold their defaults
NEW_FIELDS = {"groups": 1}


def graph_dump(g) -> dict:
    """One 10-hex-digit SHA-256 prefix per node and per tensor, over every field of the dataclass by name (a difference is located
    node for node; the full rows of seven nets would be 300 KB of fixture), the rest literally."""
    def row(obj):
        text = json.dumps([type(obj).__name__] + [[f.name, getattr(obj, f.name)] for f in dataclasses.fields(obj) if f.name not in NEW_FIELDS])
        return hashlib.sha256(text.encode()).hexdigest()[:10]
    return json.loads(json.dumps({
        "arch": g.arch, "in_hw": list(g.in_hw), "buffers": list(g.buffers), "input": g.input, "video": g.video,
        "tensors": " ".join(row(t) for t in g.tensors), "nodes": " ".join(row(nd) for nd in g.nodes),
        "hooks": sorted(g.hooks.items()), "hooks_module": sorted(g.hooks_module.items()),
    }))


def dump_all() -> dict:
    from i2v_amd import graphs
    out = {}
    for name in EXISTING_NAMES:
        out[name] = graph_dump(graphs.build(name, (224, 224)))
        out["tiny:" + name] = graph_dump(graphs.build_tiny(name, (64, 64)))
    return out


if __name__ == "__main__":          # python tests/graph_dump_util.py  (run on the commit whose graphs are to be pinned)
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "image-to-video-i2v-attack_amd"))
    with open(DUMP_PATH, "w") as f:
        f.write("{\n" + ",\n".join(json.dumps(k) + ":" + json.dumps(v, separators=(",", ":")) for k, v in dump_all().items()) + "\n}\n")
    print(DUMP_PATH, os.path.getsize(DUMP_PATH))
