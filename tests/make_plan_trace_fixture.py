"""TEST INFRASTRUCTURE: writes tests/golden/plan_trace.txt, the planner's decisions over a fixed catalogue of graphs.
Every entry is planned on the host simulation in a child process with `I2V_FUSE_DEBUG=1`; the engine then prints one line per decision
(`[i2v fuse]`, `[i2v fastblock]`, `[i2v scpair]`, `[i2v overlap]`: list positions and shapes, no addresses).  The fixture keeps a
`== name size hooks` header per entry and those lines.  tests/test_plan_trace_cpu.py runs the same catalogue on the working tree and
compares line for line, so a change to the plan-time passes of csrc/i2v_tune.cpp that moves a decision shows up without a GPU.
The committed fixture was recorded with this script on the parent of the commit that rephrased those passes on one shared
read/write-set analysis (`access_of`): it is that older code's answer, and a re-recording needs the same care.
Run from the repository root: python tests/make_plan_trace_fixture.py"""
import json
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, os.path.join(ROOT, "image-to-video-i2v-attack_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)
FIXTURE = os.path.join(HERE, "golden", "plan_trace.txt")

#: every admissible group is admitted and forced, every launch that can be hoisted is, and nothing is timed
ENV = {"I2V_AUTOTUNE": "0", "I2V_FORCE_FUSE": "2", "I2V_FORCE_FASTBLOCK": "1", "I2V_OVERLAP_MAX_FRAMES": "1000", "I2V_FUSE_DEBUG": "1"}
OFF = {"I2V_FASTBLOCK": "0", "I2V_SCPAIR": "0"}
IMAGE = [("resnet50", 64), ("resnet50", 96), ("wide_resnet50_2", 64), ("resnext50_32x4d", 64), ("seresnet50", 64), ("densenet121", 64),
         ("squeezenet", 64), ("mnasnet1_0", 64)]
VIDEO = ["slowfast_resnet50", "i3d_resnet50", "tpn_resnet50"]
VIDEO_THW = (8, 32, 32)


def catalogue():
    """(kind, name, size, hooks, extra environment) per plan."""
    out = []
    for name, hw in IMAGE:
        out += [("image", name, hw, "deepest", {}), ("image", name, hw, "all", {})]
    # a hook on a projection shortcut's output, and one on a 3x3's: the groups that would leave them unstored are refused (other_reader=1)
    out += [("image", "resnet50", 64, "deepest+" + t, {}) for t in ("layer1.0.downsample", "layer1.1.conv2")]
    out += [("video", name, VIDEO_THW, "video_hooks", {}) for name in VIDEO]
    out += [("image", "resnet50", hw, hooks, OFF) for hw in (64, 96) for hooks in ("deepest", "all")]
    out.append(("video", "slowfast_resnet50", VIDEO_THW, "video_hooks", OFF))
    return out


def header(entry):
    kind, name, size, hooks, extra = entry
    size = "x".join(str(s) for s in size) if kind == "video" else str(size)
    return " ".join(["==", name, size, hooks] + [f"{k}={v}" for k, v in sorted(extra.items())])


def plan(entry):
    """In the child: plan the entry's net once (the engine prints its decisions to stderr)."""
    from i2v_amd import graphs, weights
    from tests.hostsim_util import hostsim_engine
    kind, name, size, hooks, _ = entry
    if kind == "video":
        g = graphs.build_video_tiny(name, tuple(size))
        ht, frames = graphs.video_hooks(g, name), 2 * size[0]
    else:
        g = graphs.build(name, (size, size))
        deepest = g.hooks[max(g.hooks)]
        if hooks == "all":
            ht = [g.hooks[d] for d in sorted(g.hooks)]
        elif hooks == "deepest":
            ht = [deepest]
        else:
            suffix = hooks.split("+", 1)[1]
            ht = [deepest, next(i for i, t in enumerate(g.tensors) if (t.name or "").endswith(suffix))]
        frames = 2
    hostsim_engine().build_net(g, weights.synthetic_state_dict(g, 0), ht, frames).close()


def trace_of(entry):
    env = {k: v for k, v in os.environ.items() if not k.startswith("I2V_")}
    env.update(ENV)
    env.update(entry[4])
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--plan", json.dumps(entry)], env=env, cwd=ROOT, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"planning {header(entry)} failed:\n{r.stderr[-2000:]}")
    return [header(entry)] + [l for l in r.stderr.splitlines() if l.startswith("[i2v ")]


def trace():
    """The whole catalogue's lines, in catalogue order."""
    from tests.hostsim_util import hostsim_engine
    hostsim_engine()                # (builds the host simulation once, before the children look for it)
    with ThreadPoolExecutor(max(1, min(8, os.cpu_count() or 1))) as pool:
        return [l for lines in pool.map(trace_of, catalogue()) for l in lines]


if __name__ == "__main__":
    if sys.argv[1:2] == ["--plan"]:
        plan(json.loads(sys.argv[2]))
    else:
        lines = trace()
        for tag in ("[i2v fuse]", "[i2v fastblock]", "[i2v scpair]", "[i2v overlap]"):
            assert any(l.startswith(tag) for l in lines), f"no {tag} line: widen the catalogue"
        assert any("other_reader=1" in l for l in lines), "no other_reader=1 line: widen the catalogue"
        assert any(l.startswith("[i2v scpair]") and ("dependent=1" in l or "other_reader=1" in l) for l in lines), "no refused shortcut pair"
        with open(FIXTURE, "w") as f:
            f.write("\n".join(lines) + "\n")
        print(FIXTURE, len(lines), "lines")
