"""Writes tests/golden/family_table.json (run on the CPU: `python -m tests.make_family_table_fixture`): what the Python package
answers about every transformer surrogate family, recorded BEFORE the families were folded into one block of `graphs.py` and one table row each,
so that the fold can be held to "nothing a caller can observe changes" (tests/test_family_table.py asserts every entry).

The committed file was written by this script on commit 1ff3f02 ("Serve timm's TNT family; add a batched short-sequence attention
kernel"), the last one before the fold.  It must not be regenerated from a later tree: it is the record
of that commit.

The script reaches every family through names that exist on both sides of the fold (`graphs.<word>_named`, `graphs.build_tiny`,
`weights.synthetic_state_dict`, ...), never through the family table, so that the table is checked and not trusted.  Three values are
reached by different accessors before and after; `_units`, `_native` and `_config` use the one the running commit has.

Per twin (family, served name the twin stands for, frame side) and seed (0 and 3):
  sd          sha256 over the keys and the bytes of `synthetic_state_dict`
  native      sha256 over the shapes and bytes of `native_arrays(sd, all blocks / stages)`
per twin:
  keys        sha256 over the ordered key list and shapes of `param_shapes()`
  macs, hooks, type, arch, config (the bytes of the ctypes config, hex), hook_shapes, and `workspace_bytes(hooks at depths 1 and 4,
  3 frames)` -- at the shallowest and the deepest depth the twin has where it has no depth 4 (the 6-block ViT twins).
The sides: every side a twin function names, and for the functions that take any multiple of a step, 64 and one more multiple.
Per family, refusals (exception type and message) of `<word>_named`, `build`, `build_surrogate` and `build_tiny` for a name of the
family's vocabulary that is not served and for a served name at 96 x 96, the KeyError of a depth outside the hooks, and the command
line's error for such a depth; `build` / `build_surrogate` / `build_tiny` on "transformer", "densenet" and "pit_s_224"; and the help
string of `image_main.py`'s `--direction_image_model`."""
import contextlib
import hashlib
import io
import json
import os

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "golden", "family_table.json")

#: (family word, a served name that maps to the twin, frame sides)
TWINS = [("vit", "vit_base_patch16_224", (64, 96)), ("vit", "deit_tiny_distilled_patch16_224", (64,)), ("vit", "vit_base_patch32_224", (64,)),
         ("swin", "swin_tiny_patch4_window7_224", (64, 96)), ("convnext", "convnext_tiny", (64, 96)),
         ("mixer", "mixer_b16_224", (64, 96)), ("mixer", "mixer_b32_224", (64,)), ("mixer", "resmlp_12_224", (64,)),
         ("cait", "cait_xxs24_224", (64, 80)), ("convit", "convit_tiny", (64, 80)), ("xcit", "xcit_nano_12_p16_224", (64, 80)),
         ("twins", "twins_pcpvt_small", (64, 96)), ("twins", "twins_svt_small", (128, 224)),
         ("beit", "beit_base_patch16_224", (64, 96, 224)), ("pit", "pit_s_224", (64, 70, 224)), ("coat", "coat_lite_tiny", (64, 96, 224)),
         ("tnt", "tnt_s_patch16_224", (64, 48, 224))]
SEEDS = (0, 3)
#: family word -> (a name of its vocabulary that is not served, a served name)
BAD = {"vit": ("vit_base_patch16_384", "vit_base_patch16_224"), "swin": ("swin_base_patch4_window12_384", "swin_tiny_patch4_window7_224"),
       "convnext": ("convnextv2_tiny", "convnext_tiny"), "mixer": ("gmlp_s16_224", "mixer_b16_224"), "cait": ("cait_m48_448", "cait_xxs24_224"),
       "convit": ("convit_huge", "convit_tiny"), "xcit": ("xcit_nano_12_p8_224", "xcit_nano_12_p16_224"),
       "twins": ("twins_svt_huge", "twins_svt_small"), "beit": ("beit_large_patch16_512", "beit_base_patch16_224"),
       "pit": ("pit_xl_224", "pit_s_224"), "coat": ("coat_tiny", "coat_lite_tiny"), "tnt": ("tnt_l_patch16_224", "tnt_s_patch16_224")}
RESOLVER_NAMES = ("transformer", "densenet", "pit_s_224")


def _units(spec):
    """All blocks / stages of the spec, as the create entry counts them."""
    from i2v_amd import engine
    if hasattr(spec, "units"):
        return spec.units
    return engine.TOKEN_FAMILIES[type(spec)][2](spec)


def _native(spec, sd, depth):
    from i2v_amd import engine
    if hasattr(spec, "native_arrays"):
        return spec.native_arrays(sd, depth)
    net = {"VitSpec": "VitNet", "SwinSpec": "SwinNet"}[type(spec).__name__]       # (before the fold these two packed in their Net class)
    return getattr(engine, net)._weights(None, spec, sd, depth)


def _config(spec):
    from i2v_amd import engine
    if hasattr(engine, "token_config"):
        return engine.token_config(spec)
    return engine.TOKEN_FAMILIES[type(spec)][1](spec)


def _sha_tensors(named):
    h = hashlib.sha256()
    for k, t in named:
        t = t.detach().cpu().contiguous()
        h.update(f"{k}{tuple(t.shape)}{t.dtype}".encode())
        h.update(t.numpy().tobytes())
    return h.hexdigest()


def _hook_shape(spec, where):
    """(tokens, width) of the stream hooked at block / stage `where`: the spec's own `hook_shape` where it has one, else by the
    rules `TokenNet.hook_shape` had before the fold."""
    if hasattr(spec, "hook_shape"):
        return list(spec.hook_shape(where))[:2]
    if hasattr(spec, "tokens_at"):
        return [spec.tokens_at(where), spec.dim]
    if callable(spec.tokens):
        return [spec.tokens(where), spec.width(where)]
    return [spec.tokens, spec.dim]


def twin_record(name, side):
    from i2v_amd import graphs, weights
    spec = graphs.build_tiny(name, (side, side))
    shapes = spec.param_shapes()
    depths = sorted(spec.hooks)
    rec = {"type": type(spec).__name__, "arch": spec.arch, "in_hw": list(spec.in_hw),
           "keys": hashlib.sha256(json.dumps([[k, list(v)] for k, v in shapes.items()]).encode()).hexdigest(),
           "macs": int(spec.macs_per_frame()), "hooks": {str(d): spec.hooks[d] for d in depths},
           "hook_shapes": {str(d): _hook_shape(spec, spec.hooks[d]) for d in depths},
           "config": bytes(_config(spec)).hex(), "units": int(_units(spec))}
    if hasattr(spec, "workspace_bytes"):
        rec["workspace_bytes"] = int(spec.workspace_bytes([spec.hook_for(depths[0]), spec.hook_for(depths[-1])], 3))
    for seed in SEEDS:
        sd = weights.synthetic_state_dict(spec, seed)
        assert list(sd) == list(shapes)
        rec[f"sd{seed}"] = _sha_tensors(sd.items())
        rec[f"native{seed}"] = _sha_tensors((str(i), t) for i, t in enumerate(_native(spec, sd, _units(spec))))
    return rec


def _raised(fn, *args):
    try:
        out = fn(*args)
    except Exception as e:      # noqa: BLE001 -- the type is what is recorded
        return [type(e).__name__, str(e)]
    return ["returned", type(out).__name__ + ":" + out.arch]


def _cli_error(argv):
    import image_main
    err = io.StringIO()
    with contextlib.redirect_stderr(err):
        try:
            image_main.arg_parse(argv)
        except SystemExit as e:
            return [f"SystemExit({e.code})", err.getvalue().splitlines()[-1].split(": error: ", 1)[-1]]
    return ["returned", ""]


def refusal_record(word):
    from i2v_amd import graphs
    unserved, served = BAD[word]
    named = getattr(graphs, f"{word}_named")
    rec = {"is_name": [bool(getattr(graphs, f"is_{word}_name")(n)) for n in (unserved, served, "resnet")]}
    for label, fn in (("named", named), ("build", graphs.build), ("build_surrogate", graphs.build_surrogate)):
        rec[f"{label}_unserved"] = _raised(fn, unserved)
        rec[f"{label}_96"] = _raised(fn, served, (96, 96))
    rec["build_tiny_unserved"] = _raised(graphs.build_tiny, unserved)
    rec["build_tiny_unserved_224"] = _raised(graphs.build_tiny, unserved, (224, 224))
    rec["depth_9"] = _raised(named(served).hook_for, 9)
    cli = ["--attack_method", "ImageGuidedStd_Adam", "--direction_image_model"]
    rec["cli_depth_9"] = _cli_error(cli + [served, "--depth", "9"])
    rec["cli_unserved"] = _cli_error(cli + [unserved])
    rec["cli_96"] = _cli_error(cli + [served, "--hw", "96"])
    return rec


def help_string():
    """The `help` of `--direction_image_model`, taken from the parser `arg_parse` builds."""
    import argparse
    import image_main
    seen = {}

    class Stop(Exception):
        pass

    def grab(self, *a, **k):
        seen["parser"] = self
        raise Stop()
    real = argparse.ArgumentParser.parse_args
    argparse.ArgumentParser.parse_args = grab
    try:
        image_main.arg_parse([])
    except Stop:
        pass
    finally:
        argparse.ArgumentParser.parse_args = real
    return next(a.help for a in seen["parser"]._actions if a.dest == "direction_image_model")


def collect():
    from i2v_amd import graphs
    record = {"twins": {f"{word}/{name}/{side}": twin_record(name, side) for word, name, sides in TWINS for side in sides},
              "refusals": {word: refusal_record(word) for word in BAD},
              "resolvers": {f"{fn}/{name}": _raised(getattr(graphs, fn), name) for fn in ("build", "build_surrogate", "build_tiny")
                            for name in RESOLVER_NAMES},
              "help": help_string()}
    return record


if __name__ == "__main__":
    import sys
    sys.path[:0] = [os.path.join(os.path.dirname(HERE), "image-to-video-i2v-attack_amd"), os.path.dirname(HERE)]
    record = collect()
    with open(OUT, "w") as fh:          # one line per twin, family and resolver call
        parts = []
        for sec in sorted(record):
            if isinstance(record[sec], dict):
                rows = ",\n".join(f"  {json.dumps(k)}: {json.dumps(v, sort_keys=True)}" for k, v in sorted(record[sec].items()))
                parts.append(f" {json.dumps(sec)}: {{\n{rows}\n }}")
            else:
                parts.append(f" {json.dumps(sec)}: {json.dumps(record[sec])}")
        fh.write("{\n" + ",\n".join(parts) + "\n}\n")
    print("wrote", OUT)
