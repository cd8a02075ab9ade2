#!/usr/bin/env python
"""Writes tests/golden/kinetics_frame_indices.npz: the frame indices the reference's Kinetics loader
(`datasets.VideoClsDataset.loadvideo_decord`, validation mode) passes to `vr.get_batch`, taken from the UNMODIFIED
reference class imported under stubs -- `oracle.ref_shim.install()`, a `gluoncv.torch.data` with no-op transforms and a
`decord.VideoReader` whose length is the case's frame count and whose `get_batch(idx)` returns `idx`.  Only the index
arrays are stored.

Cases: every frame count N = 1..400 x frame_sample_rate {1, 2, 4} x clip_len {8, 32} x num_segment {1, 2} x clip_index
{-1, 6, 9, 0, 12345}, plus the 400 rows of the sample list (tests/golden/kinetics400_attack_samples.csv) with their own
clip_index at the defaults 32 / 2 / 1 and an ASSUMED length per row (`assumed_length`: Kinetics clips are ten-second cuts, 240-300
frames).  A case with fewer frames than segments, where the reference clips to [0, -1], is stored as refused (length 0).

    python tools/make_kinetics_indices.py [--out tests/golden/kinetics_frame_indices.npz]
"""
import argparse
import contextlib
import csv
import os
import sys
import tempfile
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CSV = os.path.join(ROOT, "tests", "golden", "kinetics400_attack_samples.csv")
GRID_N = range(1, 401)
GRID_RATE = (1, 2, 4)
GRID_CLIP_LEN = (8, 32)
GRID_NSEG = (1, 2)
GRID_CLIP_INDEX = (-1, 6, 9, 0, 12345)


def assumed_length(row):
    """The frame count assumed for sample-list row `row` (0-based)."""
    return 240 + (37 * row) % 61


class _Reader:
    """`decord.VideoReader` stand-in: `len()` is the current case's frame count, `get_batch(idx)` hands back the indices."""
    n_frames = 0

    def __init__(self, *a, **k):
        self.n = _Reader.n_frames

    def __len__(self):
        return self.n

    def seek(self, pos):
        pass

    def get_batch(self, idx):
        arr = np.asarray(idx, dtype=np.int64)
        return types.SimpleNamespace(asnumpy=lambda: arr)


def _install_stubs():
    from oracle import ref_shim
    ref_shim.install()
    noop = type("NoOp", (), {"__init__": lambda self, *a, **k: None, "__call__": lambda self, x: x})
    data = types.ModuleType("gluoncv.torch.data")
    data.video_transforms = types.SimpleNamespace(Compose=noop, Resize=noop, CenterCrop=noop, Normalize=noop, RandomResize=noop,
                                                  RandomCrop=noop, RandomHorizontalFlip=noop)
    data.volume_transforms = types.SimpleNamespace(ClipToTensor=noop)
    data.multiGridHelper = noop
    data.MultiGridBatchSampler = noop
    sys.modules["gluoncv.torch.data"] = data
    sys.modules["gluoncv.torch"].data = data
    decord = types.ModuleType("decord")
    decord.VideoReader = _Reader
    decord.cpu = lambda i: None
    sys.modules["decord"] = decord
    # by file: a `datasets` package elsewhere on the path (Hugging Face's) must not shadow the reference module
    import importlib.util
    spec = importlib.util.spec_from_file_location("_reference_datasets", os.path.join(ref_shim.REFERENCE_DIR, "datasets.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@contextlib.contextmanager
def reference_loader(clip_len, frame_sample_rate, num_segment):
    """Yields `indices(n_frames, clip_index)` -> what the reference's loader selects (numpy's global random state is restored
    afterwards: the reference seeds it)."""
    datasets = _install_stubs()
    state = np.random.get_state()
    with tempfile.TemporaryDirectory() as d:
        with open(os.path.join(d, "v.mp4"), "wb") as fh:      # the loader skips files under 1 KB
            fh.write(b"\0" * 1024)
        with open(os.path.join(d, "a.csv"), "w") as fh:
            fh.write("path,gt_label,clip_index\nv.mp4,0,-1\n")
        ds = datasets.VideoClsDataset(os.path.join(d, "a.csv"), d, mode="validation", clip_len=clip_len,
                                      frame_sample_rate=frame_sample_rate, num_segment=num_segment)

        def indices(n_frames, clip_index):
            _Reader.n_frames = n_frames
            return np.asarray(ds.loadvideo_decord("v.mp4", clip_index), np.int64)
        try:
            yield indices
        finally:
            np.random.set_state(state)


def cases():
    """(n_frames, frame_sample_rate, clip_len, num_segment, clip_index, sample-list row or -1)."""
    for rate in GRID_RATE:
        for clip_len in GRID_CLIP_LEN:
            for nseg in GRID_NSEG:
                for ci in GRID_CLIP_INDEX:
                    for n in GRID_N:
                        yield n, rate, clip_len, nseg, ci, -1
    with open(CSV) as fh:
        for row, r in enumerate(csv.DictReader(fh)):
            yield assumed_length(row), 2, 32, 1, int(r["clip_index"]), row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "kinetics_frame_indices.npz"))
    args = ap.parse_args()
    table, flat, loaders = [], [], {}
    with contextlib.ExitStack() as stack:
        for n, rate, clip_len, nseg, ci, row in cases():
            key = (clip_len, rate, nseg)
            if key not in loaders:
                loaders[key] = stack.enter_context(reference_loader(clip_len, rate, nseg))
            if n < nseg:
                table.append((n, rate, clip_len, nseg, ci, row, 0))
                continue
            idx = loaders[key](n, ci)
            assert idx.shape == (clip_len * nseg,) and idx.min() >= 0 and idx.max() < n, (n, rate, clip_len, nseg, ci, idx)
            table.append((n, rate, clip_len, nseg, ci, row, len(idx)))
            flat.append(idx)
    np.savez_compressed(args.out, cases=np.asarray(table, np.int32), indices=np.concatenate(flat).astype(np.int16))
    print(f"{args.out}: {len(table)} cases, {sum(len(f) for f in flat)} indices")


if __name__ == "__main__":
    main()
