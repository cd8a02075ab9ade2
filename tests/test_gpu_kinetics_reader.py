"""GPU (-m gpu): the ragged clip transform `i2v_clip_gather_resize_crop_u8_f32` (csrc/i2v_loader.hip) on the MI355X -- bit for
bit against the CPU restatement of the reference's validation transform and against the dense `clip_resize_crop` kernel, its
host-side refusals, and `image_main.py --video_dir` end to end against a `--clip_dir` run on the same clips cut by hand."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from i2v_amd import attacks, clips
from i2v_amd import lib as _lib
from oracle import restate

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def eng():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return attacks.get_engine("cuda:0")


def _video(seed, n, h, w):
    return np.random.RandomState(seed).randint(0, 256, size=(n, h, w, 3), dtype=np.uint8)


def test_ragged_batch_matches_the_restatement_and_the_dense_kernel(eng):
    vids = [_video(1, 300, 256, 340), _video(2, 40, 240, 320), _video(3, 120, 360, 480)]     # 40 frames: short branch, repeats
    idx = [clips.kinetics_frame_indices(len(v), ci) for v, ci in zip(vids, (9, -1, 6))]
    assert len(set(idx[1].tolist())) < 32
    pool, offsets = clips.pack_frames(vids, idx, pin=True)
    geom = clips.gather_geometry([v.shape[1:3] for v in vids])
    out = eng.clip_gather_resize_crop(pool, offsets, geom).cpu()
    assert out.shape == (3, 3, 32, 224, 224)
    for k, (v, i) in enumerate(zip(vids, idx)):
        ref = restate.resize_center_crop_normalise(v[i][None])
        assert torch.equal(out[k:k + 1], ref), k
    # a dense same-size batch: the existing kernel on the gathered frames, bit for bit (device pool, frame sizes as geometry)
    same = [_video(4, 200, 256, 340), _video(5, 50, 256, 340)]
    idx = [clips.kinetics_frame_indices(len(v), ci) for v, ci in zip(same, (-1, 9))]
    pool, offsets = clips.pack_frames(same, idx)
    got = eng.clip_gather_resize_crop(pool.to(eng.device), offsets, [(256, 340), (256, 340)])
    dense = torch.from_numpy(np.stack([v[i] for v, i in zip(same, idx)])).to(eng.device)
    assert torch.equal(got, eng.clip_resize_crop(dense))


def test_bad_tables_are_refused_before_any_launch(eng):
    vids = [_video(6, 70, 64, 80), _video(7, 30, 48, 64)]
    idx = [clips.kinetics_frame_indices(len(v), -1, 8, 2, 1) for v in vids]
    pool, offsets = clips.pack_frames(vids, idx)
    pool = pool.to(eng.device)
    geom, xtab, ytab = clips.gather_geometry([v.shape[1:3] for v in vids], 56, 48)
    capi = eng.capi
    b, t = offsets.shape
    nbytes = capi.i2v_clip_gather_scratch_bytes(b, t, len(xtab), len(ytab))
    scratch = torch.zeros(nbytes, dtype=torch.uint8, device=eng.device)
    out = torch.full((b, 3, t, 48, 48), float("nan"), device=eng.device)
    stream = eng.stream()

    def call(off, g):
        p = lambda a: a.ctypes.data_as(C.c_void_p)                                                     # noqa: E731
        return capi.i2v_clip_gather_resize_crop_u8_f32(C.c_void_p(pool.data_ptr()), pool.numel(), p(off), p(g), b, t, p(xtab), len(xtab),
                                                       p(ytab), len(ytab), 48, 48, C.c_void_p(out.data_ptr()), C.c_void_p(scratch.data_ptr()),
                                                       nbytes, stream)
    bad_off = offsets.copy()
    bad_off[1, 5] = pool.numel() - 100                                   # the frame would run past the pool
    assert call(bad_off, geom) != 0 and b"outside the pool" in capi.i2v_last_error()
    bad_geom = geom.copy()
    bad_geom[0, 5] = bad_geom[0, 3] - 47                                 # crop x origin: the window leaves the resized frame
    assert call(offsets, bad_geom) != 0 and b"crop window" in capi.i2v_last_error()
    bad_geom = geom.copy()
    bad_geom[1, 6] = len(xtab) - 10                                      # table rows past the end of xtab
    assert call(offsets, bad_geom) != 0 and b"resize table" in capi.i2v_last_error()
    with pytest.raises(_lib.I2VError, match="outside the pool"):
        eng.clip_gather_resize_crop(pool, bad_off, (geom, xtab, ytab), crop=48)
    torch.cuda.synchronize()
    assert torch.isnan(out).all() and int(scratch.count_nonzero()) == 0   # nothing was staged, nothing launched
    assert call(offsets, geom) == 0                                       # the intact tables go through
    torch.cuda.synchronize()
    assert torch.isfinite(out).all()


def test_image_main_video_dir_equals_clip_dir_of_the_same_frames(tmp_path, monkeypatch):
    import image_main
    rows = open(os.path.join(ROOT, "tests", "golden", "kinetics400_attack_samples.csv")).read().strip().split("\n")
    picked = [rows[1], rows[2], rows[-2], rows[-1]]                     # clip_index -1, -1, 6, 9
    shapes = [(12, 128, 170), (300, 128, 170), (120, 144, 192), (40, 144, 192)]     # 12 frames: short branch
    z = np.load(os.path.join(ROOT, "tests", "golden", "kinetics_frame_indices.npz"))
    cases, flat = z["cases"], z["indices"].astype(np.int64)
    starts = np.concatenate([[0], np.cumsum(cases[:, 6])])
    vdir, cdir = tmp_path / "videos", tmp_path / "clips"
    os.makedirs(cdir)
    for k, (row, (n, h, w)) in enumerate(zip(picked, shapes)):
        path, label, ci = row.split(",")
        v = _video(10 + k, n, h, w)
        p = clips.kinetics_video_path(str(vdir), path)
        os.makedirs(os.path.dirname(p), exist_ok=True)
        np.save(p, v)
        hit = np.nonzero((cases[:, 0] == n) & (cases[:, 1] == 2) & (cases[:, 2] == 8) & (cases[:, 3] == 1) & (cases[:, 4] == int(ci))
                         & (cases[:, 5] == -1))[0]
        assert len(hit) == 1, (n, ci)
        np.save(cdir / f"{label}-raw.npy", v[flat[starts[hit[0]]:starts[hit[0] + 1]]])
    (tmp_path / "picked.csv").write_text("\n".join([rows[0]] + picked) + "\n")
    monkeypatch.setattr(image_main, "OPT_PATH", str(tmp_path))
    common = ["--attack_method", "ImageGuidedFMDirection_Adam", "--step", "2", "--depth", "2", "--direction_image_model", "resnet50",
              "--frames", "8", "--hw", "112", "--batch_size", "2", "--synthetic_weights"]
    image_main.main(common + ["--file_prefix", "video", "--video_dir", str(vdir), "--anno", str(tmp_path / "picked.csv")])
    # the clip_dir run reads {label}-raw.npy in file-name order: same pairs of frame sizes only if the labels sort that way
    labels = [int(r.split(",")[1]) for r in picked]
    assert sorted(labels, key=str) == labels
    image_main.main(common + ["--file_prefix", "clips", "--clip_dir", str(cdir)])
    a, b = tmp_path / "Image-ImageGuidedFMDirection_Adam-2-video", tmp_path / "Image-ImageGuidedFMDirection_Adam-2-clips"
    for label in labels:
        x, y = (a / f"{label}-adv.npy").read_bytes(), (b / f"{label}-adv.npy").read_bytes()
        assert x == y, label
