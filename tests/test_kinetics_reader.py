"""CPU: the whole-video Kinetics reader -- the reference loader's frame selection (`datasets.py:216-244`) against the stored
reference results (tests/golden/kinetics_frame_indices.npz, tools/make_kinetics_indices.py) and, where the reference is present,
against the imported reference class live; the pool / offset / geometry tables the ragged transform takes; the refusals."""
import importlib.util
import os

import numpy as np
import pytest
import torch

from i2v_amd import clips

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def _golden():
    z = np.load(os.path.join(GOLDEN, "kinetics_frame_indices.npz"))
    cases, flat = z["cases"], z["indices"].astype(np.int64)
    starts = np.concatenate([[0], np.cumsum(cases[:, 6])])
    return cases, flat, starts


def test_frame_indices_match_the_reference_on_every_stored_case():
    cases, flat, starts = _golden()
    assert len(cases) == 400 * 3 * 2 * 2 * 5 + 400
    refused = 0
    for k, (n, rate, clip_len, nseg, ci, _row, length) in enumerate(cases):
        if length == 0:             # fewer frames than segments: the reference clips to [0, -1]; refused here
            with pytest.raises(ValueError):
                clips.kinetics_frame_indices(n, ci, clip_len, rate, nseg)
            refused += 1
            continue
        got = clips.kinetics_frame_indices(n, ci, clip_len, rate, nseg)
        assert got.dtype == np.int64
        np.testing.assert_array_equal(got, flat[starts[k]:starts[k + 1]], err_msg=str((n, rate, clip_len, nseg, ci)))
    assert refused == 3 * 2 * 5            # N = 1 with two segments


def test_frame_indices_cover_both_branches_and_leave_numpy_state_alone():
    state = np.random.get_state()
    short = clips.kinetics_frame_indices(40, -1)                      # 40 <= 64: linspace(0, 40, 20) padded with the last frame
    assert len(short) == 32 and short[-1] == 39 and (short[20:] == 39).all()
    assert clips.kinetics_frame_indices(300, -1)[-1] == 298             # the end of the video: clip to end_idx - 1
    a, b = clips.kinetics_frame_indices(300, 9), clips.kinetics_frame_indices(300, 6)
    assert not np.array_equal(a, b)
    after = np.random.get_state()
    assert all(np.array_equal(x, y) if isinstance(x, np.ndarray) else x == y for x, y in zip(state, after))
    with pytest.raises(ValueError):
        clips.kinetics_frame_indices(0, -1)


def _tool():
    spec = importlib.util.spec_from_file_location("make_kinetics_indices", os.path.join(ROOT, "tools", "make_kinetics_indices.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_frame_indices_match_the_imported_reference_live():
    from oracle import ref_shim
    if not ref_shim.available() or not os.path.isfile(os.path.join(ref_shim.REFERENCE_DIR, "datasets.py")):
        pytest.skip("the reference is not on this machine")
    tool = _tool()
    rng = np.random.RandomState(2024)
    for clip_len, rate, nseg in ((32, 2, 1), (8, 4, 2), (16, 3, 3)):      # (16, 3, 3) is outside the stored grid
        with tool.reference_loader(clip_len, rate, nseg) as ref:
            for n in list(rng.randint(nseg, 500, size=12)) + [nseg, clip_len * rate, clip_len * rate + 1]:
                n = int(max(n, nseg))
                for ci in (-1, 9, int(rng.randint(0, 1 << 30))):
                    np.testing.assert_array_equal(clips.kinetics_frame_indices(n, ci, clip_len, rate, nseg), ref(n, ci),
                                                  err_msg=str((n, ci, clip_len, rate, nseg)))


def _write_videos(tmp_path, specs):
    """specs: [(csv path, label, clip_index, (N, H, W) or None for no file)] -> (csv, video_dir, {path: video})."""
    vdir = tmp_path / "videos"
    videos = {}
    lines = ["path,gt_label,clip_index"]
    for k, (path, label, ci, shape) in enumerate(specs):
        lines.append(f"{path},{label},{ci}")
        if shape is None:
            continue
        v = np.random.RandomState(k).randint(0, 256, size=shape + (3,), dtype=np.uint8)
        p = clips.kinetics_video_path(str(vdir), path)
        os.makedirs(os.path.dirname(p), exist_ok=True)
        np.save(p, v)
        videos[path] = v
    csv = tmp_path / "samples.csv"
    csv.write_text("\n".join(lines) + "\n")
    return str(csv), str(vdir), videos


def test_reader_pools_distinct_frames_with_offsets_geometry_and_names(tmp_path):
    specs = [("abseiling/a_000001.mp4", 0, -1, (300, 64, 80)), ("air drumming/b.c.mp4", 1, 9, (40, 50, 60)),
             ("applauding/c.mp4", 2, 6, (120, 72, 96))]
    csv, vdir, videos = _write_videos(tmp_path, specs)
    out = list(clips.kinetics_video_batches(2, csv, vdir, short_side=56, crop=48, pin=False, workers=1))
    assert len(out) == 2 == clips.kinetics_num_batches(2, csv)
    assert [n for b in out for n in b[3]] == ["abseiling/a_000001", "air drumming/b", "applauding/c"]      # path.split(".")[0]
    assert [int(x) for b in out for x in b[2]] == [0, 1, 2]
    k = 0
    for pool, (offsets, geom, xtab, ytab), labels, _ in out:
        assert pool.dtype == torch.uint8 and offsets.dtype == np.int64 and geom.dtype == np.int32
        assert offsets.shape == (len(labels), 32) and geom.shape == (len(labels), 8)
        host = pool.numpy()
        distinct = 0
        for ci in range(len(labels)):
            path, _, clip_ind, (n, h, w) = specs[k]
            v = videos[path]
            idx = clips.kinetics_frame_indices(n, clip_ind)
            distinct += len(set(idx.tolist()))
            H, W, rh, rw, cy, cx, xr, yr = geom[ci]
            assert (H, W) == (h, w) and (rh, rw) == clips.resize_sizes(h, w, 56) and (cy, cx) == clips.center_crop_origin(rh, rw, 48, 48)
            np.testing.assert_array_equal(xtab[xr:xr + rw], clips.resize_table(rw, w))
            np.testing.assert_array_equal(ytab[yr:yr + rh], clips.resize_table(rh, h))
            for ti, f in enumerate(idx):
                o = offsets[ci, ti]
                assert o % clips.POOL_ALIGN == 0
                np.testing.assert_array_equal(host[o:o + h * w * 3].reshape(h, w, 3), v[f])
            same = {}                                        # repeated frames share one slot
            for ti, f in enumerate(idx):
                assert same.setdefault(int(f), offsets[ci, ti]) == offsets[ci, ti]
            k += 1
        assert len(np.unique(offsets)) == distinct
    short = out[0][1][0][1]                                 # the 40-frame video: short branch, frame 39 repeated 13 times
    assert len(np.unique(short)) == 20


def test_reader_refuses_missing_and_empty_videos_naming_the_row(tmp_path):
    csv, vdir, _ = _write_videos(tmp_path, [("a/x.mp4", 0, -1, (70, 8, 8)), ("b/missing.mp4", 1, -1, None)])
    with pytest.raises(FileNotFoundError, match=r"row 1 \(b/missing.mp4\)"):
        list(clips.kinetics_video_batches(1, csv, vdir, short_side=8, crop=8, pin=False))
    csv, vdir, _ = _write_videos(tmp_path, [("a/x.mp4", 0, -1, (70, 8, 8)), ("c/empty.mp4", 1, -1, (0, 8, 8))])
    with pytest.raises(ValueError, match=r"row 1 \(c/empty.mp4\).*no frames"):
        list(clips.kinetics_video_batches(1, csv, vdir, short_side=8, crop=8, pin=False))


def test_gather_geometry_shares_tables_and_refuses_small_frames():
    geom, xtab, ytab = clips.gather_geometry([(256, 340), (360, 480), (256, 340)])
    assert geom[0].tolist() == [256, 340, 256, 340, 16, 58, 0, 0] and geom[2].tolist() == geom[0].tolist()
    assert geom[1].tolist()[:6] == [360, 480, 256, 341, 16, 58] and tuple(geom[1, 6:]) == (340, 256)
    assert xtab.shape == (340 + 341, 3) and ytab.shape == (256 + 256, 3)
    with pytest.raises(ValueError, match="smaller than"):
        clips.gather_geometry([(100, 100)], short_side=128, crop=224)


@pytest.mark.parametrize("module", ["image_main", "attack"])
def test_cli_video_flags_are_checked(module, tmp_path, monkeypatch):
    monkeypatch.setenv("I2V_OPT_PATH", str(tmp_path))
    mod = __import__(module)
    monkeypatch.setattr(mod, "OPT_PATH", str(tmp_path))
    anno = os.path.join(GOLDEN, "kinetics400_attack_samples.csv")
    for bad in (["--video_dir", str(tmp_path)],                                                        # no sample list
                ["--video_dir", str(tmp_path), "--anno", anno, "--clip_dir", str(tmp_path)],           # two sources
                ["--video_dir", str(tmp_path), "--anno", anno, "--num_segment", "3"],                  # 32 frames != clip_len * 3
                ["--video_dir", str(tmp_path), "--anno", anno, "--frame_sample_rate", "0"],
                ["--video_dir", str(tmp_path), "--anno", anno, "--short_side", "200"]):               # below the 224 crop
        with pytest.raises(SystemExit):
            mod.arg_parse(bad)
    args = mod.arg_parse(["--video_dir", str(tmp_path), "--anno", anno, "--num_segment", "2", "--frame_sample_rate", "4"])
    assert (args.frames, args.num_segment, args.frame_sample_rate, args.short_side) == (32, 2, 4, 256)
    args = mod.arg_parse([])
    assert (args.video_dir, args.frame_sample_rate, args.num_segment) == ("", 2, 1)
