"""Clip sources for the CLI.  The reference decodes Kinetics-400 mp4s with decord
(`/root/reference/datasets.py`; mp4 decoding is out of scope: SURVEY.md 8(f) N4); here a batch is either

  * synthetic: 8-bit uniform-noise clips seeded by the sample's row index, labelled
    from the reference's sample list format `path,gt_label,clip_index`,
  * a directory of `{label}-ori.npy` float32 (3,32,224,224) normalised clips (the format the
    reference's own `attack.py` writes next to `{label}-adv.npy`) or `{label}-raw.npy` decoded clips, or
  * whole decoded videos, one `.npy` per sample-list row, from which each clip's frames are selected by the
    reference loader's arithmetic (`kinetics_frame_indices`, `kinetics_video_batches`): a ragged pool of
    distinct frames plus offset / geometry tables for `Engine.clip_gather_resize_crop`.

Each item mirrors the reference's validation item `(clip, label, name)` (`datasets.py:138-150`)."""
import csv
import glob
import math
import os

import numpy as np
import torch

MEAN = (0.485, 0.456, 0.406)
STD = (0.229, 0.224, 0.225)


def synthetic_clip(seed: int, frames=32, hw=224) -> torch.Tensor:
    gen = torch.Generator().manual_seed(1000 + seed)
    u8 = torch.randint(0, 256, (3, frames, hw, hw), generator=gen, dtype=torch.uint8)
    mean = torch.tensor(MEAN).view(3, 1, 1, 1)
    std = torch.tensor(STD).view(3, 1, 1, 1)
    return (u8.float() / 255 - mean) / std


def sample_list(csv_path=None, n=400):
    """[(name, label)] -- from a `path,gt_label,clip_index` csv when given, else n synthetic rows."""
    if csv_path and os.path.exists(csv_path):
        with open(csv_path) as fh:
            return [(r["path"], int(r["gt_label"])) for r in csv.DictReader(fh)][:n]
    return [(f"synthetic/{i:03d}.mp4", i) for i in range(n)]


def batches(batch_size, csv_path=None, clip_dir=None, frames=32, hw=224, n=400, workers=0):
    """Yields (val_batch (b,3,f,h,w), val_label (b,), video_names) like the reference's DataLoader.  A `clip_dir` of
    `{label}-raw.npy` files -- DECODED uint8 frames (t,H,W,3), what decord hands the reference's loader
    (datasets.py:226-244) -- yields uint8 batches (b,t,H,W,3) instead: the caller runs the validation transform on the
    device (`Engine.clip_resize_crop`, datasets.py:86-93).  Raw clips of one batch must share their frame size."""
    raw = sorted(glob.glob(os.path.join(clip_dir, "*-raw.npy"))) if clip_dir else []
    if raw:
        items = [(os.path.basename(p), int(os.path.basename(p).split("-")[0]), p) for p in raw]
    elif clip_dir:
        files = sorted(glob.glob(os.path.join(clip_dir, "*-ori.npy")))
        items = [(os.path.basename(p), int(os.path.basename(p).split("-")[0]), p) for p in files]
    else:
        items = [(name, label, None) for name, label in sample_list(csv_path, n)]
    def load(s):
        chunk = items[s:s + batch_size]
        clips = [torch.from_numpy(np.load(p)) if p else synthetic_clip(s + i, frames, hw)
                 for i, (_, _, p) in enumerate(chunk)]
        return torch.stack(clips), torch.tensor([c[1] for c in chunk]), [c[0] for c in chunk]
    # `workers` loader threads, a window of 2 x workers batches in flight, results in order (np.load and the synthetic
    # generator release the GIL): what the reference's DataLoader workers are for
    yield from _prefetched(load, list(range(0, len(items), batch_size)), workers)


def num_batches(batch_size, csv_path=None, clip_dir=None, n=400):
    if clip_dir:
        cnt = len(glob.glob(os.path.join(clip_dir, "*-raw.npy"))) or len(glob.glob(os.path.join(clip_dir, "*-ori.npy")))
    else:
        cnt = len(sample_list(csv_path, n))
    return (cnt + batch_size - 1) // batch_size


# ---------------------------------------------------------------------------------------------------------------
# geometry of the reference's validation transform (datasets.py:86-93; gluoncv.torch.data.video_transforms), host side
# of `Engine.clip_resize_crop`.  gluoncv and OpenCV are third-party to the reference and not installed here: restated
# from their public sources, parity UNPINNED (oracle/restate.py:resize_center_crop_normalise is the CPU twin).
# ---------------------------------------------------------------------------------------------------------------
def resize_sizes(h, w, short_side):
    """`video_transforms.Resize(size: int)`: the short side becomes `size`, the other int(size * long / short);
    an image whose short side already is `size` is left alone."""
    if (w <= h and w == short_side) or (h <= w and h == short_side):
        return h, w
    if w < h:
        return int(short_side * h / w), short_side
    return short_side, int(short_side * w / h)


def center_crop_origin(h, w, ch, cw):
    """`video_transforms.CenterCrop`: (y1, x1) = round((im - crop) / 2)."""
    return int(round((h - ch) / 2.0)), int(round((w - cw) / 2.0))


def resize_table(n_out, n_in):
    """Per output index of a bilinear axis resize as cv::resize (INTER_LINEAR, 8-bit) builds it: source index,
    weight of it and of its right/lower neighbour in INTER_RESIZE_COEF_SCALE = 2048 units (int32 (n_out, 3)).
        fx = (float)((d + 0.5) * scale - 0.5); sx = floor(fx); fx -= sx
        sx < 0 -> sx = 0, fx = 0;  sx >= n_in - 1 -> sx = n_in - 1, fx = 0
        weights = saturate_cast<short>(rint((1 - fx) * 2048)), saturate_cast<short>(rint(fx * 2048))"""
    scale = np.float64(n_in) / np.float64(n_out)
    d = np.arange(n_out, dtype=np.float64)
    fx = ((d + 0.5) * scale - 0.5).astype(np.float32)
    sx = np.floor(fx).astype(np.int64)
    fx = (fx - sx.astype(np.float32)).astype(np.float32)
    lo, hi = sx < 0, sx >= n_in - 1
    fx = np.where(lo | hi, np.float32(0), fx)
    sx = np.where(lo, 0, np.where(hi, n_in - 1, sx))
    a1 = np.rint(fx * np.float32(2048)).astype(np.int64)
    a0 = np.rint((np.float32(1) - fx) * np.float32(2048)).astype(np.int64)
    return np.stack([sx, a0, a1], 1).astype(np.int32)


# ---------------------------------------------------------------------------------------------------------------
# geometry of the UCF-101 loader's validation transform (`dataset_ucf101.py:113-126`, `transforms_ucf101.py`):
# Scale(224) = PIL `Image.resize(..., BILINEAR)` to short side 224, CornerCrop(224, 'c'), ToTensor (/255), Normalize.
# Pillow IS installed here, so the restatement of its resampler (libImaging/Resample.c: antialiased two-pass convolution,
# 8-bit path with 22-bit fixed-point coefficients) is pinned bit for bit against the library itself
# (tests/test_pil_resample.py); host side of `Engine.clip_resample_crop`.
# ---------------------------------------------------------------------------------------------------------------
PIL_PRECISION_BITS = 32 - 8 - 2


def scale_sizes(h, w, size):
    """`transforms_ucf101.Scale(size: int)` (:271-289): the smaller edge becomes `size`, the other int(size * long / short)."""
    if (w <= h and w == size) or (h <= w and h == size):
        return h, w
    if w < h:
        return int(size * h / w), size
    return size, int(size * w / h)


def corner_crop_center_origin(h, w, size):
    """`CornerCrop(size, 'c')` (:343-348): x1 = int(round((W - size) / 2.)), y1 likewise (Python 3 banker's rounding)."""
    return int(round((h - size) / 2.0)), int(round((w - size) / 2.0))


def pil_resample_table(n_in, n_out):
    """Pillow's `precompute_coeffs` + `normalize_coeffs_8bpc` for the BILINEAR filter over the full axis: per output index the
    first source index, the number of taps, and the taps as 22-bit fixed-point integers.  Returns (bounds int32 (n_out, 2),
    coeffs int32 (n_out, ksize), ksize).  Downscaling widens the triangle filter by the scale factor (antialiasing)."""
    scale = float(n_in) / float(n_out)
    filterscale = max(scale, 1.0)
    support = 1.0 * filterscale                         # bilinear: support 1
    ksize = int(math.ceil(support)) * 2 + 1
    bounds = np.zeros((n_out, 2), np.int32)
    coeffs = np.zeros((n_out, ksize), np.int32)
    ss = 1.0 / filterscale
    for xx in range(n_out):
        center = 0.0 + (xx + 0.5) * scale
        xmin = int(center - support + 0.5)              # C cast: truncation
        if xmin < 0:
            xmin = 0
        xmax = int(center + support + 0.5)
        if xmax > n_in:
            xmax = n_in
        xmax -= xmin
        w = []
        for x in range(xmax):
            t = abs((x + xmin - center + 0.5) * ss)
            w.append(1.0 - t if t < 1.0 else 0.0)
        ww = sum(w)                                     # left-to-right double sum, as the C loop
        for x in range(xmax):
            k = w[x] / ww if ww != 0.0 else w[x]
            coeffs[xx, x] = int(-0.5 + k * (1 << PIL_PRECISION_BITS)) if k < 0 else int(0.5 + k * (1 << PIL_PRECISION_BITS))
        bounds[xx] = (xmin, xmax)
    return bounds, coeffs, ksize


# ---------------------------------------------------------------------------------------------------------------
# UCF-101 jpg-frame folders (`/root/reference/dataset_ucf101.py`): the clip list, the temporal selection and the
# decoding -- everything in front of the loader's spatial transform, which runs on the device (`Engine.clip_resample_crop`).
# Decoding is Pillow's (installed here, and what the reference calls, :14-18), so the reader is pinned by construction.
# (The Kinetics-400 half of N4 -- decord reading mp4s, `datasets.py:188-244` -- is NOT buildable in this image: no decord,
# PyAV, OpenCV or ffmpeg.  Its entry points are `--clip_dir` of `{label}-raw.npy` cut clips and `--video_dir` of whole decoded
# videos, below.)
# ---------------------------------------------------------------------------------------------------------------
def loop_padding(frame_indices, size=32):
    """`transforms_ucf101.LoopPadding(size)` (:23-40), quirks included: the selection starts at the SECOND entry
    (`frame_indices[1:size+1]`), and a clip shorter than `size + 1` frames is padded by cycling through that selection (the
    reference appends to the list it is iterating over, which walks the growing list from its start)."""
    out = list(frame_indices[1:size + 1])
    k = 0
    while len(out) < size and k < len(out):
        out.append(out[k])
        k += 1
    return out


def _load_index_list(path):
    """The reference's `used_idxs.pkl` (a pickled list of ints, `dataset_ucf101.py:59-63`) -- read with an unpickler that
    admits NO globals (a list of ints needs none; anything else in the file is refused) --, or a .json / whitespace-separated
    text file holding the same list."""
    if path.endswith(".pkl"):
        import pickle

        class _NoGlobals(pickle.Unpickler):
            def find_class(self, module, name):
                raise pickle.UnpicklingError(f"{path}: only a plain list of integers is accepted (found {module}.{name})")
        with open(path, "rb") as fh:
            idx = _NoGlobals(fh).load()
    elif path.endswith(".json"):
        import json
        with open(path) as fh:
            idx = json.load(fh)
    else:
        with open(path) as fh:
            idx = fh.read().split()
    return [int(i) for i in idx]


def ucf101_clip_list(setting, image_root, used_idxs=None):
    """`attack_ucf101._make_dataset` (:81-99) + the index selection (:59-64): [(frame directory, duration, label)] from the
    lines `video_path duration label` of `test01_setting.txt`, reduced to the rows `used_idxs` names (a path to the index list,
    a list of ints, or None = every row)."""
    if not os.path.exists(setting):
        raise RuntimeError("Setting file %s doesn't exist. Check opt.train-list and opt.val-list. " % setting)      # :83
    rows = []
    with open(setting) as fh:
        for line in fh.readlines():
            info = line.split()
            if len(info) < 3:
                raise RuntimeError("Video input format is not correct, missing one or more element. %s" % line)     # :91
            rows.append((os.path.join(image_root, info[0]), int(info[1]), int(info[2])))
    if used_idxs is None:
        return rows
    idx = _load_index_list(used_idxs) if isinstance(used_idxs, str) else [int(i) for i in used_idxs]
    return [rows[i] for i in idx]


def load_frame_folder(directory, frame_indices):
    """`video_loader` + `pil_loader` (:14-18, 36-45): `image_{:05d}.jpg` of every index, decoded by Pillow and converted to
    RGB; the list ENDS at the first missing file (as the reference's loader returns what it has).  uint8 (t,H,W,3)."""
    from PIL import Image
    frames = []
    for i in frame_indices:
        path = os.path.join(directory, "image_{:05d}.jpg".format(i))
        if not os.path.exists(path):
            break
        with open(path, "rb") as fh:
            with Image.open(fh) as img:
                frames.append(np.asarray(img.convert("RGB")))
    if not frames:
        raise FileNotFoundError(f"no frames under {directory} (expected image_{{:05d}}.jpg)")
    return np.stack(frames)


def ucf101_batches(batch_size, setting, image_root, used_idxs=None, frames=32, workers=0):
    """The UCF-101 loader (`attack_genearte_dataeset`, :103-110) up to its spatial transform: yields (uint8 (b,t,H,W,3) decoded
    frames, labels (b,), names) in list order; the caller runs Scale / CornerCrop / ToTensor / Normalize on the device.  `workers`
    decoder threads (Pillow releases the GIL while decoding) with 2 x workers batches in flight -- the reference's DataLoader
    `num_workers=9`.  Clips of one batch must share their frame size (UCF-101: 240 x 320) and length (`frames`, LoopPadding)."""
    rows = ucf101_clip_list(setting, image_root, used_idxs)

    def load(s):
        chunk = rows[s:s + batch_size]
        clips_ = [load_frame_folder(d, loop_padding(list(range(1, dur + 1)), frames)) for d, dur, _ in chunk]     # :66-72
        return (torch.from_numpy(np.stack(clips_)), torch.tensor([t for _, _, t in chunk]),
                [os.path.basename(d) for d, _, _ in chunk])
    starts = list(range(0, len(rows), batch_size))
    yield from _prefetched(load, starts, workers)


def ucf101_num_batches(batch_size, setting, image_root, used_idxs=None):
    return (len(ucf101_clip_list(setting, image_root, used_idxs)) + batch_size - 1) // batch_size


# ---------------------------------------------------------------------------------------------------------------
# Kinetics-400 whole decoded videos (`VideoClsDataset`, `/root/reference/datasets.py`, validation mode): the frame selection of
# `loadvideo_decord` (:216-244) with each row's `clip_index` (:48-51, 138-150), applied to videos decoded ahead of time.  The
# spatial transform runs on the device over the ragged batch (`Engine.clip_gather_resize_crop`).
# The reference reads clip_len / frame_sample_rate / num_segment and the Resize / CenterCrop sizes from gluoncv's
# `i3d_nl5_resnet101_v1_kinetics400.yaml` (image_main.py:55), which it does not ship: 32 / 2 / 1 and 256 / 224 are ASSUMED values
# from that public config, and every one of them is a flag of the CLIs (--frames, --frame_sample_rate, --num_segment,
# --short_side, --hw).
# ---------------------------------------------------------------------------------------------------------------
KINETICS_CLIP_LEN, KINETICS_FRAME_SAMPLE_RATE, KINETICS_NUM_SEGMENT = 32, 2, 1
KINETICS_SHORT_SIDE, KINETICS_CROP = 256, 224


def kinetics_frame_indices(n_frames, clip_ind, clip_len=KINETICS_CLIP_LEN, frame_sample_rate=KINETICS_FRAME_SAMPLE_RATE,
                           num_segment=KINETICS_NUM_SEGMENT):
    """int64 indices of the frames `loadvideo_decord` hands to `vr.get_batch` for a video of `n_frames` frames (validation mode,
    sample_rate_scale = 1), `clip_len * num_segment` of them:
      converted_len = clip_len * frame_sample_rate, seg_len = n_frames // num_segment; per segment i
      short (seg_len <= converted_len): linspace(0, seg_len, seg_len // rate), padded to clip_len with seg_len, clipped to
                                        [0, seg_len - 1] -- the padding repeats the segment's last frame;
      long: end = seg_len - 1 for clip_ind == -1, else randint(converted_len, seg_len) seeded by clip_ind; the clip is
            linspace(end - converted_len, end, clip_len) clipped to [start, end - 1];
      then cast to int64 and shifted by i * seg_len.
    Deliberate difference: the draw comes from a local `np.random.RandomState(clip_ind)` -- the same number as the reference's
    `np.random.seed(clip_ind); np.random.randint(...)` -- and leaves numpy's global random state alone.  A video with fewer frames
    than segments (the reference would clip to [0, -1]) is refused."""
    n_frames, clip_len, rate, nseg = int(n_frames), int(clip_len), int(frame_sample_rate), int(num_segment)
    if clip_len < 1 or rate < 1 or nseg < 1:
        raise ValueError(f"clip_len, frame_sample_rate and num_segment must be >= 1 (got {clip_len}, {rate}, {nseg})")
    if n_frames < 1 or n_frames < nseg:
        raise ValueError(f"a video of {n_frames} frames cannot give {nseg} segment(s)")
    converted_len = clip_len * rate
    seg_len = n_frames // nseg
    out = []
    for i in range(nseg):
        if seg_len <= converted_len:
            index = np.linspace(0, seg_len, num=seg_len // rate)
            index = np.concatenate((index, np.ones(clip_len - seg_len // rate) * seg_len))
            index = np.clip(index, 0, seg_len - 1).astype(np.int64)
        else:
            if clip_ind == -1:
                end_idx = seg_len - 1
            else:
                end_idx = np.random.RandomState(clip_ind).randint(converted_len, seg_len)
            str_idx = end_idx - converted_len
            index = np.linspace(str_idx, end_idx, num=clip_len)
            index = np.clip(index, str_idx, end_idx - 1).astype(np.int64)
        out.append(index + i * seg_len)
    return np.concatenate(out).astype(np.int64)


def kinetics_rows(csv_path, n=400):
    """[(path, gt_label, clip_index)] of the reference's sample list `path,gt_label,clip_index` (datasets.py:48-51)."""
    with open(csv_path) as fh:
        return [(r["path"], int(r["gt_label"]), int(r["clip_index"])) for r in csv.DictReader(fh)][:n]


def kinetics_video_path(video_dir, path):
    """`<video_dir>/<path minus its extension>.npy`: the whole decoded video of a row (VAL_DATA_PATH + path, datasets.py:190)."""
    return os.path.join(video_dir, os.path.splitext(path)[0] + ".npy")


def gather_geometry(sizes, short_side=KINETICS_SHORT_SIDE, crop=KINETICS_CROP):
    """Per clip frame size (H, W) -> the tables of `i2v_clip_gather_resize_crop_u8_f32`: geometry int32 (b, 8) = (H, W, rh, rw,
    crop y, crop x, first xtab row, first ytab row) and the concatenated cv2 resize tables xtab / ytab int32 (rows, 3).  Clips of
    one frame size share their tables."""
    geom, xparts, yparts, seen = [], [], [], {}
    xrows = yrows = 0
    for H, W in sizes:
        H, W = int(H), int(W)
        rh, rw = resize_sizes(H, W, short_side)
        if rh < crop or rw < crop:
            raise ValueError(f"a {H} x {W} frame resized to {rh} x {rw} is smaller than the {crop} x {crop} crop")
        if (H, W) not in seen:
            seen[(H, W)] = (xrows, yrows)
            xparts.append(resize_table(rw, W))
            yparts.append(resize_table(rh, H))
            xrows, yrows = xrows + rw, yrows + rh
        cy, cx = center_crop_origin(rh, rw, crop, crop)
        geom.append((H, W, rh, rw, cy, cx) + seen[(H, W)])
    return np.asarray(geom, np.int32).reshape(-1, 8), np.concatenate(xparts), np.concatenate(yparts)


POOL_ALIGN = 16             # every frame of the pool starts on a 16-byte boundary (the kernel stages rows with 16-byte loads)


def pack_frames(videos, indices, pin=False):
    """Distinct selected frames of each clip, packed once: returns (pool uint8 (bytes,), offsets int64 (b, t)).  `videos[i]` is an
    array-like (N, H, W, 3) uint8 (a memory map reads only the frames asked for); `indices[i]` the clip's frame indices."""
    offsets = np.empty((len(videos), len(indices[0])), np.int64)
    picks, total = [], 0
    for ci, (v, idx) in enumerate(zip(videos, indices)):
        slot = {}
        fbytes = int(np.prod(v.shape[1:]))
        for ti, f in enumerate(idx):
            f = int(f)
            if f not in slot:
                slot[f] = total
                picks.append((ci, f, total, fbytes))
                total += (fbytes + POOL_ALIGN - 1) // POOL_ALIGN * POOL_ALIGN
            offsets[ci, ti] = slot[f]
    pool = torch.empty(max(total, POOL_ALIGN), dtype=torch.uint8, pin_memory=pin)
    host = pool.numpy()
    for ci, f, off, fbytes in picks:
        host[off:off + fbytes] = np.ascontiguousarray(videos[ci][f]).reshape(-1)
    return pool, offsets


def _open_video(video_dir, path, row):
    p = kinetics_video_path(video_dir, path)
    if not os.path.exists(p):
        raise FileNotFoundError(f"row {row} ({path}): no decoded video {p}")
    v = np.load(p, mmap_mode="r")
    if v.dtype != np.uint8 or v.ndim != 4 or v.shape[-1] != 3:
        raise ValueError(f"row {row} ({path}): {p} holds {v.dtype} {v.shape}, expected uint8 (N, H, W, 3)")
    if v.shape[0] == 0:
        raise ValueError(f"row {row} ({path}): {p} holds no frames")
    return v


def kinetics_video_batches(batch_size, csv_path, video_dir, clip_len=KINETICS_CLIP_LEN, frame_sample_rate=KINETICS_FRAME_SAMPLE_RATE,
                           num_segment=KINETICS_NUM_SEGMENT, short_side=KINETICS_SHORT_SIDE, crop=KINETICS_CROP, n=400, workers=0,
                           pin=None):
    """The reference's validation loader over whole decoded videos (datasets.py:138-150, 188-244) up to its spatial transform:
    yields (pool, tables, labels (b,), names) in list order, where pool is one uint8 tensor of the batch's DISTINCT selected frames
    (pinned when a GPU is present) and tables = (offsets int64 (b, t), geometry int32 (b, 8), xtab, ytab) as `gather_geometry`
    describes them; `Engine.clip_gather_resize_crop(pool, offsets, (geometry, xtab, ytab))` gives the (b,3,t,crop,crop) batch.
    Names follow the reference, `path.split(".")[0]` (:150).  Each row's video is `kinetics_video_path(video_dir, path)`, memory
    mapped so that only the selected frames are read.  A missing or empty video is an error naming its row -- where the reference
    draws another row, calls `loadvideo_decord(sample)` without its clip index and dies with a TypeError (:144-147)."""
    rows = kinetics_rows(csv_path, n)
    if pin is None:
        pin = torch.cuda.is_available()

    def load(s):
        chunk = rows[s:s + batch_size]
        videos = [_open_video(video_dir, path, s + i) for i, (path, _, _) in enumerate(chunk)]
        indices = [kinetics_frame_indices(v.shape[0], ci, clip_len, frame_sample_rate, num_segment) for v, (_, _, ci) in zip(videos, chunk)]
        pool, offsets = pack_frames(videos, indices, pin)
        geom, xtab, ytab = gather_geometry([v.shape[1:3] for v in videos], short_side, crop)
        return pool, (offsets, geom, xtab, ytab), torch.tensor([r[1] for r in chunk]), [r[0].split(".")[0] for r in chunk]
    yield from _prefetched(load, list(range(0, len(rows), batch_size)), workers)


def kinetics_num_batches(batch_size, csv_path, n=400):
    return (len(kinetics_rows(csv_path, n)) + batch_size - 1) // batch_size


def _prefetched(load, starts, workers):
    """`load(start)` for every start, in order, on `workers` threads with a window of 2 x workers results in flight."""
    if workers <= 0:
        for s in starts:
            yield load(s)
        return
    import collections
    from concurrent.futures import ThreadPoolExecutor
    with ThreadPoolExecutor(workers) as ex:
        window = collections.deque()
        it = iter(starts)
        for s in it:
            window.append(ex.submit(load, s))
            if len(window) >= 2 * workers:
                break
        while window:
            out = window.popleft().result()
            nxt = next(it, None)
            if nxt is not None:
                window.append(ex.submit(load, nxt))
            yield out
