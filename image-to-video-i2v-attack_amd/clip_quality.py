#!/usr/bin/env python
"""PSNR, SSIM and L-infinity of the adversarial clips of a run directory against their clean clips, measured on the device
(`Engine.clip_quality`, include/i2v_quality.h): pairs `<adv_path>/{label}-adv.npy` with `<clean_dir>/{label}-ori.npy`, writes
`<adv_path>/quality_all_clips.json` (`label -> {psnr_db, ssim, linf_levels}`, as `image_main.py --quality` records them) and prints the
means.  Run directories that already exist can be measured this way.

A float adversarial clip (3,t,h,w) is measured against the float clean clip.  A uint8 one (t,h,w,3) -- `image_main.py --export_u8`,
`--adv_path RUN/u8` -- is measured against the clean clip's frames: a uint8 clean clip as it is, a float one through
`Engine.clip_to_u8`.  `$I2V_OPT_PATH` is joined in front of `--adv_path`, as the evaluator does."""
import argparse
import json
import os

import numpy as np
import torch

from i2v_amd import quality


def measure(eng, adv, clean):
    """One clip pair on the engine's device -> the clip's record."""
    adv, clean = adv.to(eng.device).contiguous(), clean.to(eng.device).contiguous()
    if adv.dtype == torch.uint8:
        if clean.dtype != torch.uint8:
            clean = eng.clip_to_u8(clean[None])[0]
        t, h, w, _ = adv.shape
    else:
        if clean.dtype == torch.uint8:
            clean = eng.clip_from_u8(clean[None])[0]
        _, t, h, w = adv.shape
        adv, clean = adv[None], clean[None]
    rows = eng.clip_quality(adv, clean).cpu()
    return quality.summarise(rows, t, h, w)[0]


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--adv_path", type=str, required=True, help="directory of {label}-adv.npy, float32 (3,t,h,w) or uint8 (t,h,w,3)")
    ap.add_argument("--clean_dir", type=str, required=True, help="directory of {label}-ori.npy clean clips")
    ap.add_argument("--gpu", type=str, default="0", help="gpu device.")
    args = ap.parse_args(argv)
    from i2v_amd import attacks as _attacks
    if "LOCAL_RANK" not in os.environ:
        os.environ["LOCAL_RANK"] = args.gpu.split(",")[0]
    eng = _attacks.get_engine()
    adv_path = os.path.join(os.environ.get("I2V_OPT_PATH", ""), args.adv_path)
    files = sorted(f for f in os.listdir(adv_path) if f.endswith("-adv.npy"))
    out = {}
    for f in files:
        label = f[:-len("-adv.npy")]
        adv = torch.from_numpy(np.load(os.path.join(adv_path, f)))
        clean = torch.from_numpy(np.load(os.path.join(args.clean_dir, f"{label}-ori.npy")))
        out[label] = measure(eng, adv, clean)
    with open(os.path.join(adv_path, "quality_all_clips.json"), "w") as fh:
        json.dump(out, fh)
    if out:
        psnr = [r["psnr_db"] for r in out.values() if r["psnr_db"] is not None]
        print("clips {}: PSNR {} dB  SSIM {:.6f}  L-inf {:.3f} levels".format(
            len(out), "{:.3f}".format(sum(psnr) / len(psnr)) if psnr else "inf", sum(r["ssim"] for r in out.values()) / len(out),
            max(r["linf_levels"] for r in out.values())))
    return out


if __name__ == "__main__":
    main()
