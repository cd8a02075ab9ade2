"""Host arithmetic on the per-frame figures of `Engine.clip_quality` (include/i2v_quality.h): (SSE in level^2, max |a - b| in levels,
mean SSIM) per frame -> PSNR, SSIM and L-infinity per clip.  Nothing here touches a frame: the frames are measured on the device."""
import math
from typing import List, Optional


def psnr_db(sse: float, count: int) -> Optional[float]:
    """10 log10(255^2 / (sse / count)) for `count` 8-bit elements; None (JSON null) where the operands are identical."""
    if sse <= 0:
        return None
    return 10.0 * math.log10(255.0 * 255.0 * count / sse)


def summarise(per_frame, t: int, h: int, w: int) -> List[dict]:
    """per_frame: (clips * t, 3) rows of (SSE, max, SSIM), frame clip * t + f -> one record per clip: `psnr_db` from the clip's total
    SSE over its 3 t h w elements, `ssim` the mean of the frame values, `linf_levels` the maximum."""
    rows = [[float(v) for v in r] for r in (per_frame.tolist() if hasattr(per_frame, "tolist") else per_frame)]
    if t <= 0 or len(rows) % t != 0:
        raise ValueError(f"{len(rows)} frames do not make clips of {t}")
    out = []
    for i in range(0, len(rows), t):
        clip = rows[i:i + t]
        out.append({"psnr_db": psnr_db(math.fsum(r[0] for r in clip), 3 * t * h * w),
                    "ssim": math.fsum(r[2] for r in clip) / t,
                    "linf_levels": max(r[1] for r in clip)})
    return out


def epsilon_levels(epsilon: float) -> int:
    """The L-infinity budget in whole levels: floor(255 epsilon + 1e-3) (16 / 255 -> 16, 0.05 -> 12)."""
    return int(math.floor(255.0 * epsilon + 1e-3))
