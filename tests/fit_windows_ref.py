"""The fit of a window of an image restated (include/jcm.h: jcm_fit_windows): the padded crop, then tests/fit_ref.py's float64
letterbox fit of it.  The filter is fit_ref's; nothing here restates it, and nothing is shared with the library."""
import numpy as np

import fit_ref as F


def window(img, y0, x0, h, w, pad=0):
    """uint8 [h,w,C]: rows [y0, y0 + h) and columns [x0, x0 + w) of img, the byte `pad` where img has no sample (np.pad, then a crop)."""
    H, W, C = img.shape
    out = np.full((h, w, C), pad, np.uint8)
    ya, yb, xa, xb = max(y0, 0), min(y0 + h, H), max(x0, 0), min(x0 + w, W)
    if ya < yb and xa < xb:
        out[ya - y0:yb - y0, xa - x0:xb - x0] = img[ya:yb, xa:xb]
    return out


def fit_window(img, y0, x0, h, w, OH, OW, pad=0):
    """(uint8 [OH,OW,C], (y0, x0, ch, cw)): fit_ref.fit of the padded window."""
    return F.fit(window(img, y0, x0, h, w, pad), OH, OW, pad)


def fit_windows(images, windows, OH, OW, pad=0):
    """windows: rows (image index, y0, x0, h, w) -> (uint8 [NW,OH,OW,C], int32 [NW,4])."""
    outs, geoms = zip(*(fit_window(images[int(i)], int(y0), int(x0), int(h), int(w), OH, OW, pad) for i, y0, x0, h, w in windows))
    return np.stack(outs), np.array(geoms, np.int32)


def desc7(desc3, windows):
    """fit_ref.pack's desc [B,3] and windows [NW,5] -> the int64 [NW,7] rows jcm_fit_windows takes."""
    windows = np.asarray(windows, np.int64).reshape(-1, 5)
    return np.ascontiguousarray(np.concatenate([np.asarray(desc3, np.int64)[windows[:, 0]], windows[:, 1:]], axis=1))
