"""numpy restatement of the reference's det_rate (evaluation.py:15-36) as curves: the arithmetic line by line in explicit float32
operations, every joint and every radius kept instead of one mean.  What jcm_det_curve (csrc/det_curve.hip) is held to bit for bit:
every step is one correctly rounded float32 operation on integers that float32 holds exactly."""
import numpy as np


def argmax_coords(y, K):
    """evaluation.py:15-24 on y[..., :K]: first-occurrence flat arg-max per (image, joint) -> int32 [B,2,K] (row, col).  The rule of the
    library's arg-max kernels, which start from (-inf, no pixel) and take a value when it is larger, or equal at a lower index: the largest
    non-NaN value wins (-inf included: a map of NaN and -inf gives its first -inf), ties go to the lower index, a map of NaN only gives (0,0)."""
    B, H, W = y.shape[:3]
    hm = np.asarray(y, np.float32)[..., :K].reshape(B, H * W, K)                      # :18
    nan = np.isnan(hm)
    hm = np.where(nan, np.float32(-np.inf), hm)
    raw = np.argmax(hm, axis=1)                                                       # :19  [B,K]
    raw = np.where(hm.max(axis=1) == -np.inf, np.argmax(~nan, axis=1), raw)           # nothing above -inf: the first entry that is no NaN (0 if none)
    rows = raw // W                                                                   # :21
    cols = raw - rows * W                                                             # :22
    return np.stack([rows, cols], axis=1).astype(np.int32)                            # :23


def det_curve(pred, y, radii):
    """pred int [B,2,K] (row, col), y [B,H,W,C >= K] targets, radii [R] -> (true int32 [B,2,K], nd float32 [B,K], counts int64 [K,R])."""
    pred = np.asarray(pred).astype(np.int64)
    K = pred.shape[2]
    radii = np.asarray(radii, np.float32).reshape(-1)
    true = argmax_coords(y, K)
    t = true.astype(np.int64)
    lhip_idx, rsho_idx = 0, 7                                                         # :26
    d = t[:, :, lhip_idx] - t[:, :, rsho_idx]                                         # [B,2]
    torso = np.sqrt((d * d).sum(axis=1).astype(np.float32))                           # :29  [B]
    e = pred - t
    dist = np.sqrt((e * e).sum(axis=1).astype(np.float32))                            # :30  [B,K]
    assert torso.dtype == np.float32 and dist.dtype == np.float32
    with np.errstate(divide='ignore', invalid='ignore'):
        nd = (dist * np.float32(100)) / torso[:, None]
    assert nd.dtype == np.float32
    hit = nd[:, :, None] <= radii[None, None, :]                                      # :36 before the mean; inf / NaN: never
    return true, nd, hit.sum(axis=0).astype(np.int64)


def same_floats(a, b):
    """Bit equality of two float32 arrays, NaN matching NaN."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    if a.shape != b.shape or not np.array_equal(np.isnan(a), np.isnan(b)):
        return False
    fin = ~np.isnan(a)
    return np.array_equal(a[fin].view(np.uint32), b[fin].view(np.uint32))


def blob_targets(rs, B, H, W, C, noisy=()):
    """3x3 binomial blobs at seeded random cells, clipped at the border as data.target_heat_maps clips them; channels listed in `noisy` get
    uniform noise below the blob's peak (0.25) under the blob."""
    kern = np.outer([1, 2, 1], [1, 2, 1]).astype(np.float32) / 16
    y = np.zeros((B, H + 2, W + 2, C), np.float32)
    for b in range(B):
        for c in range(C):
            if c in noisy:
                y[b, :, :, c] = rs.uniform(0, 0.2, (H + 2, W + 2)).astype(np.float32)
            r, q = rs.randint(0, H), rs.randint(0, W)
            y[b, r:r + 3, q:q + 3, c] = kern
    return np.ascontiguousarray(y[:, 1:H + 1, 1:W + 1])


def displaced(rs, true, H, W, lo=-6, hi=6):
    """The true cells moved by seeded offsets in lo..hi, clamped to the map -> int32 [B,2,K]."""
    p = true.astype(np.int64) + rs.randint(lo, hi + 1, true.shape)
    p[:, 0] = np.clip(p[:, 0], 0, H - 1)
    p[:, 1] = np.clip(p[:, 1], 0, W - 1)
    return p.astype(np.int32)
