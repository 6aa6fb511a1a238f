"""CPU restatement of the antialiased affine sample (the contract of jcm_augment_affine_aa in include/jcm.h), in numpy float64.

The image recurrence is written pixel by pixel in the kernel's order -- ascending rows j, within a row ascending columns i, one rounded operation per
step: row = row + tx_i * u, acc = acc + ty_j * row, out = float32(acc / (Sx * Sy)) -- with none of the kernel's short cuts: every pixel walks its taps,
a pixel whose taps all miss the source included.  The colour step, the contrast mean and the maps are those of tests/affine_ref.py; an image of width
exactly 1 is affine_ref.sample_image itself, as the contract says.
"""
import math

import numpy as np

import affine_ref as R

f32 = np.float32


def triangle_taps(p, w):
    """The taps of one axis around position p for half-width w: [(index, weight)] in ascending order, weights 1 - |p - i| / w, those <= 0 left out."""
    taps = []
    for i in range(int(math.ceil(p - w)), int(math.floor(p + w)) + 1):
        t = 1.0 - abs(p - float(i)) / w
        if t > 0.0:
            taps.append((i, t))
    return taps


def sample_values(v, g, w, pad, count=None):
    """v [H,W,C] float64 source values (already colour-transformed), g the 12 numbers of a geom row, w the half-width, pad -> float32 [H,W,C].
    count: an optional int array [H,W] that receives the number of taps of every pixel."""
    H, W, C = v.shape
    padv = float(f32(pad))
    out = np.empty((H, W, C), f32)
    g = [float(t) for t in g]
    for r in range(H):
        for q in range(W):
            xs = (g[0] * float(q) + g[1] * float(r)) + g[2]
            ys = (g[3] * float(q) + g[4] * float(r)) + g[5]
            if not (math.isfinite(xs) and math.isfinite(ys)):
                out[r, q] = f32(pad)
                continue
            cols, rows = triangle_taps(xs, w), triangle_taps(ys, w)
            Sx = 0.0
            for _, tx in cols:
                Sx = Sx + tx
            Sy = 0.0
            acc = [0.0] * C
            for j, ty in rows:
                Sy = Sy + ty
                row = [0.0] * C
                for i, tx in cols:
                    inside = 0 <= i < W and 0 <= j < H
                    for k in range(C):
                        row[k] = row[k] + tx * (float(v[j, i, k]) if inside else padv)
                for k in range(C):
                    acc[k] = acc[k] + ty * row[k]
            S = Sx * Sy
            for k in range(C):
                out[r, q, k] = f32(acc[k] / S)
            if count is not None:
                count[r, q] = len(cols) * len(rows)
    return out


def taps_inside(g, w, H, W):
    """bool [H,W]: the output pixels all of whose taps (of positive weight) lie inside the H x W source."""
    ok = np.zeros((H, W), bool)
    for r in range(H):
        for q in range(W):
            xs = (g[0] * float(q) + g[1] * float(r)) + g[2]
            ys = (g[3] * float(q) + g[4] * float(r)) + g[5]
            cols, rows = triangle_taps(xs, w), triangle_taps(ys, w)
            ok[r, q] = cols[0][0] >= 0 and cols[-1][0] <= W - 1 and rows[0][0] >= 0 and rows[-1][0] <= H - 1
    return ok


def sample_image(img, col, g, w, pad):
    """img [H,W,3] float32, col = (flip, delta, factor), g one geom row, w its filter half-width -> the augmented image, float32."""
    if w == 1.0:
        return R.sample_image(img, col, g, pad)
    return sample_values(R.colour(img, col[1], col[2]).astype(np.float64), g, float(w), pad)


def augment(x, cells, colour_rows, geom, width, pad=0.0):
    """x [B,H,W,3] float32, cells [B,10,2], colour_rows [B,3], geom [B,12], width [B] -> (x_out float32, y_out float32 [B,H/8,W/8,10], the moved cells)."""
    B, H, W, _ = x.shape
    hh, hw = H // 8, W // 8
    xo = np.stack([sample_image(np.asarray(x[b], f32), colour_rows[b], geom[b], width[b], pad) for b in range(B)])
    moved = np.stack([R.move_cells(cells[b], colour_rows[b][0] == 1, geom[b], hh, hw) for b in range(B)])
    return xo, R.data.target_heat_maps(moved, hh, hw), moved
