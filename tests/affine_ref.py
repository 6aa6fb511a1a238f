"""CPU restatement of the affine training augmentation (the contract of jcm_augment_affine in include/jcm.h), in numpy.

Positions, weights and the interpolation are float64, one rounded operation per step in the order the contract writes them; the colour steps are float32 in
the order of DESIGN.md 4.7 (tests/augment_ref.color_f32), except that the contrast mean is summed in the kernels' fixed order (`contrast_mean`: 128 parts
per image, 192 running sums per part, a halving fold), so that it is the same float32 number and the comparison can be bit for bit.  The maps are not
computed here at all: the cells go through the forward map and data.target_heat_maps draws them.
"""
import numpy as np

import joint_cnn_mrf_amd  # noqa: F401
from joint_cnn_mrf_amd import data

f32 = np.float32
HM_FLIP_PERM = np.array([3, 4, 5, 0, 1, 2, 7, 6, 8, 9])
PARTS, RED = 128, 192


def _fold3(red):
    """red [..., 192] -> [..., 3]: slot t += slot t + s for s = 96, 48, ..., 3 (slot t holds channel t % 3)."""
    red = red.copy()
    s = RED // 2
    while s >= 3:
        red[..., :s] += red[..., s:2 * s]
        s //= 2
    return red[..., :3]


def contrast_mean(img, delta):
    """float32 [3]: the mean over the image of float32(img + delta) per channel, as a double sum in the kernels' order, / (H W), rounded."""
    v = (np.asarray(img, f32).reshape(-1) + f32(delta)).astype(np.float64)
    n = v.size
    chunk = (n // 3 + PARTS - 1) // PARTS * 3
    rows = -(-chunk // RED)
    partial = np.zeros((PARTS, 3))
    for p in range(PARTS):
        seg = v[p * chunk:min(n, (p + 1) * chunk)]
        grid = np.zeros(rows * RED)
        grid[:seg.size] = seg
        red = np.zeros(RED)
        for row in grid.reshape(rows, RED):          # running sum t takes elements t, t + 192, ... in ascending order
            red = red + row
        partial[p] = _fold3(red)
    flat = partial.reshape(-1)
    return (_fold3(flat[:RED] + flat[RED:]) / np.float64(n // 3)).astype(f32)


def colour(img, delta, factor):
    """clip(((img + delta) - m) * factor + m, 0, 1), float32 step by step."""
    delta, factor = f32(delta), f32(factor)
    m = contrast_mean(img, delta)
    v = np.asarray(img, f32) + delta
    v = (v - m) * factor + m
    return np.minimum(np.maximum(v, f32(0)), f32(1)).astype(f32)


def sample_image(img, col, g, pad):
    """img [H,W,3] float32, col = (flip, delta, factor), g = the 12 numbers of one geom row -> the augmented image, float32."""
    H, W = img.shape[:2]
    v = colour(img, col[1], col[2]).astype(np.float64)
    padv = np.float64(f32(pad))
    q = np.arange(W, dtype=np.float64)[None, :]
    r = np.arange(H, dtype=np.float64)[:, None]
    with np.errstate(over='ignore', invalid='ignore'):
        xs = (g[0] * q + g[1] * r) + g[2]
        ys = (g[3] * q + g[4] * r) + g[5]
        ok = np.isfinite(xs) & np.isfinite(ys)
        xs, ys = np.where(ok, xs, 0.0), np.where(ok, ys, 0.0)
    x0, y0 = np.floor(xs), np.floor(ys)
    fx, fy = (xs - x0)[..., None], (ys - y0)[..., None]

    def tap(yy, xx):
        inside = (yy >= 0) & (yy <= H - 1) & (xx >= 0) & (xx <= W - 1)
        at = v[np.where(inside, yy, 0).astype(np.int64), np.where(inside, xx, 0).astype(np.int64)]
        return np.where(inside[..., None], at, padv)
    top = (1.0 - fx) * tap(y0, x0) + fx * tap(y0, x0 + 1.0)
    bot = (1.0 - fx) * tap(y0 + 1.0, x0) + fx * tap(y0 + 1.0, x0 + 1.0)
    out = ((1.0 - fy) * top + fy * bot).astype(f32)
    return np.where(ok[..., None], out, f32(pad)).astype(f32)


def move_cells(cells, flip, g, hh, hw):
    """cells [10,2] (row, col) -> the cells of the augmented image's ten channels, by the rule of data.joint_cells."""
    src = np.asarray(cells)[HM_FLIP_PERM] if flip else np.asarray(cells)
    px, py = 8.0 * src[:, 1].astype(np.float64) + 3.5, 8.0 * src[:, 0].astype(np.float64) + 3.5
    with np.errstate(over='ignore', invalid='ignore'):
        qx = (g[6] * px + g[7] * py) + g[8]
        qy = (g[9] * px + g[10] * py) + g[11]
        qx = np.where(qx >= 0, np.where(qx <= 8.0 * hw, qx, 8.0 * hw), 0.0)
        qy = np.where(qy >= 0, np.where(qy <= 8.0 * hh, qy, 8.0 * hh), 0.0)
    return np.stack([(qy / 8.0).astype(np.int64), (qx / 8.0).astype(np.int64)], axis=1)


def augment(x, cells, colour_rows, geom, pad=0.0):
    """x [B,H,W,3] float32, cells [B,10,2], colour_rows [B,3], geom [B,12] -> (x_out float32, y_out float32 [B,H/8,W/8,10], the moved cells [B,10,2])."""
    B, H, W, _ = x.shape
    hh, hw = H // 8, W // 8
    xo = np.stack([sample_image(np.asarray(x[b], f32), colour_rows[b], geom[b], pad) for b in range(B)])
    moved = np.stack([move_cells(cells[b], colour_rows[b][0] == 1, geom[b], hh, hw) for b in range(B)])
    return xo, data.target_heat_maps(moved, hh, hw), moved
