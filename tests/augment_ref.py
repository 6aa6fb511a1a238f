"""CPU restatements of the training-time augmentation (augmentation.py:58-78 of the reference).

TensorFlow is not available, so these restate the TF-1.x ops the reference calls (flip_left_right, adjust_brightness,
adjust_contrast, clip_by_value, contrib.image.rotate BILINEAR = ImageProjectiveTransform, crop_and_resize, the heat-map
renormalisation).  Like the rest of the oracle they are not pinned against a TF run.

(a) `augment_f32`: float32, step by step, in the operation order of the kernels (csrc/augment.hip) -- the GPU results
    reproduce it to the last bit except for powf (one ulp) and, very rarely, the rounding of a double sum to float32.
(b) `augment_f64`: float64 arithmetic; the rotation by scipy.ndimage.map_coordinates (order 1, zero fill), the crop by an
    explicit float64 bilinear.  Both formulations sample at the float32 positions TF computes (the rotation grid (yi, xi)
    and the crop's in_y / in_x are part of the ops' definition); what differs is the interpolation and the colour arithmetic.
"""
import numpy as np

f32 = np.float32
HM_FLIP_PERM = np.array([3, 4, 5, 0, 1, 2, 7, 6, 8, 9])      # augmentation.py:20
CROP_SIZE = 0.95                                              # augmentation.py:40


# ------------------------------------------------------------------ sampling positions (float32, as TF computes them)
def rot_grid(angle, h, w):
    """(yi, xi) [h, w] float32: the input position read by output pixel (r, q) (angles_to_projective_transforms)."""
    c, s = f32(np.cos(np.float64(angle))), f32(np.sin(np.float64(angle)))
    wm, hm = f32(w - 1), f32(h - 1)
    x_off = (wm - (c * wm - s * hm)) / f32(2)
    y_off = (hm - (s * wm + c * hm)) / f32(2)
    q = np.arange(w, dtype=f32)[None, :]
    r = np.arange(h, dtype=f32)[:, None]
    xi = (c * q + (-s) * r) + x_off
    yi = (s * q + c * r) + y_off
    return yi, xi


def crop_axis(b1, n, crop_size=CROP_SIZE):
    """in_y (or in_x) [n] float32 of crop_and_resize for the box edge b1 and crop extent crop_size, resized back to n."""
    b1 = f32(b1)
    b2 = f32(b1 + f32(crop_size))
    nm = f32(n - 1)
    scale = ((b2 - b1) * nm) / nm
    return b1 * nm + np.arange(n, dtype=f32) * scale


# ------------------------------------------------------------------ (a) float32
def rotate_f32(img, angle):
    """ImageProjectiveTransform, BILINEAR, fill 0; img [h, w, C] float32."""
    h, w = img.shape[:2]
    yi, xi = rot_grid(angle, h, w)
    ok = np.isfinite(xi) & np.isfinite(yi)
    xi, yi = np.where(ok, xi, f32(0)), np.where(ok, yi, f32(0))
    x0, y0 = np.floor(xi), np.floor(yi)
    x1, y1 = x0 + f32(1), y0 + f32(1)

    def P(yy, xx):
        inb = (yy >= 0) & (yy < h) & (xx >= 0) & (xx < w)
        v = img[np.where(inb, yy, 0).astype(np.int64), np.where(inb, xx, 0).astype(np.int64)]
        return np.where(inb[..., None], v, f32(0))
    e = lambda a: a[..., None]
    top = e(x1 - xi) * P(y0, x0) + e(xi - x0) * P(y0, x1)
    bot = e(x1 - xi) * P(y1, x0) + e(xi - x0) * P(y1, x1)
    out = e(y1 - yi) * top + e(yi - y0) * bot
    return np.where(e(ok), out, f32(0)).astype(f32)


def crop_resize_f32(img, rh, rw, crop_size=CROP_SIZE):
    """tf.image.crop_and_resize of the box [rh, rw, rh + crop_size, rw + crop_size] back to img's own size; extrapolation 0."""
    h, w = img.shape[:2]
    in_y, in_x = crop_axis(rh, h, crop_size), crop_axis(rw, w, crop_size)
    vy, vx = (in_y >= 0) & (in_y <= f32(h - 1)), (in_x >= 0) & (in_x <= f32(w - 1))
    in_y, in_x = np.where(vy, in_y, f32(0)), np.where(vx, in_x, f32(0))
    top, bot = np.floor(in_y).astype(np.int64), np.ceil(in_y).astype(np.int64)
    lef, rig = np.floor(in_x).astype(np.int64), np.ceil(in_x).astype(np.int64)
    ly = (in_y - np.floor(in_y))[:, None, None]
    lx = (in_x - np.floor(in_x))[None, :, None]
    tl, tr = img[top][:, lef], img[top][:, rig]
    bl, br = img[bot][:, lef], img[bot][:, rig]
    t = tl + (tr - tl) * lx
    b = bl + (br - bl) * lx
    out = t + (b - t) * ly
    return np.where((vy[:, None] & vx[None, :])[..., None], out, f32(0)).astype(f32)


def flip(img, hm):
    """random_flip: columns reversed, heat-map channel k <- old channel HM_FLIP_PERM[k]."""
    return img[:, ::-1], hm[:, ::-1][:, :, HM_FLIP_PERM]


def color_f32(img, delta, factor):
    """adjust_brightness, adjust_contrast (mean as a double sum rounded to float32), clip to [0, 1]."""
    v = img + f32(delta)
    m = (v.astype(np.float64).sum(axis=(0, 1)) / np.float64(v.shape[0] * v.shape[1])).astype(f32)
    v = (v - m) * f32(factor) + m
    return np.minimum(np.maximum(v, f32(0)), f32(1)).astype(f32)


def renorm_f32(hm):
    t = np.power(hm, f32(1.6)) + f32(1e-5)
    return (t / t.astype(np.float64).sum(axis=(0, 1)).astype(f32)).astype(f32)


def augment_one_f32(img, hm, p, crop_size=CROP_SIZE):
    fl, delta, factor, angle, rh, rw = [f32(v) for v in p]
    x, y = flip(img, hm) if fl == 1 else (img, hm)
    v = color_f32(x, delta, factor)
    v = crop_resize_f32(rotate_f32(v, angle), rh, rw, crop_size)
    y = crop_resize_f32(rotate_f32(y, angle), rh, rw, crop_size)
    return v, renorm_f32(y)


def augment_f32(x, y, params):
    """x [B,H,W,3], y [B,h,w,10], params [B,6] -> (x_aug, y_aug), float32."""
    out = [augment_one_f32(np.asarray(x[b], f32), np.asarray(y[b], f32), params[b]) for b in range(x.shape[0])]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


# ------------------------------------------------------------------ (b) float64
def rotate_f64(img, angle):
    from scipy import ndimage
    h, w = img.shape[:2]
    yi, xi = rot_grid(angle, h, w)
    coords = np.stack([yi.astype(np.float64), xi.astype(np.float64)])
    return np.stack([ndimage.map_coordinates(img[..., k].astype(np.float64), coords, order=1, mode='grid-constant', cval=0.0)
                     for k in range(img.shape[2])], axis=-1)


def crop_resize_f64(img, rh, rw, crop_size=CROP_SIZE):
    """Weights (1 - l, l) on the floor / ceil taps, rows and columns outside the image 0."""
    h, w = img.shape[:2]
    img = np.asarray(img, np.float64)
    in_y, in_x = crop_axis(rh, h, crop_size).astype(np.float64), crop_axis(rw, w, crop_size).astype(np.float64)
    vy, vx = (in_y >= 0) & (in_y <= h - 1), (in_x >= 0) & (in_x <= w - 1)
    in_y, in_x = np.where(vy, in_y, 0.0), np.where(vx, in_x, 0.0)
    y0, y1 = np.floor(in_y).astype(np.int64), np.ceil(in_y).astype(np.int64)
    x0, x1 = np.floor(in_x).astype(np.int64), np.ceil(in_x).astype(np.int64)
    ly, lx = (in_y - y0)[:, None, None], (in_x - x0)[None, :, None]
    rows0 = (1 - lx) * img[y0][:, x0] + lx * img[y0][:, x1]
    rows1 = (1 - lx) * img[y1][:, x0] + lx * img[y1][:, x1]
    out = (1 - ly) * rows0 + ly * rows1
    return np.where((vy[:, None] & vx[None, :])[..., None], out, 0.0)


def augment_one_f64(img, hm, p):
    fl, delta, factor, angle, rh, rw = [float(f32(v)) for v in p]
    x = np.asarray(img, np.float64)
    y = np.asarray(hm, np.float64)
    if fl == 1:
        x, y = flip(x, y)
    v = x + delta
    m = v.mean(axis=(0, 1))
    v = np.clip((v - m) * factor + m, 0.0, 1.0)
    v = crop_resize_f64(rotate_f64(v, angle), rh, rw)
    t = crop_resize_f64(rotate_f64(y, angle), rh, rw) ** 1.6 + 1e-5
    return v, t / t.sum(axis=(0, 1))


def augment_f64(x, y, params):
    out = [augment_one_f64(x[b], y[b], params[b]) for b in range(x.shape[0])]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])
