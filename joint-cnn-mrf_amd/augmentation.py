"""Training-time data augmentation (reference: augmentation.py:58-78, applied to x_in / y_in at main.py:494-497).

Per image, in the reference's order: horizontal flip (the heat maps' left / right channels swapped), brightness,
contrast, clip to [0, 1], rotation, crop_and_resize back to the input size, and the heat maps' pow(., 1.6) + 1e-5
renormalisation -- three HIP kernels behind `jcm_augment_train` (csrc/augment.hip; semantics in DESIGN.md 4.7, a
restatement of the TF-1.x ops that is not pinned against a TF run).  The random draws the reference left to TF's
unseeded ops are made on the host from a numpy RandomState (`draw_params`), for the whole global batch before the
towers slice it, so a run is reproducible from its seed and does not depend on the tower count.
"""
import numpy as np
import torch

MAX_ROTATE_ANGLE = np.pi / 9                 # augmentation.py:67
CROP_SIZE = 0.95                             # augmentation.py:40 (relative size of the crop box)
MAX_BRIGHTNESS_DELTA = 32. / 255.            # augmentation.py:69
CONTRAST_LOWER, CONTRAST_UPPER = 0.8, 1.2    # augmentation.py:70
HM_FLIP_PERM = (3, 4, 5, 0, 1, 2, 7, 6, 8, 9)   # augmentation.py:20: heat-map channel k of a flipped image is old channel HM_FLIP_PERM[k]
N_PARAMS = 6                                 # (flip, delta, factor, angle, rh, rw)


def draw_params(rng, B):
    """[B, 6] float32 = (flip, delta, factor, angle, rh, rw) from one rng.random_sample((B, 6)) draw."""
    u = rng.random_sample((int(B), N_PARAMS))
    p = np.empty_like(u)
    p[:, 0] = u[:, 0] > 0.5                                                          # horizontal_flip, :27
    p[:, 1] = -MAX_BRIGHTNESS_DELTA + u[:, 1] * (2 * MAX_BRIGHTNESS_DELTA)           # random_brightness, :69
    p[:, 2] = CONTRAST_LOWER + (CONTRAST_UPPER - CONTRAST_LOWER) * u[:, 2]           # random_contrast, :70
    p[:, 3] = -MAX_ROTATE_ANGLE + u[:, 3] * (2 * MAX_ROTATE_ANGLE)                   # random_rotation, :34
    p[:, 4] = (1 - CROP_SIZE) * u[:, 4]                                              # random_crop rh, :44
    p[:, 5] = (1 - CROP_SIZE) * u[:, 5]                                              # random_crop rw, :45
    return p.astype(np.float32)


def check_params(p):
    """Host-side check of a parameter array: [B, 6], finite, flip 0 or 1.  Returns it as float32; raises ValueError."""
    a = np.asarray(p, dtype=np.float32)
    if a.ndim != 2 or a.shape[1] != N_PARAMS or a.shape[0] < 1:
        raise ValueError('augmentation parameters must be [B, %d], got shape %s' % (N_PARAMS, a.shape))
    if not np.isfinite(a).all():
        raise ValueError('augmentation parameters must be finite')
    if not np.isin(a[:, 0], (0.0, 1.0)).all():
        raise ValueError('augmentation parameter flip (column 0) must be 0 or 1')
    return np.ascontiguousarray(a)


def augment_train(engine, x, y, params):
    """x [B,H,W,3], y [B,h,w,10] device fp32 tensors, params [B,6] (host array) -> (x_aug, y_aug) new device tensors."""
    p = check_params(params)
    pd = torch.from_numpy(p).pin_memory().to(engine.device, non_blocking=True)
    return engine.augment_train(x, y, pd)


# ------------------------------------------------------------------ the affine augmentation (csrc/augment_affine.hip)
# One composed affine sample of the image (flip, rotation, scale, shift; `pad` outside) and target maps redrawn as the data set's 3x3 blobs at the
# transformed joint cells.  Not in the reference: its docstring promises "scale [0.5, 1.5]" (augmentation.py:60-61) but its code has the fixed 0.95 crop.
N_AFFINE_PARAMS = 7                          # (flip, delta, factor, angle, scale, tx, ty)
# The default ranges are those of the reference's docstring.  They are UNTUNED PLACEHOLDERS: no trained weights and no FLIC images were available to
# measure what any range buys in detection rate.
AFFINE_SCALE = (0.5, 1.5)
AFFINE_SHIFT = 0.0


def draw_affine_params(rng, B, scale=AFFINE_SCALE, max_angle=MAX_ROTATE_ANGLE, shift=AFFINE_SHIFT):
    """[B, 7] float64 = (flip, delta, factor, angle, scale, tx, ty) from one rng.random_sample((B, 7)) draw: flip, delta and factor in the ranges of
    draw_params, angle uniform in +-max_angle, scale uniform in [lo, hi], tx / ty uniform in +-shift as fractions of the frame width / height."""
    lo, hi = float(scale[0]), float(scale[1])
    max_angle, shift = float(max_angle), float(shift)
    if not (0 < lo <= hi) or not np.isfinite(hi):
        raise ValueError('scale must be (lo, hi) with 0 < lo <= hi, got %r' % (scale,))
    if not (0 <= shift < 0.5):
        raise ValueError('shift must be in [0, 0.5), got %r' % (shift,))
    if not (0 <= max_angle <= np.pi):
        raise ValueError('max_angle must be in [0, pi], got %r' % (max_angle,))
    u = rng.random_sample((int(B), N_AFFINE_PARAMS))
    p = np.empty_like(u)
    p[:, 0] = u[:, 0] > 0.5
    p[:, 1] = -MAX_BRIGHTNESS_DELTA + u[:, 1] * (2 * MAX_BRIGHTNESS_DELTA)
    p[:, 2] = CONTRAST_LOWER + (CONTRAST_UPPER - CONTRAST_LOWER) * u[:, 2]
    p[:, 3] = -max_angle + u[:, 3] * (2 * max_angle)
    p[:, 4] = lo + u[:, 4] * (hi - lo)
    p[:, 5] = -shift + u[:, 5] * (2 * shift)
    p[:, 6] = -shift + u[:, 6] * (2 * shift)
    return p


def affine_geometry(params, H, W):
    """params [B, 7] (draw_affine_params) for H x W images -> (colour float32 [B, 3] = (flip, delta, factor), geom float64 [B, 12]).

    geom[:, :6] = (a, b, c0, d, e, f0), the inverse map: output pixel (q, r) reads the source at xs = a q + b r + c0, ys = d q + e r + f0, which is
        u = q - cx - tx W,  v = r - cy - ty H,  xs = cx + (c u + s v) / scale,  ys = cy + (-s u + c v) / scale,  with flip xs <- (W - 1) - xs
    (cx, cy = (W - 1) / 2, (H - 1) / 2; c, s = cos, sin of the angle) folded into six numbers.
    geom[:, 6:] = (A, B, C0, D, E, F0), the forward map of a source point (x, y) to its output position qx = A x + B y + C0, qy = D x + E y + F0: the same
    steps undone in reverse order, in closed form -- not a numerical matrix inversion.  All trigonometry of the augmentation happens here, in float64."""
    p = np.asarray(params, np.float64)
    if p.ndim != 2 or p.shape[1] != N_AFFINE_PARAMS or p.shape[0] < 1:
        raise ValueError('affine parameters must be [B, %d], got shape %s' % (N_AFFINE_PARAMS, p.shape))
    H, W = int(H), int(W)
    flip, ang, sc, tx, ty = p[:, 0] == 1.0, p[:, 3], p[:, 4], p[:, 5], p[:, 6]
    cx, cy = (W - 1) / 2.0, (H - 1) / 2.0
    c, s = np.cos(ang), np.sin(ang)
    ox, oy = cx + tx * W, cy + ty * H                 # where the source's centre lands in the output
    g = np.empty((p.shape[0], 12), np.float64)
    a, b, c0 = c / sc, s / sc, cx - (c * ox + s * oy) / sc
    g[:, 0] = np.where(flip, -a, a)
    g[:, 1] = np.where(flip, -b, b)
    g[:, 2] = np.where(flip, (W - 1) - c0, c0)
    g[:, 3] = (-s) / sc
    g[:, 4] = c / sc
    g[:, 5] = cy - ((-s) * ox + c * oy) / sc
    A, D = sc * c, sc * s
    C0, F0 = ox - sc * (c * cx - s * cy), oy - sc * (s * cx + c * cy)
    g[:, 6] = np.where(flip, -A, A)
    g[:, 7] = -(sc * s)
    g[:, 8] = np.where(flip, C0 + A * (W - 1), C0)
    g[:, 9] = np.where(flip, -D, D)
    g[:, 10] = sc * c
    g[:, 11] = np.where(flip, F0 + D * (W - 1), F0)
    return np.ascontiguousarray(p[:, :3], np.float32), g


def check_affine(colour, geom):
    """Host-side check of (colour [B, 3], geom [B, 12]): shapes, finite, flip 0 or 1, both maps non-singular.  Returns them as contiguous float32 / float64
    arrays; raises ValueError."""
    col, g = np.asarray(colour, dtype=np.float32), np.asarray(geom, dtype=np.float64)
    if col.ndim != 2 or col.shape[1] != 3 or col.shape[0] < 1:
        raise ValueError('affine colour parameters must be [B, 3], got shape %s' % (col.shape,))
    if g.ndim != 2 or g.shape[1] != 12 or g.shape[0] != col.shape[0]:
        raise ValueError('affine geometry must be [%d, 12] for %d colour rows, got shape %s' % (col.shape[0], col.shape[0], g.shape))
    if not np.isfinite(col).all() or not np.isfinite(g).all():
        raise ValueError('affine parameters must be finite')
    if not np.isin(col[:, 0], (0.0, 1.0)).all():
        raise ValueError('affine parameter flip (colour column 0) must be 0 or 1')
    det_inv, det_fwd = g[:, 0] * g[:, 4] - g[:, 1] * g[:, 3], g[:, 6] * g[:, 10] - g[:, 7] * g[:, 9]
    with np.errstate(over='ignore', invalid='ignore'):
        if not (np.isfinite(det_inv) & (det_inv != 0) & np.isfinite(det_fwd) & (det_fwd != 0)).all():
            raise ValueError('affine geometry is singular (a map with determinant 0)')
    return np.ascontiguousarray(col), np.ascontiguousarray(g)


MAX_AFFINE_WIDTH = 4.0                       # the widest filter of the antialiased sample (csrc/augment_affine.hip: 9 x 9 taps, scale 0.25)


def affine_footprint(geom):
    """geom [B, 12] -> float64 [B]: the filter half-width of the antialiased sample in source pixels, max(1, sqrt(|a e - b d|)) of the
    inverse map -- how many source pixels an output pixel spans along an axis of a similarity map; 1 where the picture is not shrunk.  The square root is
    taken here, on the host.  The root is rounded to 12 decimals, so that the last-bit rounding of the cosines and sines in geom does not turn scale 1
    into a width a hair above 1 (which would leave the plain four-tap form) or scale 0.25 into one a hair above 4 (which the kernel refuses)."""
    g = np.asarray(geom, dtype=np.float64)
    if g.ndim != 2 or g.shape[1] != 12:
        raise ValueError('affine geometry must be [B, 12], got shape %s' % (g.shape,))
    return np.maximum(1.0, np.round(np.sqrt(np.abs(g[:, 0] * g[:, 4] - g[:, 1] * g[:, 3])), 12))


def check_width(width, B):
    """Host-side check of the filter half-widths of the antialiased sample: [B], finite, in [1, 4].  Returns them as a contiguous float64 array; raises
    ValueError."""
    w = np.asarray(width, dtype=np.float64)
    if w.shape != (int(B),):
        raise ValueError('the filter widths must be [%d], got shape %s' % (B, w.shape))
    if not ((w >= 1.0) & (w <= MAX_AFFINE_WIDTH)).all():      # (a NaN fails both comparisons)
        raise ValueError('a filter width must be finite and in [1, %g] (scale 0.25 at the least); got %s' % (MAX_AFFINE_WIDTH, w[~((w >= 1.0) & (w <= MAX_AFFINE_WIDTH))][:4]))
    return np.ascontiguousarray(w)


def affine_joints_inside(cells, geom, H, W):
    """cells [B, 10, 2] (row, col) heat-map cells, geom [B, 12] -> bool [B]: whether every one of the ten points the cells stand for, (8 col + 3.5,
    8 row + 3.5), lands inside [0, W] x [0, H] under image b's forward map -- i.e. none of them is clamped when the targets are redrawn (the clamp of
    jcm_augment_affine, in its float64 order).  A flip permutes the channels, not the set of points, so it does not enter."""
    c, g = np.asarray(cells), np.asarray(geom, dtype=np.float64)
    if c.ndim != 3 or c.shape[1:] != (10, 2) or g.shape != (c.shape[0], 12):
        raise ValueError('affine_joints_inside expects cells [B,10,2] and geom [B,12]; got %s, %s' % (c.shape, g.shape))
    px, py = 8.0 * c[:, :, 1].astype(np.float64) + 3.5, 8.0 * c[:, :, 0].astype(np.float64) + 3.5
    qx = (g[:, 6:7] * px + g[:, 7:8] * py) + g[:, 8:9]
    qy = (g[:, 9:10] * px + g[:, 10:11] * py) + g[:, 11:12]
    return ((qx >= 0.0) & (qx <= float(W)) & (qy >= 0.0) & (qy <= float(H))).all(axis=1)


class AffineDraw:
    """One batch's draw of the affine augmentation: colour [B, 3], geom [B, 12] (affine_geometry) and the pad value -- what Trainer.train_step(augment=)
    takes besides the [B, 6] array of the reference's augmentation.  draw[lo:hi] is the draw of a tower's slice of the batch.  width: None (the plain
    bilinear sample), or the [B] filter half-widths of the antialiased sample (affine_footprint(geom))."""

    def __init__(self, colour, geom, pad=0.0, width=None):
        self.colour, self.geom = check_affine(colour, geom)
        self.width = None if width is None else check_width(width, self.colour.shape[0])
        self.pad = float(pad)
        if not np.isfinite(self.pad):
            raise ValueError('pad must be finite, got %r' % (pad,))

    def __len__(self):
        return self.colour.shape[0]

    def __getitem__(self, s):
        if not isinstance(s, slice):
            raise TypeError('an AffineDraw is sliced by image ranges, got %r' % (s,))
        return AffineDraw(self.colour[s], self.geom[s], self.pad, None if self.width is None else self.width[s])


def draw_affine(rng, B, H, W, pad=0.0, antialias=False, **ranges):
    """AffineDraw for B images of H x W: draw_affine_params(rng, B, **ranges) through affine_geometry.  antialias: with the filter widths of the
    antialiased sample (the same draw from `rng`; a scale below 0.25 is refused)."""
    colour, geom = affine_geometry(draw_affine_params(rng, B, **ranges), H, W)
    return AffineDraw(colour, geom, pad=pad, width=affine_footprint(geom) if antialias else None)


def fixed_affine(B, H, W, scale, angle=0.0, shift=(0, 0), flip=False, pad=0.0, antialias=True):
    """AffineDraw of ONE geometry for all B images of H x W, the colour left as it is (delta 0, factor 1): scale and angle about the centre, shift =
    (tx, ty) as fractions of the frame width / height (draw_affine_params), the mirrored picture with flip.  What evaluation.eval_curves_affine shows the
    tower; antialias: with the filter widths of the antialiased sample."""
    scale = float(scale)
    if not (0 < scale < np.inf):
        raise ValueError('scale must be positive and finite, got %r' % (scale,))
    p = np.tile(np.array([[1.0 if flip else 0.0, 0.0, 1.0, float(angle), scale, float(shift[0]), float(shift[1])]], np.float64), (int(B), 1))
    colour, geom = affine_geometry(p, H, W)
    return AffineDraw(colour, geom, pad=pad, width=affine_footprint(geom) if antialias else None)


def augment_test(x, y):
    """augmentation.py:81-90: the identity."""
    return x, y
