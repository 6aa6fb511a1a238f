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


def augment_test(x, y):
    """augmentation.py:81-90: the identity."""
    return x, y
