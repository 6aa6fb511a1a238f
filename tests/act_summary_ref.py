"""numpy restatement of Engine.act_summary (csrc/act_summary.hip) and of the tag list of summary.activation_summaries.
Shares no code with the package: its own bucket table, grouping and tag names."""
import math
import sys

import numpy as np

N_BUCKETS = 1551
SCOPES = ['conv1_fullres', 'conv2_fullres', 'conv3_fullres', 'conv4_fullres',
          'conv1_halfres', 'conv2_halfres', 'conv3_halfres', 'conv4_halfres',
          'conv1_quarterres', 'conv2_quarterres', 'conv3_quarterres', 'conv4_quarterres', 'conv5', 'conv6']      # main.py:44-72, in call order


def limits():
    """histogram.cc InitDefaultBucketsInner: 1e-12 * 1.1^k below 1e20, DBL_MAX, mirrored, 0.0 in the middle."""
    pos, v = [], 1.0e-12
    while v < 1.0e20:
        pos.append(v)
        v = v * 1.1
    pos.append(sys.float_info.max)
    return np.array([-p for p in pos[::-1]] + [0.0] + pos, np.float64)


def groups(n_images, n_groups):
    """[(first, last + 1)] of the groups of n_images // n_groups consecutive images; the trailing remainder belongs to no group."""
    if n_groups < 1 or n_images < n_groups:
        raise ValueError('%d images do not fill %d groups' % (n_images, n_groups))
    per = n_images // n_groups
    return [(g * per, (g + 1) * per) for g in range(n_groups)]


def stats(z, n_groups, lim=None):
    """Per group of the float32 tensor z [B,...]: dict of min, max (float64 of the float32 extremes over the finite values; DBL_MAX / -DBL_MAX
    when there are none), num, n_pos, n_nonfinite, buckets [1551], and the exact sums sum, sum_squares (math.fsum) with the bounds
    n * 2^-52 * sum|v| and n * 2^-52 * sum v^2 that any order of double additions keeps."""
    lim = limits() if lim is None else lim
    z = np.asarray(z, np.float32)
    out = []
    for lo, hi in groups(z.shape[0], n_groups):
        v = z[lo:hi].reshape(-1)
        fin = v[np.isfinite(v)].astype(np.float64)
        sq = fin * fin
        out.append({
            'min': float(fin.min()) if fin.size else sys.float_info.max,
            'max': float(fin.max()) if fin.size else -sys.float_info.max,
            'num': int(fin.size), 'n_pos': int((fin > 0).sum()), 'n_nonfinite': int(v.size - fin.size),
            'buckets': np.bincount(np.searchsorted(lim, fin, 'right'), minlength=N_BUCKETS).astype(np.int64),
            'sum': math.fsum(fin.tolist()), 'sum_squares': math.fsum(sq.tolist()),
            'sum_bound': fin.size * 2.0 ** -52 * math.fsum(np.abs(fin).tolist()), 'sum_squares_bound': fin.size * 2.0 ** -52 * math.fsum(sq.tolist()),
            'size': int(v.size)})
    return out


def fold64(gamma, beta, mean, var, eps=1e-3):
    """The inference-mode BatchNorm folded in float64 and rounded once: (scale, shift) float32."""
    g, b, m, v = (np.asarray(t, np.float64) for t in (gamma, beta, mean, var))
    sc = g / np.sqrt(v + eps)
    return sc.astype(np.float32), (b - m * sc).astype(np.float32)


def activation(z, scale, shift):
    """float32(float32(relu(z)) * scale[c]) + shift[c] in float32, two rounded operations; relu keeps a NaN (tf.nn.relu)."""
    z = np.asarray(z, np.float32)
    with np.errstate(invalid='ignore', over='ignore'):
        r = np.where(z > 0, z, np.where(np.isnan(z), z, np.float32(0))).astype(np.float32)
        m = (r * np.asarray(scale, np.float32)).astype(np.float32)
        return (m + np.asarray(shift, np.float32)).astype(np.float32)


def pictures(activ, n_groups, channel, n_pics):
    """[n_groups, n_pics, H, W]: channel `channel` of the first n_pics images of every group."""
    return np.stack([activ[lo:lo + n_pics, :, :, channel] for lo, _ in groups(activ.shape[0], n_groups)])


def tags(n_towers, per_tower, scopes=SCOPES):
    out = []
    for i in range(n_towers):
        for s in scopes:
            out += ['tower_%d/pre_activ_%s/%s' % (i, s, k) for k in ('max', 'mean', 'min', 'std', 'n_pos', 'histogram')]
            out += ['tower_%d/f_activ_%s/image/%d' % (i, s, k) for k in range(min(3, per_tower))]
    return out
