"""Shapes and float64 references of the front-end tests (test_gpu_front_end.py, test_front_end_cpu.py): conv1_<res> + pool1 and, on bf16 handles,
conv2_<res> + pool2, as the tower runs them (csrc/conv1_mfma.hip, csrc/pd_tower.hip: conv1_pool_stage, pool2_layout).  No GPU is needed here."""
import functools

import numpy as np

from joint_cnn_mrf_amd import synth
from oracle import jcm_oracle as O

PATCH = 16      # CM_T: a work group of the fused kernels owns PATCH x PATCH conv outputs (8 x 8 pooled pixels, a 35 x 35 input window)

# (H, W) AFTER sub-sampling -> what the row is in the table for.  `fused`: both extents are multiples of 4, so the 64-filter layer runs on one of the
# fused MFMA kernels; the others take conv1_5x5s2_kernel + the 2x2 pool.  The claims are checked, with the launcher's formulas, by test_front_end_cpu.py.
SHAPES = (
    dict(hw=(4, 4), fused=True, patches=(1, 1), last=(2, 2), pooled=(1, 1), why='one conv 2x2, pooled 1x1: a patch that is almost all store mask'),
    dict(hw=(8, 36), fused=True, patches=(1, 2), last=(4, 2), pooled=(2, 9), why='the second patch column holds 2 conv columns, so ONE pooled column'),
    dict(hw=(36, 32), fused=True, patches=(2, 1), last=(2, 16), pooled=(9, 8), why='the second patch row holds 2 conv rows, so ONE pooled row'),
    dict(hw=(32, 32), fused=True, patches=(1, 1), last=(16, 16), pooled=(8, 8), why='exactly one patch, no mask at all'),
    dict(hw=(64, 96), fused=True, patches=(2, 3), last=(16, 16), pooled=(16, 24), why='fills 2 x 3 patches to the last pixel'),
    dict(hw=(60, 92), fused=True, patches=(2, 3), last=(14, 14), pooled=(15, 23), why='last patches 14 of 16 in both directions; odd pooled extents'),
    dict(hw=(120, 184), fused=True, patches=(4, 6), last=(12, 12), pooled=(30, 46), why='interior patches with neighbours on every side (4 x 6), last ones 12 of 16'),
    dict(hw=(30, 44), fused=False, patches=None, last=None, pooled=(8, 11), why='H % 4 != 0: generic conv (rows padded 1 before / 2 after) + pool of an odd height (15)'),
    dict(hw=(30, 45), fused=False, patches=None, last=None, pooled=(8, 12), why='neither extent a multiple of 4: odd width (columns padded 2 / 2), pool of odd height and width (15 x 23)'),
)
SUBS = (1, 2, 4)      # the image is sub * H x sub * W; the kernels read pixel (gy * sub, gx * sub)
BATCHES = (1, 3)
RES_OF_SUB = {1: 'fullres', 2: 'halfres', 4: 'quarterres'}

# the persistent loop: more patches than a 256-thread kernel can have resident (8 work groups on each of 256 CUs), so every launch walks t += gridDim.x
PERSISTENT = dict(B=160, hw=(128, 128), compare=(0, 1, 79, 159), resident_max=8 * 256)


def conv1_geometry(H, W):
    """The launchers' arithmetic (conv1_mfma.hip: conv1_mfma_pool*), restated, for sub-sampled extents that are multiples of 4."""
    Ho, Wo = H // 2, W // 2
    tiles_y, tiles_x = -(-Ho // PATCH), -(-Wo // PATCH)
    return dict(conv=(Ho, Wo), pooled=(Ho // 2, Wo // 2), patches=(tiles_y, tiles_x), last=(Ho - PATCH * (tiles_y - 1), Wo - PATCH * (tiles_x - 1)),
                pad=(((Ho - 1) * 2 + 5 - H) // 2, ((Wo - 1) * 2 + 5 - W) // 2))


def fused_name_rule(H, W):
    """jcm_conv_kernel_name for a Cin == 3 layer with the packed 64-filter image: fused where this holds (H, W: the layer's own input extents)."""
    return H % 4 == 0 and W % 4 == 0


def tower_takes_fused(H0, W0, sub):
    """The tower's size condition on the image it reads at every sub-th pixel (pd_tower.hip, conv1_pool_stage)."""
    return H0 % sub == 0 and W0 % sub == 0 and (H0 // sub) % 4 == 0 and (W0 // sub) % 4 == 0


@functools.lru_cache(maxsize=None)
def front_end_params(seed=3):
    """conv1 .. conv3 of the three branches at full width (64 / 128 / 256 filters), BatchNorm 'trained'; the biases -- zero at initialisation -- are given
    seeded values, so that a dropped or misplaced bias shows.  Made once and shared: callers leave it unchanged."""
    full = synth.make_pd_params(debug=False, bn='trained')
    rs = np.random.RandomState(seed)
    p = {}
    for name in sorted(full):
        if name.startswith(('conv1_', 'conv2_', 'conv3_')):
            p[name] = full[name]
            if name.endswith('/biases'):
                p[name] = (0.1 * rs.standard_normal(full[name].shape)).astype(np.float32)
    return p


def conv1_pool_ref(x, p, scope, sub=1, emulate=None):
    """float64 pool1(conv1(x[:, ::sub, ::sub])); emulate='bf16': the arithmetic of a bf16 handle (rounding commutes with max: pool-then-round = round-then-pool)."""
    return O.max_pool_same(O.conv_layer(np.asarray(x, np.float64)[:, ::sub, ::sub], p, 5, 2, scope, emulate=emulate))


def conv2_pool_ref(p1, p, scope):
    """float64 pool2(conv2(p1)) in the arithmetic of a bf16 handle."""
    return O.max_pool_same(O.conv_layer(np.asarray(p1, np.float64), p, 5, 1, scope, emulate='bf16'))


def conv1_pool_torch(x, p, scope):
    """The same function by another road: torch conv2d in float64 with explicit asymmetric SAME padding, then max_pool2d with ceil_mode."""
    import torch
    import torch.nn.functional as F
    xt = torch.as_tensor(np.asarray(x, np.float64)).permute(0, 3, 1, 2)
    H, W = xt.shape[2], xt.shape[3]
    th, tw = max((-(-H // 2) - 1) * 2 + 5 - H, 0), max((-(-W // 2) - 1) * 2 + 5 - W, 0)
    xt = F.pad(xt, (tw // 2, tw - tw // 2, th // 2, th - th // 2))
    w = torch.as_tensor(np.asarray(p[scope + '/weights'], np.float64)).permute(3, 2, 0, 1)
    z = F.conv2d(xt, w, torch.as_tensor(np.asarray(p[scope + '/biases'], np.float64)), stride=2)
    g, b, m, v = (torch.as_tensor(np.asarray(p['%s/BatchNorm/%s' % (scope, n)], np.float64)).view(1, -1, 1, 1)
                  for n in ('gamma', 'beta', 'moving_mean', 'moving_variance'))
    y = (torch.relu(z) - m) * (g / torch.sqrt(v + O.BN_EPS)) + b
    return F.max_pool2d(y, 2, 2, ceil_mode=True).permute(0, 2, 3, 1).contiguous().numpy()
