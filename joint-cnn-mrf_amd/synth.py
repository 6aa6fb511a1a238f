"""Deterministic synthetic inputs and parameters for the joint-heat-map path.

There is no network for FLIC images or trained checkpoints, so tests and `bench.py` use
seeded data of the reference's shapes and initial distributions:

* conv weights: He truncated normal, sigma = sqrt(2/(k*k*Cin)), HWIO   (main.py:138-147)
* conv biases: 0                                                        (main.py:150-153)
* BatchNorm: contrib defaults gamma=1, beta=0, mean=0, var=1 ('identity'), or a
  'trained'-like set (gamma~U[.5,1.5], beta,mean~N(0,.1), var~U[.5,1.5])
* pairwise energies: float32 cast of the prior histograms               (main.py:482-484)
* pairwise biases: 1e-5                                                  (main.py:486-487)
* images: U[0,1) float32 [B,480,720,3]                                   (data.py:129-130)
* torso map: the 3x3 binomial blob [1,2,1]^T[1,2,1]/16                   (data.py:112-114,180-186)

Everything is keyed by the reference's TF variable names so a real checkpoint would map 1:1.
"""
import numpy as np
from scipy.special import ndtri

JOINT_NAMES = ['lsho', 'lelb', 'lwri', 'rsho', 'relb', 'rwri', 'lhip', 'rhip', 'nose', 'torso']  # main.py:18
N_JOINTS = 9                                                                                     # main.py:458
N_FILTERS = (64, 128, 256, 512, 512)                                                             # main.py:38
RESOLUTIONS = ('fullres', 'halfres', 'quarterres')

_PHI_M2 = 0.022750131948179195   # Phi(-2)
_PHI_P2 = 0.9772498680518208     # Phi(+2)


def n_filters(debug=False):
    """main.py:38-41."""
    return tuple(f // 4 for f in N_FILTERS) if debug else N_FILTERS


def conv_scopes(debug=False, n_joints=N_JOINTS):
    """[(scope, k, stride, Cin, Cout, last_layer)] in graph order (main.py:44-72)."""
    f = n_filters(debug)
    out = []
    for res in RESOLUTIONS:
        out += [('conv1_' + res, 5, 2, 3, f[0], False), ('conv2_' + res, 5, 1, f[0], f[1], False),
                ('conv3_' + res, 5, 1, f[1], f[2], False), ('conv4_' + res, 9, 1, f[2], f[3], False)]
    out += [('conv5', 9, 1, f[3], f[4], False), ('conv6', 9, 1, f[4], n_joints, True)]
    return out


def truncated_normal(rs, shape, stddev):
    """tf.truncated_normal (main.py:146): N(0, stddev) restricted to +-2 sigma.  Drawn by
    inverse CDF from one uniform stream so the sequence is a pure function of the seed."""
    u = rs.random_sample(int(np.prod(shape)))
    z = ndtri(_PHI_M2 + u * (_PHI_P2 - _PHI_M2))
    return (z * stddev).astype(np.float32).reshape(shape)


def make_pd_params(debug=False, seed=7, bn='identity', conv6_gain=1.0, n_joints=N_JOINTS):
    """Part-detector parameters under the reference's variable names."""
    rs = np.random.RandomState(seed)
    p = {}
    for scope, k, _s, cin, cout, last in conv_scopes(debug, n_joints):
        w = truncated_normal(rs, (k, k, cin, cout), np.sqrt(2.0 / (k * k * cin)))   # main.py:141,146
        if last and conv6_gain != 1.0:
            w = (w * np.float32(conv6_gain)).astype(np.float32)
        p[scope + '/weights'] = w
        p[scope + '/biases'] = np.zeros(cout, np.float32)                             # main.py:152
        if not last:
            _add_bn(p, scope, cout, rs, bn)
    return p


def _add_bn(p, scope, c, rs, kind):
    if kind == 'identity':
        g, b, m, v = np.ones(c), np.zeros(c), np.zeros(c), np.ones(c)
    elif kind == 'trained':
        g = rs.uniform(0.5, 1.5, c)
        b = rs.normal(0, 0.1, c)
        m = rs.normal(0, 0.1, c)
        v = rs.uniform(0.5, 1.5, c)
    else:
        raise ValueError(kind)
    for n, a in (('gamma', g), ('beta', b), ('moving_mean', m), ('moving_variance', v)):
        p['%s/BatchNorm/%s' % (scope, n)] = np.asarray(a, np.float32)


def pair_keys(n_joints=N_JOINTS):
    """The 81 '<j>_<c>' keys in graph order (main.py:479-481)."""
    return ['%s_%s' % (j, c) for j in JOINT_NAMES[:n_joints] for c in JOINT_NAMES if c != j]


def make_sm_params(priors, kind='init', seed=11, n_joints=N_JOINTS):
    """Spatial-model parameters.  `priors`: dict '<j>_<c>' -> [120,180] (pairwise_distribution
    pickle, main.py:297-299).  kind='init' reproduces main.py:477-487 exactly; 'trained' scales
    the energies/biases and gives bn_sm a non-trivial affine so the pairwise terms have real
    dynamic range (at init they are nearly constant)."""
    rs = np.random.RandomState(seed)
    p = {}
    for key in pair_keys(n_joints):
        e = np.asarray(priors[key], np.float32)                                       # main.py:482
        if kind == 'init':
            b = np.full((60, 90), 1e-5, np.float32)                                   # main.py:486
        else:
            e = (e * np.float32(400.0) - np.float32(0.05)).astype(np.float32)
            b = (0.02 * rs.random_sample((60, 90))).astype(np.float32)
        p['energy_' + key] = e.reshape(1, e.shape[0], e.shape[1], 1)                   # main.py:483
        p['bias_' + key] = b.reshape(1, 60, 90, 1)
    if kind == 'init':
        _add_bn(p, 'bn_sm', 10, rs, 'identity')
    else:
        p['bn_sm/BatchNorm/gamma'] = rs.uniform(20.0, 40.0, 10).astype(np.float32)
        p['bn_sm/BatchNorm/beta'] = rs.normal(-0.05, 0.02, 10).astype(np.float32)
        p['bn_sm/BatchNorm/moving_mean'] = rs.uniform(0.0, 1e-3, 10).astype(np.float32)
        p['bn_sm/BatchNorm/moving_variance'] = rs.uniform(0.5, 1.5, 10).astype(np.float32)
    return p


def synthetic_priors(seed=5, n_joints=N_JOINTS):
    """Seeded stand-ins for the 120x180 displacement histograms: a few Gaussian bumps per
    pair, normalised to sum 1 like the real ones (prepare_pairwise_distribution.py:46)."""
    rs = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:120, 0:180].astype(np.float64)
    out = {}
    for key in pair_keys(n_joints):
        pd = np.zeros((120, 180))
        for _ in range(3):
            cy, cx = 60 + rs.normal(0, 12), 90 + rs.normal(0, 18)
            sy, sx = rs.uniform(2, 8), rs.uniform(2, 10)
            pd += rs.uniform(0.2, 1.0) * np.exp(-0.5 * (((yy - cy) / sy) ** 2 + ((xx - cx) / sx) ** 2))
        out[key] = pd / pd.sum()
    return out


def make_images(batch, seed=1234, height=480, width=720):
    """U[0,1) float32 NHWC images (data.py:129-130 scales JPEG bytes to [0,1])."""
    return np.random.RandomState(seed).random_sample((batch, height, width, 3)).astype(np.float32)


def make_torso(batch, seed=4321, hm_height=60, hm_width=90):
    """[B,60,90,1] torso heat maps: 3x3 binomial blob at a uniform interior cell
    (data.py:112-114,180-186)."""
    rs = np.random.RandomState(seed)
    kern = np.outer([1, 2, 1], [1, 2, 1]).astype(np.float32) / 16
    t = np.zeros((batch, hm_height, hm_width, 1), np.float32)
    for b in range(batch):
        r, c = rs.randint(1, hm_height - 1), rs.randint(1, hm_width - 1)
        t[b, r - 1:r + 2, c - 1:c + 2, 0] = kern
    return t


def make_targets(batch, seed=4321, hm_height=60, hm_width=90, n_channels=10):
    """[B,60,90,10] target heat maps y_in (main.py:488): one 3x3 binomial blob per joint and image
    (data.py:112-114,180-186).  Channel 9 (torso) uses the same stream as `make_torso(batch, seed)`
    so `make_targets(...)[..., 9:]` equals it."""
    kern = np.outer([1, 2, 1], [1, 2, 1]).astype(np.float32) / 16
    t = np.zeros((batch, hm_height, hm_width, n_channels), np.float32)
    t[..., n_channels - 1:] = make_torso(batch, seed, hm_height, hm_width)
    rs = np.random.RandomState(seed + 1)
    for b in range(batch):
        for k in range(n_channels - 1):
            r, c = rs.randint(1, hm_height - 1), rs.randint(1, hm_width - 1)
            t[b, r - 1:r + 2, c - 1:c + 2, k] = kern
    return t


# ------------------------------------------------------------------ rendered people (include/jcm.h: jcm_synth_people)
SYNTH_REC_INTS, SYNTH_PRIM_INTS, SYNTH_PRIM_MAX = 20, 16, 64
SYNTH_SHIFTS = (6, 4, 2, 0)                      # the octaves' lattice cells: 64, 16, 4, 1 pixels
LR_PERM = (3, 4, 5, 0, 1, 2, 7, 6, 8)           # where joint k of a mirrored pose reads from (data.py / hm_flip.h, the first nine entries)
# The ranges people_scene draws from.  CHOICES, not measurements (DESIGN.md 4.22 has the table): picked so that the figures look like people at
# FLIC's scale in a 480x720 frame; none of them has been tuned against anything.
PEOPLE_DEFAULTS = dict(
    scale=(0.6, 1.0),             # the similarity's scale about the pose's centre
    shift=0.12,                   # its shift, +- this share of the frame's width and height
    tries=32,                     # draws of the similarity before the pose is left as it is
    other_scale=(0.5, 1.0),       # the second person's scale
    other_dist=12,                # the least distance of the two torso centres, in heat-map cells of 8 pixels
    r_thigh=0.24, r_upper=0.13, r_fore=0.10, r_hand=0.12, r_neck=0.11, r_head=0.34,      # radii as shares of the shoulder-to-hip distance
    torso_margin=0.16,            # the torso quadrilateral's growth, the same share
    head_lift=0.12,               # the head disc's centre above the nose, the same share
    min_hand=2.0,                 # pixels: the least hand radius, so that the wrist's own pixel is covered whole
    cloth=((20, 235), (20, 235), (20, 235)),          # the clothing colour box (R, G, B), one draw for the top and one for the trousers
    skin=((140, 245), (95, 200), (70, 170)),          # the skin colour box
    cloth_tex=(8, 48), skin_tex=(4, 20),              # texture amplitudes
    cloth_ts=2, skin_ts=1,                            # texture shifts: lattice cells of 4 and 2 pixels
    clutter=(0, 12),              # the count of clutter capsules
    clutter_skin=0.3,             # the share of them in a skin colour
    clutter_len=(10.0, 160.0), clutter_r=(3.0, 22.0),      # pixels
    bg=((30, 225), (30, 225), (30, 225)),             # the box both background colours are drawn from
    bg_amp=((10, 70), (8, 50), (4, 30), (0, 14)),     # the four octaves' amplitude ranges
    noise=(0, 6),                 # the sensor-noise amplitude
)
KIND_CAPSULE, KIND_QUAD = 0, 1


def _colour(rng, box):
    return [int(rng.randint(lo, hi + 1)) for lo, hi in box]


def _capsule(a, b, r, col, tamp, ts, tseed):
    """A primitive before rounding: (kind, geometry float64 [8] in pixels (y, x order), colour, tamp, ts, tseed); a, b = (x, y)."""
    return (KIND_CAPSULE, [a[1], a[0], b[1], b[0], r, 0.0, 0.0, 0.0], col, tamp, ts, tseed)


def _figure(rng, J, H, rg, skin=None):
    """The primitives of one person, back to front, from the joints J float64 [2,9] (x, y).  Draws, in this order: the top's colour, the trousers'
    colour, the skin colour, the three texture amplitudes, the three texture seeds, which arm is listed first, and for each arm (left, right)
    whether it lies over the torso."""
    top, trousers = _colour(rng, rg['cloth']), _colour(rng, rg['cloth'])
    skin = _colour(rng, rg['skin'])
    ta_top, ta_trousers = (int(rng.randint(rg['cloth_tex'][0], rg['cloth_tex'][1] + 1)) for _ in range(2))
    ta_skin = int(rng.randint(rg['skin_tex'][0], rg['skin_tex'][1] + 1))
    s_top, s_trousers, s_skin = (int(rng.randint(0, 2 ** 31 - 1)) for _ in range(3))
    left_first = rng.random_sample() < 0.5
    over = [rng.random_sample() < 0.5, rng.random_sample() < 0.5]
    P = [J[:, k] for k in range(9)]
    lsho, lelb, lwri, rsho, relb, rwri, lhip, rhip, nose = P
    msho, mhip = (lsho + rsho) / 2, (lhip + rhip) / 2
    u = max(float(np.hypot(*(msho - mhip))), 8.0)
    cloth_kw, trousers_kw, skin_kw = (top, ta_top, rg['cloth_ts'], s_top), (trousers, ta_trousers, rg['cloth_ts'], s_trousers), (skin, ta_skin, rg['skin_ts'], s_skin)
    r_thigh = rg['r_thigh'] * u
    thighs = [_capsule(hip, np.array([hip[0], H + 2 * r_thigh + u]), r_thigh, *trousers_kw) for hip in (lhip, rhip)]
    centre = (lsho + rsho + rhip + lhip) / 4
    quad = []
    for v in (lsho, rsho, rhip, lhip):
        d = v - centre
        n = float(np.hypot(*d))
        v = v + rg['torso_margin'] * u * d / n if n > 0 else v
        quad += [v[1], v[0]]
    torso = [(KIND_QUAD, quad, top, ta_top, rg['cloth_ts'], s_top)]
    up = nose - msho
    n = float(np.hypot(*up))
    up = up / n if n > 0 else np.array([0.0, -1.0])
    head = [_capsule(msho, nose, rg['r_neck'] * u, *skin_kw), _capsule(nose + rg['head_lift'] * u * up, nose + rg['head_lift'] * u * up, rg['r_head'] * u, *skin_kw)]
    arms = [[_capsule(sho, elb, rg['r_upper'] * u, *cloth_kw), _capsule(elb, wri, rg['r_fore'] * u, *skin_kw)] for sho, elb, wri in ((lsho, lelb, lwri), (rsho, relb, rwri))]
    hands = [_capsule(wri, wri, max(rg['r_hand'] * u, rg['min_hand']), *skin_kw) for wri in (lwri, rwri)]
    order = (0, 1) if left_first else (1, 0)
    under = [p for i in order if not over[i] for p in arms[i]]
    above = [p for i in order if over[i] for p in arms[i]]
    return thighs + under + torso + head + above + hands      # the hands last: the pixel under an annotated wrist is skin


def _fit_inside(J, H, W):
    """J [2,9] moved -- and, only if its box is larger than the frame, shrunk about its centre -- by the least amount that puts it inside."""
    J = J.copy()
    span = J.max(axis=1) - J.min(axis=1)
    k = min(1.0, (W - 1.0) / max(span[0], 1e-9), (H - 1.0) / max(span[1], 1e-9))
    if k < 1.0:
        c = (J.max(axis=1, keepdims=True) + J.min(axis=1, keepdims=True)) / 2
        J = c + (J - c) * (k * (1 - 1e-9))
    for ax, hi in ((0, W - 1.0), (1, H - 1.0)):
        J[ax] += max(0.0, -J[ax].min())
        J[ax] -= max(0.0, J[ax].max() - hi)
        J[ax] = np.clip(J[ax], 0.0, hi)      # (the last bit of the two shifts)
    return J


def _inside(J, H, W):
    return bool((J[0] >= 0).all() and (J[0] <= W - 1).all() and (J[1] >= 0).all() and (J[1] <= H - 1).all())


def _similarity(J, s, dx, dy):
    c = J.mean(axis=1, keepdims=True)
    return c + s * (J - c) + np.array([[dx], [dy]])


def _mirror(J, W):
    M = J[:, list(LR_PERM)].copy()
    M[0] = (W - 1) - M[0]
    return M


def people_scene(rng, pose_xy, other_xy=None, H=480, W=720, **ranges):
    """One scene of rendered people -> (record int32 [20], prims int32 [n,16], xy float64 [2,9]): what jcm_synth_people draws and
    the annotated person's nine joints (x, y) in the H x W frame.  pose_xy, other_xy: float64 [2,9] annotations in a 480x720 frame (data.py's xy;
    another frame size maps them by min(H / 480, W / 720) about the centre); other_xy None: no second person.  ranges: entries of PEOPLE_DEFAULTS.
    Every draw comes from `rng` (a numpy RandomState) in a fixed order, so the scene is a pure function of the generator's state:
      the annotated person: up to `tries` times (scale, mirror, shift x, shift y) until all nine joints lie inside the frame -- after that the
        pose as it is (moved inside by the least shift if the annotation itself is not); then the draws of _figure;
      the second person (other_xy): scale, mirror, up to `tries` torso centres (x, y) until the centre is `other_dist` cells from the annotated
        one -- after that the frame's left or right edge, whichever is farther; then the draws of _figure;
      the clutter: the count, then per capsule (centre x, y, angle, length, radius, skin?, colour, texture amplitude, texture seed);
      the background: seed, c0, c1, the four amplitudes, the sensor-noise amplitude.
    Listing order, back to front: the second person, the clutter, the annotated person.  Geometry is rounded to sixteenths of a pixel last."""
    sc = _scene_draw(rng, pose_xy, other_xy, H, W, _ranges(ranges))
    record, prims = _scene_place(sc, sc['person'])
    return record, prims, sc['J']


def _ranges(ranges):
    unknown = set(ranges) - set(PEOPLE_DEFAULTS)
    if unknown:
        raise TypeError('people_scene: unknown ranges %s' % sorted(unknown))
    return dict(PEOPLE_DEFAULTS, **ranges)


def _scene_draw(rng, pose_xy, other_xy, H, W, rg):
    """Every draw of people_scene, in its order -> the scene before it is listed: the annotated person's joints 'J' and primitives 'person', 'move'
    (the map of the plane that took the pose to J: a pose [2,9] of the 480x720 frame -> the H x W frame), 'look' (the generator's state just
    before the person's _figure: replaying _figure from it with other joints gives the same clothes, skin, seeds and listing order, since none of
    its draws depends on the joints), 'other', 'clutter', 'record' (its count and first index still 0) and the geometry."""
    f = min(H / 480.0, W / 720.0)
    frame_c, src_c = np.array([[(W - 1) / 2.0], [(H - 1) / 2.0]]), np.array([[719 / 2.0], [479 / 2.0]])

    def to_frame(p):
        return frame_c + f * (np.asarray(p, np.float64).reshape(2, 9) - src_c)

    J0 = to_frame(pose_xy)
    J = move = None
    for _ in range(int(rg['tries'])):
        s = rng.uniform(*rg['scale'])
        mirror = rng.random_sample() < 0.5
        dx, dy = rng.uniform(-rg['shift'], rg['shift']) * W, rng.uniform(-rg['shift'], rg['shift']) * H
        base = _mirror(J0, W) if mirror else J0
        cand = _similarity(base, s, dx, dy)
        if _inside(cand, H, W):
            J = cand
            c = base.mean(axis=1, keepdims=True)      # the same similarity about the SAME centre, for another pose

            def move(p, s=s, dx=dx, dy=dy, mirror=mirror, c=c):
                q = to_frame(p)
                return c + s * ((_mirror(q, W) if mirror else q) - c) + np.array([[dx], [dy]])
            break
    if J is None:
        J = J0 if _inside(J0, H, W) else _fit_inside(J0, H, W)

        def move(p, J=J):      # the pose as it is: another pose keeps its offsets from this one
            return J + (to_frame(p) - J0)
    look = rng.get_state()
    person = _figure(rng, J, H, rg)

    other = []
    if other_xy is not None:
        O = to_frame(other_xy)
        s = rng.uniform(*rg['other_scale'])
        if rng.random_sample() < 0.5:
            O = _mirror(O, W)
        O = _similarity(O, s, 0.0, 0.0)
        tc = (J[:, 0] + J[:, 3] + J[:, 6] + J[:, 7]) / 4
        oc = (O[:, 0] + O[:, 3] + O[:, 6] + O[:, 7]) / 4
        need, place = rg['other_dist'] * 8.0, None
        for _ in range(int(rg['tries'])):
            c = np.array([rng.uniform(0.05, 0.95) * (W - 1), rng.uniform(0.2, 0.9) * (H - 1)])
            if np.hypot(*(c - tc)) >= need:
                place = c
                break
        if place is None:
            place = np.array([0.0 if tc[0] > (W - 1) / 2.0 else W - 1.0, tc[1]])
        O = O + (place - oc).reshape(2, 1)
        other = _figure(rng, O, H, rg)

    clutter = []
    for _ in range(int(rng.randint(rg['clutter'][0], rg['clutter'][1] + 1))):
        c = np.array([rng.uniform(0, W - 1), rng.uniform(0, H - 1)])
        ang, ln, r = rng.uniform(0, np.pi), rng.uniform(*rg['clutter_len']), rng.uniform(*rg['clutter_r'])
        is_skin = rng.random_sample() < rg['clutter_skin']
        col = _colour(rng, rg['skin'] if is_skin else rg['cloth'])
        tamp = int(rng.randint(rg['cloth_tex'][0], rg['cloth_tex'][1] + 1))
        d = np.array([np.cos(ang), np.sin(ang)]) * ln / 2
        clutter.append(_capsule(c - d, c + d, r, col, tamp, rg['skin_ts'] if is_skin else rg['cloth_ts'], int(rng.randint(0, 2 ** 31 - 1))))

    record = np.zeros(SYNTH_REC_INTS, np.int32)
    record[0] = rng.randint(0, 2 ** 31 - 1)
    record[1:4], record[4:7] = _colour(rng, rg['bg']), _colour(rng, rg['bg'])
    record[7:11] = [rng.randint(lo, hi + 1) for lo, hi in rg['bg_amp']]
    record[11:15] = SYNTH_SHIFTS
    record[15] = rng.randint(rg['noise'][0], rg['noise'][1] + 1)
    return dict(J=J, move=move, look=look, person=person, other=other, clutter=clutter, record=record, H=H, rg=rg)


def _scene_place(sc, person, first=0):
    """The scene listed with `person` as the annotated person's primitives -> (record int32 [20], prims int32 [n,16])."""
    record = sc['record'].copy()
    listed = sc['other'] + sc['clutter'] + person
    if len(listed) > SYNTH_PRIM_MAX:
        raise ValueError('people_scene: %d primitives, the kernel takes %d an image' % (len(listed), SYNTH_PRIM_MAX))
    record[16] = len(listed)
    prims = np.zeros((len(listed), SYNTH_PRIM_INTS), np.int32)
    lim = float(2 ** 20)
    for i, (kind, geo, col, tamp, ts, tseed) in enumerate(listed):
        g = np.clip(np.rint(np.asarray(geo, np.float64) * 16.0), -lim, lim)      # sixteenths of a pixel, last
        prims[i, 0], prims[i, 1:9], prims[i, 9:12], prims[i, 12:15] = kind, g.astype(np.int64), col, (tamp, ts, tseed)
    record[17] = first
    return record, prims


def people_clip(rng, pose_a, pose_b, T, other_xy=None, H=480, W=720, cuts=(), **ranges):
    """T frames of ONE scene of rendered people in which the annotated person moves -> (records int32 [T,20], prims int32 [NP,16],
    xy float64 [T,2,9]); records[t, 17] is frame t's first row of prims, so Engine.synth_people draws the clip as it is.  The scene -- similarity,
    look, clutter, background, second person, draw order -- is people_scene(rng, pose_a, other_xy, ...)'s, and frame 0 IS that scene, bit for bit
    (and the generator is left where people_scene leaves it).  In frame t the annotated person's joints are A + (t / (T - 1)) * (B - A): A the
    joints of frame 0, B pose_b under the same similarity -- brought towards A along the straight line by the least amount that keeps all nine
    joints inside the frame, so that every frame's joints are known and inside.  The clothes, skin, texture seeds and listing order do not change:
    _figure is replayed from the generator state saved before it with the frame's joints.  A frame index in `cuts` (1 .. T-1) starts a new
    scene, drawn from the generator as it stands, with the same pose pair and the same t / (T - 1).  Everything else stands still, the sensor
    noise included: its seed is the record's, so the noise pattern repeats from frame to frame within a scene."""
    T = int(T)
    cuts = sorted({int(c) for c in cuts})
    if T < 1 or any(c < 1 or c >= T for c in cuts):
        raise ValueError('people_clip: T >= 1 and cuts in 1 .. T-1 are expected, got T = %d, cuts = %s' % (T, cuts))
    rg = _ranges(ranges)
    records, prims, xy, first, sc = [], [], [], 0, None
    replay = np.random.RandomState(0)
    for t in range(T):
        if t == 0 or t in cuts:
            sc = _scene_draw(rng, pose_a, other_xy, H, W, rg)
            A, B = sc['J'], sc['move'](pose_b)
            lam = 1.0
            for lo_side, hi_side, ax in ((0.0, W - 1.0, 0), (0.0, H - 1.0, 1)):      # A is inside: the largest share of the way to B that still is
                for k in range(9):
                    if B[ax, k] < lo_side:
                        lam = min(lam, (A[ax, k] - lo_side) / (A[ax, k] - B[ax, k]))
                    elif B[ax, k] > hi_side:
                        lam = min(lam, (hi_side - A[ax, k]) / (B[ax, k] - A[ax, k]))
            step = (lam * (1 - 1e-9) if lam < 1.0 else 1.0) * (B - A)
        J = sc['J'] + (t / float(max(T - 1, 1))) * step
        if t == 0:
            person = sc['person']
        else:
            replay.set_state(sc['look'])
            person = _figure(replay, J, H, rg)
        r, p = _scene_place(sc, person, first)
        first += p.shape[0]
        records.append(r)
        prims.append(p)
        xy.append(J)
    return np.stack(records), np.concatenate(prims).reshape(-1, SYNTH_PRIM_INTS), np.stack(xy)


def people_batch(rng, poses, indices, H=480, W=720, second=True, **ranges):
    """Scenes of the poses poses[indices] ([N,2,9] float64, data.py's xy) stacked -> (records int32 [B,20], prims int32 [NP,16], xy float64 [B,2,9],
    cells int64 [B,10,2], y float32 [B,60,90,10]).  Per image, from `rng`: the index of the second person's pose among ALL of `poses` (second=True),
    then the draws of people_scene.  cells = data.joint_cells(xy) and y = data.target_heat_maps(cells): the data set's own path from an annotation
    to its target maps, which reads the frame as 480x720."""
    from . import data
    poses = np.asarray(poses, np.float64)
    recs, prims, xy, first = [], [], [], 0
    for i in np.asarray(indices).reshape(-1):
        other = poses[int(rng.randint(0, poses.shape[0]))] if second else None
        r, p, j = people_scene(rng, poses[int(i)], other, H, W, **ranges)
        r[17] = first
        first += p.shape[0]
        recs.append(r)
        prims.append(p)
        xy.append(j)
    xy = np.stack(xy)
    cells = data.joint_cells(xy)
    return np.stack(recs), np.concatenate(prims).reshape(-1, SYNTH_PRIM_INTS), xy, cells, data.target_heat_maps(cells)
