"""Rendered people restated in numpy from the text of include/jcm.h (jcm_synth_people); nothing here is shared with the library.
Every step is the header's, in its order, on int64 arrays (the capsule test on float64 products of integers, as the header states it), so the
device's bytes are expected to equal these bit for bit.  A primitive is evaluated on the pixels of a generous box around it only: outside it no
sub-sample can be inside, c = 0 and the pixel is unchanged."""
import numpy as np

REC_INTS, PRIM_INTS = 20, 16
NOISE_KEY = 0x5BD1E995
M32 = np.uint64(0xFFFFFFFF)
SUB = np.array([-6, -2, 2, 6], np.int64)      # the sub-samples of a pixel, sixteenths around its centre


def hash32(seed, i, j):
    """uint32 mix of the header on uint64 arrays masked to 32 bits; seed, i, j: integers or integer arrays (negative = two's complement)."""
    u = lambda v: np.asarray(v, np.int64).astype(np.uint64) & M32      # noqa: E731
    mul = lambda a, c: (a * np.uint64(c)) & M32                        # noqa: E731
    h = mul(u(seed), 0x9E3779B1) ^ mul(u(i), 0x85EBCA77) ^ mul(u(j), 0xC2B2AE3D)
    h ^= h >> np.uint64(16)
    h = mul(h, 0x7FEB352D)
    h ^= h >> np.uint64(15)
    h = mul(h, 0x846CA68B)
    h ^= h >> np.uint64(16)
    return h


def vnoise(seed, s, y, x):
    """int64 in 0..255, broadcast over the integer arrays y and x."""
    y, x = np.asarray(y, np.int64), np.asarray(x, np.int64)
    cell = 1 << s
    i, j, fy, fx = y >> s, x >> s, y & (cell - 1), x & (cell - 1)
    L = lambda a, b: (hash32(seed, a, b) >> np.uint64(24)).astype(np.int64)      # noqa: E731
    return ((cell - fy) * ((cell - fx) * L(i, j) + fx * L(i, j + 1)) + fy * ((cell - fx) * L(i + 1, j) + fx * L(i + 1, j + 1))) >> (2 * s)


def _samples(ys, xs):
    sy = (16 * ys[:, None] + SUB[None, :]).reshape(len(ys), 1, 4, 1)
    sx = (16 * xs[:, None] + SUB[None, :]).reshape(1, len(xs), 1, 4)
    return sy, sx


def capsule_coverage(ys, xs, ay, ax, by, bx, r):
    """int64 [len(ys), len(xs)]: how many of the 16 sub-samples of every pixel (y in ys, x in xs) lie in the capsule (jcm_render_poses)."""
    sy, sx = _samples(ys, xs)
    ey, ex = (sy - ay).astype(np.float64), (sx - ax).astype(np.float64)
    fy, fx = (sy - by).astype(np.float64), (sx - bx).astype(np.float64)
    dy, dx = np.float64(by - ay), np.float64(bx - ax)
    ee, t, L2, rr = ey * ey + ex * ex, ey * dy + ex * dx, dy * dy + dx * dx, np.float64(r) * np.float64(r)
    inside = np.where((L2 == 0) | (t <= 0), ee <= rr, np.where(t >= L2, fy * fy + fx * fx <= rr, ee * L2 - t * t <= rr * L2))
    return inside.sum(axis=(2, 3)).astype(np.int64)


def quad_coverage(ys, xs, q):
    """The same for the quadrilateral q = (y0, x0, .., y3, x3): all four cross products >= 0 or all <= 0, in int64."""
    sy, sx = _samples(ys, xs)
    ge = le = True
    for i in range(4):
        y0, x0, y1, x1 = int(q[2 * i]), int(q[2 * i + 1]), int(q[2 * ((i + 1) % 4)]), int(q[2 * ((i + 1) % 4) + 1])
        cr = (y1 - y0) * (sx - x0) - (x1 - x0) * (sy - y0)
        ge, le = ge & (cr >= 0), le & (cr <= 0)
    return (ge | le).sum(axis=(2, 3)).astype(np.int64)


def render(record, prims, H, W):
    """One image: record int [20], prims int [NP,16] (the whole list; the record names its own) -> uint8 [H,W,3]."""
    rec = [int(v) for v in np.asarray(record).reshape(REC_INTS)]
    prims = np.asarray(prims, np.int64).reshape(-1, PRIM_INTS)
    seed, c0, c1, amp, sh, a, n, first = rec[0], rec[1:4], rec[4:7], rec[7:11], rec[11:15], rec[15], rec[16], rec[17]
    y, x = np.arange(H, dtype=np.int64)[:, None], np.arange(W, dtype=np.int64)[None, :]
    noise = np.zeros((H, W), np.int64)
    for o in range(4):
        noise = noise + (amp[o] * (vnoise(seed + o, sh[o], y, x) - 128)) // 256
    v = np.empty((H, W, 3), np.int64)
    for k in range(3):
        g = c0[k] + ((c1[k] - c0[k]) * y) // max(H - 1, 1)
        v[:, :, k] = np.clip(g + noise, 0, 255)
    for p in prims[first:first + n]:
        kind, geo, col, tamp, ts, tseed = int(p[0]), [int(t) for t in p[1:9]], p[9:12], int(p[12]), int(p[13]), int(p[14])
        if kind == 0:
            lo_y, hi_y, lo_x, hi_x = min(geo[0], geo[2]) - geo[4], max(geo[0], geo[2]) + geo[4], min(geo[1], geo[3]) - geo[4], max(geo[1], geo[3]) + geo[4]
        else:
            lo_y, hi_y, lo_x, hi_x = min(geo[0::2]), max(geo[0::2]), min(geo[1::2]), max(geo[1::2])
        ys = np.arange(max(0, lo_y // 16 - 2), min(H, hi_y // 16 + 3), dtype=np.int64)
        xs = np.arange(max(0, lo_x // 16 - 2), min(W, hi_x // 16 + 3), dtype=np.int64)
        if len(ys) == 0 or len(xs) == 0:
            continue
        c = capsule_coverage(ys, xs, *geo[:5]) if kind == 0 else quad_coverage(ys, xs, geo)
        tex = (tamp * (vnoise(tseed, ts, ys[:, None], xs[None, :]) - 128)) // 256
        box = v[ys[0]:ys[-1] + 1, xs[0]:xs[-1] + 1]
        for k in range(3):
            t = np.clip(int(col[k]) + tex, 0, 255)
            box[:, :, k] = np.where(c > 0, (c * t + (16 - c) * box[:, :, k] + 8) >> 4, box[:, :, k])
    pos = y * W + x
    for k in range(3):
        d = (hash32(seed ^ NOISE_KEY, pos, k) % np.uint64(2 * a + 1)).astype(np.int64) - a
        v[:, :, k] = np.clip(v[:, :, k] + d, 0, 255)
    return v.astype(np.uint8)


def render_batch(records, prims, H, W):
    """records int [B,20], prims int [NP,16] -> uint8 [B,H,W,3]."""
    return np.stack([render(r, prims, H, W) for r in np.asarray(records).reshape(-1, REC_INTS)])


def record(seed=1, c0=(0, 0, 0), c1=None, amp=(0, 0, 0, 0), shifts=(6, 4, 2, 0), a=0, n=0, first=0):
    """A scene record from its parts (c1 None: c0)."""
    r = np.zeros(REC_INTS, np.int32)
    r[0], r[1:4], r[4:7], r[7:11], r[11:15], r[15], r[16], r[17] = seed, c0, c0 if c1 is None else c1, amp, shifts, a, n, first
    return r


def capsule(ay, ax, by, bx, r, col, tamp=0, ts=0, tseed=0):
    """A capsule primitive, geometry in sixteenths."""
    p = np.zeros(PRIM_INTS, np.int32)
    p[1:6], p[9:12], p[12:15] = (ay, ax, by, bx, r), col, (tamp, ts, tseed)
    return p


def quad(vertices, col, tamp=0, ts=0, tseed=0):
    """A quadrilateral primitive from four (y, x) vertices in sixteenths."""
    p = np.zeros(PRIM_INTS, np.int32)
    p[0], p[1:9], p[9:12], p[12:15] = 1, np.asarray(vertices).reshape(8), col, (tamp, ts, tseed)
    return p
