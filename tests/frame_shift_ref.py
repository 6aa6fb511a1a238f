"""jcm_frame_shift restated in numpy (include/jcm.h): the global whole-pixel translation between consecutive fitted frames, a
two-level exhaustive block match on integer luma.  All arithmetic is int64, so every output of the device kernels must be bit-equal to this.
tests/test_frame_shift_cpu.py holds it to a second formulation (plain Python loops); the GPU tests hold the library to it."""
import numpy as np

MAX_D, MAX_SIDE, MAX_T = 16, 4096, 65534


def check_args(T, H, W, rect, D):
    """The refusals of jcm_frame_shift that depend on sizes alone -> ValueError."""
    y0, x0, ch, cw = (int(v) for v in rect)
    if T < 1 or T > MAX_T:
        raise ValueError('T = %d' % T)
    if not 1 <= D <= MAX_D:
        raise ValueError('D = %d' % D)
    if H < 1 or W < 1 or H > MAX_SIDE or W > MAX_SIDE or H * W * 1020 >= 2 ** 32:
        raise ValueError('a frame of %d x %d' % (H, W))
    if y0 < 0 or x0 < 0 or ch < 1 or cw < 1 or y0 + ch > H or x0 + cw > W:
        raise ValueError('the rectangle %r is not inside %d x %d' % (rect, H, W))
    if ch < 8 * D + 7 or cw < 8 * D + 7:
        raise ValueError('a rectangle of %d x %d at D = %d' % (ch, cw, D))


def luma(frame, rect):
    """uint8 [H,W,3] -> int64 [ch,cw]: R + 2G + B of the content rectangle."""
    y0, x0, ch, cw = rect
    f = np.asarray(frame)[y0:y0 + ch, x0:x0 + cw].astype(np.int64)
    return f[..., 0] + 2 * f[..., 1] + f[..., 2]


def coarse(L):
    """int64 [ch,cw] -> [ch//4, cw//4]: sums over 4 x 4 blocks from the rectangle's corner, trailing pixels dropped."""
    Hc, Wc = L.shape[0] // 4, L.shape[1] // 4
    return L[:4 * Hc, :4 * Wc].reshape(Hc, 4, Wc, 4).sum(axis=(1, 3))


def sad(cur, prv, m, dy, dx):
    """sum |cur(y,x) - prv(y+dy, x+dx)| over the plane less a margin of m on every side."""
    h, w = cur.shape
    return int(np.abs(cur[m:h - m, m:w - m] - prv[m + dy:h - m + dy, m + dx:w - m + dx]).sum())


def _winner(cands):
    """[(S, dy, dx)] -> the one that minimises (S, dy^2 + dx^2, dy, dx)."""
    return min(cands, key=lambda c: (c[0], c[1] * c[1] + c[2] * c[2], c[1], c[2]))


def pair_shift(Lt, Lp, D):
    """One pair: the luma of frame t and of frame t-1 -> ((dy, dx), (S_f at the winner, S_f at (0,0)))."""
    Ct, Cp = coarse(Lt), coarse(Lp)
    _, cy, cx = _winner([(sad(Ct, Cp, D, dy, dx), dy, dx) for dy in range(-D, D + 1) for dx in range(-D, D + 1)])
    M = 4 * D + 3
    best = _winner([(sad(Lt, Lp, M, 4 * cy + ey, 4 * cx + ex), 4 * cy + ey, 4 * cx + ex) for ey in range(-3, 4) for ex in range(-3, 4)])
    return (best[1], best[2]), (best[0], sad(Lt, Lp, M, 0, 0))


def frame_shift(x, rect, D, prev=None):
    """x uint8 [T,H,W,3], rect (y0, x0, ch, cw), D, prev uint8 [H,W,3] or None -> (disp int32 [T,2], sad int64 [T,2])."""
    x = np.asarray(x)
    T, H, W = x.shape[:3]
    rect = tuple(int(v) for v in rect)
    check_args(T, H, W, rect, int(D))
    disp, sads = np.zeros((T, 2), np.int32), np.zeros((T, 2), np.int64)
    Lp = luma(prev, rect) if prev is not None else None
    for t in range(T):
        Lt = luma(x[t], rect)
        if Lp is not None:
            disp[t], sads[t] = pair_shift(Lt, Lp, int(D))
        Lp = Lt
    return disp, sads


def pan_canvas(rng, H, W, box=5):
    """A canvas to cut panned frames from: random bytes box-filtered with integers (a box x box sum, integer-divided by box^2), uint8 [H,W,3].
    Smooth enough for the coarse level to see a pan that is no multiple of 4, busy enough to have one best match."""
    raw = rng.integers(0, 256, size=(H + box - 1, W + box - 1, 3)).astype(np.int64)
    acc = np.zeros((H, W, 3), np.int64)
    for j in range(box):
        for i in range(box):
            acc += raw[j:j + H, i:i + W]
    return (acc // (box * box)).astype(np.uint8)


def pan_frames(canvas, H, W, origin, pans):
    """Crops [H,W,3] of the canvas: frame 0 at `origin`, frame t at o_t = o_{t-1} + pans[t] (pans[0] belongs to a frame before the clip and is
    not used).  Pixel (y,x) of frame t is the canvas at o_t + (y,x), which frame t-1 shows at (y,x) + o_t - o_{t-1}: with the sign of
    jcm_frame_shift, pans[t] IS the displacement of frame t against frame t-1."""
    o = np.array(origin, np.int64)
    out = []
    for t, p in enumerate(pans):
        if t:
            o = o + np.array(p, np.int64)
        if o.min() < 0 or o[0] + H > canvas.shape[0] or o[1] + W > canvas.shape[1]:
            raise ValueError('crop %d leaves the canvas' % t)
        out.append(canvas[o[0]:o[0] + H, o[1]:o[1] + W])
    return np.ascontiguousarray(np.stack(out))


def known_pans(D):
    """The displacements every test of the pans must recover, none left out: rest, one pixel along each axis, both axes at once, one that is no
    multiple of 4 on either axis, and the reach of the search, 4D + 3, along each axis."""
    m = 4 * D + 3
    return [(0, 0), (1, 0), (-1, 0), (0, 1), (0, -1), (2, -2), (-5, 6), (m, 0), (-m, 0), (0, m), (0, -m)]


def pan_clip(D, H, W, seed=11):
    """The clip the CPU and GPU tests share: frame 0, then one frame per known pan, cut from one box-filtered canvas -> (x [12,H,W,3], pans)."""
    pans = known_pans(D)
    at = np.cumsum(pans, axis=0)
    lo, hi = np.minimum(at.min(axis=0), 0), np.maximum(at.max(axis=0), 0)
    canvas = pan_canvas(np.random.default_rng(seed), H + int(hi[0] - lo[0]), W + int(hi[1] - lo[1]), box=9)
    return pan_frames(canvas, H, W, (-int(lo[0]), -int(lo[1])), [(0, 0)] + pans), pans
