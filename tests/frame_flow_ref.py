"""jcm_frame_flow and jcm_hm_flow_pool restated in numpy (include/jcm.h): one whole-pixel displacement per heat-map cell by block
matching on integer luma, and the neighbours' heat maps warped by it and pooled.  The matching is int64 arithmetic and the pooling float64 in the
header's order, so every output of the device kernels must be bit-equal to this.  tests/test_frame_flow_cpu.py holds both to second formulations
(plain Python loops); the GPU tests hold the library to them.  The case tables the CPU and the GPU tests share are at the end."""
import functools

import numpy as np

MAX_D, MAX_R, MAX_SIDE, MAX_T, MAX_N, CELL = 16, 8, 4096, 65534, 4, 8


def check_args(T, H, W, rect, D, R):
    """The refusals of jcm_frame_flow that depend on sizes alone -> ValueError."""
    y0, x0, ch, cw = (int(v) for v in rect)
    if T < 1 or T > MAX_T:
        raise ValueError('T = %d' % T)
    if not 1 <= D <= MAX_D:
        raise ValueError('D = %d' % D)
    if not 1 <= R <= MAX_R:
        raise ValueError('R = %d' % R)
    if H < 1 or W < 1 or H % CELL or W % CELL or H > MAX_SIDE or W > MAX_SIDE:
        raise ValueError('a frame of %d x %d' % (H, W))
    if y0 < 0 or x0 < 0 or ch < 1 or cw < 1 or y0 + ch > H or x0 + cw > W:
        raise ValueError('the rectangle %r is not inside %d x %d' % (rect, H, W))


def luma(frame, rect):
    """uint8 [H,W,3] -> int64 [ch,cw]: R + 2G + B of the content rectangle."""
    y0, x0, ch, cw = rect
    f = np.asarray(frame)[y0:y0 + ch, x0:x0 + cw].astype(np.int64)
    return f[..., 0] + 2 * f[..., 1] + f[..., 2]


def cell_spans(n_cells, origin, size):
    """Per cell along one axis, the block [8c - 4, 8c + 12) cut to the content [origin, origin + size), in the content's own coordinates ->
    (lo, hi) int64 [n_cells]; lo >= hi is an empty span."""
    c = np.arange(n_cells, dtype=np.int64)
    return np.maximum(CELL * c - 4 - origin, 0), np.minimum(CELL * c + 12 - origin, size)


def pair_flow(Lt, Ls, rect, HH, WW, D):
    """One slot: the luma of frame t and of its reference frame -> (flow int64 [HH,WW,2], sad int64 [HH,WW,2]).  Per candidate the absolute
    differences of the overlap of the two planes, a summed-area table of them, and every cell's block sum out of its four corners; the running
    minimum of the key S * 2^22 + (dy^2 + dx^2) * 2^12 + (dy + D) * 2^6 + (dx + D) is the minimum of the tuple (S, dy^2 + dx^2, dy, dx)."""
    y0, x0, ch, cw = rect
    ylo, yhi = cell_spans(HH, y0, ch)
    xlo, xhi = cell_spans(WW, x0, cw)
    full = (ylo < yhi)[:, None] & (xlo < xhi)[None, :]
    NONE = np.int64(2) ** 62
    best = np.full((HH, WW), NONE)
    zero = np.zeros((HH, WW), np.int64)
    for dy in range(-D, D + 1):
        for dx in range(-D, D + 1):
            # rows [a0, a1) x columns [b0, b1) of frame t whose displaced pixel is inside the rectangle
            a0, a1, b0, b1 = max(0, -dy), min(ch, ch - dy), max(0, -dx), min(cw, cw - dx)
            valid = full & ((ylo >= a0) & (yhi <= a1))[:, None] & ((xlo >= b0) & (xhi <= b1))[None, :]
            if not valid.any():
                continue
            diff = np.abs(Lt[a0:a1, b0:b1] - Ls[a0 + dy:a1 + dy, b0 + dx:b1 + dx])
            sat = np.zeros((a1 - a0 + 1, b1 - b0 + 1), np.int64)
            sat[1:, 1:] = diff.cumsum(axis=0).cumsum(axis=1)
            ya, yb = np.clip(ylo - a0, 0, a1 - a0), np.clip(yhi - a0, 0, a1 - a0)
            xa, xb = np.clip(xlo - b0, 0, b1 - b0), np.clip(xhi - b0, 0, b1 - b0)
            S = sat[yb[:, None], xb[None, :]] - sat[ya[:, None], xb[None, :]] - sat[yb[:, None], xa[None, :]] + sat[ya[:, None], xa[None, :]]
            key = (S << 22) + ((dy * dy + dx * dx) << 12) + ((dy + D) << 6) + (dx + D)
            best = np.where(valid & (key < best), key, best)
            if dy == 0 and dx == 0:
                zero = np.where(valid, S, 0)
    got = best != NONE
    flow = np.stack([np.where(got, ((best >> 6) & 63) - D, 0), np.where(got, (best & 63) - D, 0)], axis=2)
    sad = np.stack([np.where(got, best >> 22, 0), zero], axis=2)
    return flow, sad


def frame_flow(x, rect, D, ref):
    """x uint8 [T,H,W,3], rect (y0, x0, ch, cw), D, ref int [T,R] -> (flow int32 [T,R,HH,WW,2], sad int32 [T,R,HH,WW,2]).  A ref entry that is
    negative or >= T is "no such frame": its slot is zero."""
    x, ref = np.asarray(x), np.asarray(ref)
    T, H, W = x.shape[:3]
    rect = tuple(int(v) for v in rect)
    if ref.ndim != 2 or ref.shape[0] != T:
        raise ValueError('ref %s' % (ref.shape,))
    R = ref.shape[1]
    check_args(T, H, W, rect, int(D), R)
    HH, WW = H // CELL, W // CELL
    flow, sad = np.zeros((T, R, HH, WW, 2), np.int32), np.zeros((T, R, HH, WW, 2), np.int32)
    L = {}
    for t in range(T):
        for r in range(R):
            s = int(ref[t, r])
            if 0 <= s < T:
                for f in (t, s):
                    if f not in L:
                        L[f] = luma(x[f], rect)
                flow[t, r], sad[t, r] = pair_flow(L[t], L[s], rect, HH, WW, int(D))
    return flow, sad


def flow_refs(T, N):
    """motion.flow_refs, written again: int32 [T,2N], slot 2(n-1) = t - n, slot 2(n-1) + 1 = t + n, -1 outside the clip."""
    ref = np.full((T, 2 * N), -1, np.int32)
    for t in range(T):
        for n in range(1, N + 1):
            if t - n >= 0:
                ref[t, 2 * (n - 1)] = t - n
            if t + n < T:
                ref[t, 2 * (n - 1) + 1] = t + n
    return ref


def sample(plane, py, px):
    """plane float64 [HH,WW,K]; py, px float64 [HH,WW], already clamped -> [HH,WW,K]: the bilinear sample in the header's association order."""
    HH, WW = plane.shape[:2]
    fy0, fx0 = np.floor(py), np.floor(px)
    ya, xa = fy0.astype(np.int64), fx0.astype(np.int64)
    yb, xb = np.minimum(ya + 1, HH - 1), np.minimum(xa + 1, WW - 1)
    fy, fx = (py - fy0)[..., None], (px - fx0)[..., None]
    top = (1.0 - fx) * plane[ya, xa] + fx * plane[ya, xb]
    bot = (1.0 - fx) * plane[yb, xa] + fx * plane[yb, xb]
    return (1.0 - fy) * top + fy * bot


def check_weights(w):
    w = np.asarray(w, np.float64).reshape(-1)
    if not 1 <= w.size - 1 <= MAX_N:
        raise ValueError('N = %d' % (w.size - 1))
    if not np.isfinite(w).all() or not w[0] > 0 or (w < 0).any():
        raise ValueError('weights %r' % (w,))
    return w


def hm_flow_pool(hm, flow, w):
    """hm fp32 [T,HH,WW,K], flow int [T,2N,HH,WW,2], w float64 [N+1] -> fp32 [T,HH,WW,K]; float64, the header's order."""
    hm, flow, w = np.asarray(hm), np.asarray(flow), check_weights(w)
    T, HH, WW, K = hm.shape
    N = w.size - 1
    if hm.dtype != np.float32 or flow.shape != (T, 2 * N, HH, WW, 2):
        raise ValueError('hm %s %s, flow %s' % (hm.dtype, hm.shape, flow.shape))
    h64 = hm.astype(np.float64)
    yy, xx = np.meshgrid(np.arange(HH, dtype=np.float64), np.arange(WW, dtype=np.float64), indexing='ij')
    out = np.empty_like(hm)
    for t in range(T):
        acc, ws = w[0] * h64[t], w[0]
        for n in range(1, N + 1):
            for side, s in enumerate((t - n, t + n)):
                if not 0 <= s < T:
                    continue
                f = flow[t, 2 * (n - 1) + side].astype(np.float64)
                py = np.minimum(np.maximum(yy + f[..., 0] / 8.0, 0.0), float(HH - 1))
                px = np.minimum(np.maximum(xx + f[..., 1] / 8.0, 0.0), float(WW - 1))
                acc = acc + w[n] * sample(h64[s], py, px)
                ws = ws + w[n]
        out[t] = (acc / ws).astype(np.float32)
    return out


# ------------------------------------------------------------------ the cases the CPU and the GPU tests share (read-only arrays, made once)
def _frozen(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def noise_clip(T, H, W, seed):
    """iid bytes, uint8 [T,H,W,3]: frames that match nowhere, so that the tie-break tuple and the validity rules decide."""
    return _frozen(np.random.default_rng(seed).integers(0, 256, size=(T, H, W, 3)).astype(np.uint8))


@functools.lru_cache(maxsize=None)
def smooth_clip(T, H, W, seed, step=(1, -2)):
    """Crops of one box-filtered canvas that drift by `step` a frame, with fresh noise in a corner of every frame: most cells have one clear best
    match, some have none.  uint8 [T,H,W,3]."""
    rng = np.random.default_rng(seed)
    m = 4 * T
    raw = rng.integers(0, 256, size=(H + 2 * m + 2, W + 2 * m + 2, 3)).astype(np.int64)
    canvas = sum(raw[j:j + H + 2 * m, i:i + W + 2 * m] for j in range(3) for i in range(3)) // 9
    x = np.stack([canvas[m + t * step[0]:m + t * step[0] + H, m + t * step[1]:m + t * step[1] + W] for t in range(T)]).astype(np.uint8)
    x[:, :H // 3, :W // 3] = rng.integers(0, 256, size=(T, H // 3, W // 3, 3))
    return _frozen(np.ascontiguousarray(x))


PLANT_SHAPE, PLANT_RECT, PLANT_D, PLANT_MOVE = (64, 128), (0, 0, 64, 128), 5, (3, -2)
PLANT_PATCH = (16, 24, 32, 40)      # (y, x, h, w) of the patch in frame 0; frame 1 shows it PLANT_MOVE further


@functools.lru_cache(maxsize=None)
def planted_pair():
    """Two frames of ONE field of iid noise (seed 5); the patch PLANT_PATCH of frame 0 is in frame 1 at PLANT_PATCH + PLANT_MOVE, and what it
    left behind is fresh noise.  With ref = [[1], [0]]: cells of frame 0 inside the patch move by PLANT_MOVE, those of frame 1 inside the moved
    patch by -PLANT_MOVE, and a cell far from both patches sees the same bytes in both frames."""
    rng = np.random.default_rng(5)
    H, W = PLANT_SHAPE
    x = np.repeat(rng.integers(0, 256, size=(1, H, W, 3)).astype(np.uint8), 2, axis=0)
    y, q, h, w = PLANT_PATCH
    x[1, y:y + h, q:q + w] = rng.integers(0, 256, size=(h, w, 3))
    x[1, y + PLANT_MOVE[0]:y + PLANT_MOVE[0] + h, q + PLANT_MOVE[1]:q + PLANT_MOVE[1] + w] = x[0, y:y + h, q:q + w]
    return _frozen(x)


def planted_cells():
    """(inside, far) bool [2,HH,WW] for the planted pair with ref [[1], [0]]: inside -- the cell's 16 x 16 block lies wholly in the patch as the
    cell's own frame shows it (the matched block is then wholly in the patch of the other frame as well); far -- the block is farther than D + 16
    pixels from the patch in both frames, so that no candidate's block touches it in either."""
    H, W = PLANT_SHAPE
    HH, WW = H // CELL, W // CELL
    y, q, h, w = PLANT_PATCH
    boxes = [(y, q, y + h, q + w), (y + PLANT_MOVE[0], q + PLANT_MOVE[1], y + PLANT_MOVE[0] + h, q + PLANT_MOVE[1] + w)]
    inside, far = np.zeros((2, HH, WW), bool), np.zeros((2, HH, WW), bool)
    g = PLANT_D + 16
    for Y in range(HH):
        for X in range(WW):
            b = (CELL * Y - 4, CELL * X - 4, CELL * Y + 12, CELL * X + 12)
            for f in range(2):
                p = boxes[f]
                inside[f, Y, X] = b[0] >= p[0] and b[1] >= p[1] and b[2] <= p[2] and b[3] <= p[3]
            far[:, Y, X] = all(b[2] + g <= p[0] or b[0] - g >= p[2] or b[3] + g <= p[1] or b[1] - g >= p[3] for p in boxes)
    return inside, far


# (name, T, H, W, rect, D, ref, the clip's maker): the smallest shapes at which each path of the matching can go wrong
SMALL = (5, 7)      # cells of the 40 x 56 frames
FLOW_CASES = (
    # origin and size no multiples of 4 or 8; cells cut by the rectangle on every side, cells wholly in a bar, candidates invalid on one side only
    ('cut on every side', 4, 40, 56, (3, 5, 30, 41), 3, ((1, -1), (0, 2), (3, 1), (2, 0)), 'smooth'),
    ('noise, ties and validity', 4, 40, 56, (3, 5, 30, 41), 3, ((1, 3), (2, 0), (1, 1), (0, 2)), 'noise'),
    # a rectangle so small that some cells' blocks fill it in one direction: only dy = 0, or only (0,0), is valid there
    ('only (0,0) is valid', 2, 40, 56, (14, 22, 9, 11), 3, ((1,), (0,)), 'noise'),
    ('a column of valid dx', 2, 40, 56, (10, 3, 12, 50), 3, ((1,), (0,)), 'smooth'),
    ('D = 1', 2, 48, 64, (0, 0, 48, 64), 1, ((1,), (0,)), 'smooth'),
    ('D = 16', 2, 48, 64, (2, 1, 45, 61), 16, ((1,), (0,)), 'smooth'),
    ('T = 1, every ref negative', 1, 40, 56, (3, 5, 30, 41), 3, ((-1, -1),), 'noise'),
    ('T = 1, matched against itself', 1, 40, 56, (3, 5, 30, 41), 3, ((0,),), 'noise'),
    ('a ref entry >= T is absent', 3, 40, 56, (3, 5, 30, 41), 2, ((3, 1), (2, 7), (2 ** 31 - 1, 0)), 'smooth'),
    ('R = 8', 3, 40, 56, (0, 0, 40, 56), 2, ((1, 2, -1, 0, 1, 2, -5, 1), (0, 0, 0, 0, 2, 2, 2, 2), (3, -1, 1, 0, 3, -1, 1, 0)), 'smooth'),
    ('two strips of cells', 2, 16, 160, (1, 3, 14, 150), 4, ((1,), (0,)), 'smooth'),
)


def flow_case(name):
    _, T, H, W, rect, D, ref, kind = next(c for c in FLOW_CASES if c[0] == name)
    x = smooth_clip(T, H, W, 21) if kind == 'smooth' else noise_clip(T, H, W, 22)
    return x, rect, D, np.array(ref, np.int32)


@functools.lru_cache(maxsize=None)
def flow_case_expected(name):
    x, rect, D, ref = flow_case(name)
    return tuple(_frozen(a) for a in frame_flow(x, rect, D, ref))


def pool_maps(T, HH, WW, K, seed):
    """fp32 [T,HH,WW,K] whose values span the fp32 exponent range: m * 2^e with m in [1, 2) and e in -120 .. 120, half of them within a few binades
    of each other: sums that absorb a term and sums that round.  (All positive, so a re-ordered sum differs in the last float64 bit only, which the
    rounding to fp32 nearly always hides: order_case below is the case that shows the order.)"""
    rng = np.random.default_rng(seed)
    m = rng.random((T, HH, WW, K)) + 1.0
    e = rng.integers(-120, 121, size=(T, HH, WW, K))
    near = rng.random((T, HH, WW, K)) < 0.5      # half of the values within a few binades of each other: sums that round
    e = np.where(near, rng.integers(-3, 4, size=e.shape), e)
    return _frozen(np.ldexp(m, e).astype(np.float32))


def pool_flow(T, N, HH, WW, seed, reach=40):
    """int32 [T,2N,HH,WW,2]: displacements up to `reach` pixels, 5 cells, either way -- past all four edges of a 5 x 7 map, with every eighth."""
    return _frozen(np.random.default_rng(seed).integers(-reach, reach + 1, size=(T, 2 * N, HH, WW, 2)).astype(np.int32))


def order_case():
    """(hm fp32 [3,5,7,2], flow int32 [3,2,5,7,2], w): maps on which the ORDER of the sum decides the rounded result, by construction.  A float64 sum
    re-ordered differs in its last bit, which the rounding to fp32 hides; it shows where a term cancels another that absorbs the third.  Frame 1 holds
    -2^60, the frame before it +2^60 and the frame after it 1, uniform weights, flows of whole cells (exact samples): (-2^60 + 2^60) + 1 = 1 in the
    header's order, t - n first, and (-2^60 + 1) + 2^60 = 0 with t + n first.  out[1] = 1/3 away from the edges the flow pushes samples over."""
    hm = np.empty((3, 5, 7, 2), np.float32)
    hm[0], hm[1], hm[2] = 2.0 ** 60, -2.0 ** 60, 1.0
    flow = np.zeros((3, 2, 5, 7, 2), np.int32)
    flow[:, 0, :, :, 1], flow[:, 1, :, :, 0] = 8, -16
    return _frozen(hm), _frozen(flow), (1.0, 1.0)


POOL_WEIGHTS = {1: (1.0, 0.7), 4: (0.9, 0.8, 0.0, 0.35, 1.25)}
# (K, N, T): T = 1, 2 and 2N + 1 so that every neighbour-absent pattern occurs
POOL_CASES = tuple((K, N, T) for K in (1, 9, 16) for N in (1, 4) for T in (1, 2, 2 * N + 1))
