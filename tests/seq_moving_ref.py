"""A numpy float64 restatement of jcm_seq_filter_moving and jcm_seq_viterbi_moving (include/jcm.h): the recurrences of tests/seq_ref.py
with a whole-cell shift of the belief plane per frame -- cell (y, x) of frame t is cell (y + sy, x + sx) of frame t-1 -- written with explicit tap
loops in the stated order, one rounded operation per step, and the sum Z in the kernel's order (seq_ref.kernel_sum).  Python integers carry the
shifts, so nothing here clamps: a term is taken exactly when its source cell lies inside the map.

Also the inputs the CPU and the GPU tests share: CASES and case_inputs()."""
import numpy as np

import seq_ref as R

INT_MIN, INT_MAX = -2 ** 31, 2 ** 31 - 1


def _span(n, d, s):
    """The cells y of 0..n-1 whose source y - d + s lies in 0..n-1: (y0, y1), possibly empty."""
    return max(0, d - s), min(n, n + d - s)


def blur_sum(a, w, R_, sy, sx):
    """m of the moving filter: c(y,x') = sum over dy of w * a(y - dy + sy, x'), then m(y,x) = sum over dx of w * c(y, x - dx + sx); terms outside
    the map skipped, ascending from 0.0."""
    HH, WW = a.shape
    c = np.zeros_like(a)
    for dy in range(-R_, R_ + 1):
        y0, y1 = _span(HH, dy, sy)
        if y0 < y1:
            c[y0:y1] = c[y0:y1] + w[dy + R_] * a[y0 - dy + sy:y1 - dy + sy]
    m = np.zeros_like(a)
    for dx in range(-R_, R_ + 1):
        x0, x1 = _span(WW, dx, sx)
        if x0 < x1:
            m[:, x0:x1] = m[:, x0:x1] + w[dx + R_] * c[:, x0 - dx + sx:x1 - dx + sx]
    return m


def blur_max(d, w, R_, sy, sx):
    """m of the moving Viterbi and the flat source cell (in frame t-1's lattice) of every cell; ascending scans, a strictly greater value replaces, a
    maximum over no term is 0.  A cell with m == 0 has no source inside the map: -1 here, the jump's source for the caller."""
    HH, WW = d.shape
    c = np.full_like(d, -1.0)
    sdy = np.zeros(d.shape, np.int64)
    for dy in range(-R_, R_ + 1):
        y0, y1 = _span(HH, dy, sy)
        if y0 < y1:
            v = w[dy + R_] * d[y0 - dy + sy:y1 - dy + sy]
            better = v > c[y0:y1]
            c[y0:y1] = np.where(better, v, c[y0:y1])
            sdy[y0:y1] = np.where(better, dy, sdy[y0:y1])
    c = np.where(c < 0.0, 0.0, c)      # no term: every term is >= 0, so -1 survives only there
    m = np.full_like(d, -1.0)
    sdx = np.zeros(d.shape, np.int64)
    for dx in range(-R_, R_ + 1):
        x0, x1 = _span(WW, dx, sx)
        if x0 < x1:
            v = w[dx + R_] * c[:, x0 - dx + sx:x1 - dx + sx]
            better = v > m[:, x0:x1]
            m[:, x0:x1] = np.where(better, v, m[:, x0:x1])
            sdx[:, x0:x1] = np.where(better, dx, sdx[:, x0:x1])
    has = m > 0.0
    m = np.where(has, m, 0.0)
    ys, xs = np.mgrid[0:HH, 0:WW]
    via_x = np.where(has, xs - sdx + sx, 0)
    src_y = np.where(has, ys - sdy[ys, via_x] + sy, 0)
    assert ((src_y >= 0) & (src_y < HH) & (via_x >= 0) & (via_x < WW)).all()
    return m, np.where(has, src_y * WW + via_x, -1)


def seq_filter(hm, taps, rho, shift, state=None, kernel_order=True):
    """seq_ref.seq_filter with shift int [S,T,2]; shift[s,0] applies to the transition from `state` and is ignored without one."""
    hm = np.asarray(hm, np.float32)
    taps = np.asarray(taps, np.float64)
    S, T, HH, WW, K = hm.shape
    R_ = (taps.shape[1] - 1) // 2
    HW = HH * WW
    om, u = np.float64(1.0) - np.float64(rho), np.float64(rho) / np.float64(HW)
    belief = np.zeros((S, T, HH, WW, K), np.float64)
    coords = np.zeros((S, T, 2, K), np.int32)
    norm = np.zeros((S, T, K), np.float64)
    reset = np.zeros((S, T, K), np.int32)
    out_state = np.zeros((S, K, HH, WW), np.float64)
    for s in range(S):
        for k in range(K):
            a = None if state is None else np.array(state[s, k], np.float64)
            for t in range(T):
                p = hm[s, t, :, :, k].astype(np.float64)
                rs, Z = 0, np.float64(0.0)
                if a is not None:
                    pred = om * blur_sum(a, taps[k], R_, int(shift[s][t][0]), int(shift[s][t][1])) + u
                    b = p * pred
                    Z = R._total(b, kernel_order)
                    if not (Z > 0.0 and np.isfinite(Z)):
                        rs = 1
                if a is None or rs == 1:
                    b = p
                    Z = R._total(b, kernel_order)
                    if Z == 0.0:
                        rs = 2
                a = np.full((HH, WW), np.float64(1.0) / np.float64(HW)) if rs == 2 else b / Z
                belief[s, t, :, :, k] = a
                i = R._argmax(a)
                coords[s, t, :, k] = (i // WW, i % WW)
                norm[s, t, k], reset[s, t, k] = Z, rs
            out_state[s, k] = a
    return {'belief': belief, 'filtered': belief.astype(np.float32), 'coords': coords, 'norm': norm, 'reset': reset, 'state': out_state}


def seq_viterbi(hm, taps, rho, shift):
    """seq_ref.seq_viterbi with shift int [S,T,2] (shift[s,0] is ignored); path[s,t] is in frame t's own lattice."""
    hm = np.asarray(hm, np.float32)
    taps = np.asarray(taps, np.float64)
    S, T, HH, WW, K = hm.shape
    R_ = (taps.shape[1] - 1) // 2
    HW = HH * WW
    om, u = np.float64(1.0) - np.float64(rho), np.float64(rho) / np.float64(HW)
    path = np.zeros((S, T, 2, K), np.int32)
    maxes = np.zeros((S, T, K), np.float64)
    breaks = np.zeros((S, T, K), np.int32)
    for s in range(S):
        for k in range(K):
            src = np.full((T, HW), -1, np.int64)
            amax = np.zeros(T, np.int64)
            d = None
            for t in range(T):
                p = hm[s, t, :, :, k].astype(np.float64)
                brk, M = 0, np.float64(0.0)
                if t > 0:
                    m, from_cell = blur_max(d, taps[k], R_, int(shift[s][t][0]), int(shift[s][t][1]))
                    e = om * m
                    jump = u * d.max()
                    jumps = jump > e
                    e = np.where(jumps, jump, e)
                    from_cell = np.where(jumps | (from_cell < 0), R._argmax(d), from_cell)
                    b = p * e
                    src[t] = from_cell.reshape(-1)
                    M = b.max()
                    if M == 0.0:
                        brk = 1
                if t == 0 or brk == 1:
                    b = p
                    src[t] = -1
                    M = b.max()
                    if M == 0.0:
                        brk = 2
                d = np.ones((HH, WW), np.float64) if brk == 2 else b / M
                amax[t] = R._argmax(d)
                maxes[s, t, k], breaks[s, t, k] = M, brk
            cell = amax[T - 1]
            for t in range(T - 1, -1, -1):
                path[s, t, :, k] = (cell // WW, cell % WW)
                if t > 0:
                    cell = src[t, cell] if src[t, cell] >= 0 else amax[t - 1]
    return {'path': path, 'maxes': maxes, 'breaks': breaks}


# ------------------------------------------------------------------ the inputs the CPU and GPU tests share
# name: (S, T, HH, WW, K, R, sigma, rho, shifts [S][T] of (sy, sx)); shifts[s][0] matters only to a call that is given a state
CASES = {
    # the geometry of the tower's maps, once, with shifts of a few cells
    'real': (1, 4, 60, 90, 9, 5, 1.5, 0.05, [[(0, 0), (2, -3), (-1, 4), (3, 1)]]),
    'one_frame': (1, 1, 5, 7, 1, 2, 1.0, 0.05, [[(3, -2)]]),
    # every tap range is clipped on both sides, shifts (+-1, +-2)
    'clipped': (1, 5, 5, 7, 2, 8, 3.0, 0.05, [[(0, 0), (1, -2), (-1, 2), (1, 2), (-1, -2)]]),
    # odd sizes, interleaved channels, a different shift per sequence, shifts larger than R = 3
    'odd': (2, 5, 13, 17, 3, 3, (0.8, 1.5, 2.5), 0.05, [[(0, 0), (1, 0), (0, -2), (5, 4), (-2, 1)], [(0, 0), (-1, 3), (2, 2), (0, 0), (-4, -5)]]),
    # HW * K a multiple of 4: the float4 staging
    'vector': (2, 3, 6, 10, 3, 2, 1.0, 0.05, [[(0, 0), (1, 1), (-2, 3)], [(0, 0), (0, -1), (2, 0)]]),
    # rows: sy = -HH, the maps share no cell but the taps reach across; sy = HH + R, INT_MIN and INT_MAX, nothing reaches
    'far_rows': (1, 5, 5, 7, 2, 2, 1.0, 0.05, [[(0, 0), (-5, 1), (7, 0), (INT_MIN, 0), (INT_MAX, 1)]]),
    # columns likewise: sx = WW, then -(WW + R), INT_MAX, INT_MIN
    'far_cols': (1, 5, 5, 7, 2, 2, 1.0, 0.05, [[(0, 0), (1, 7), (0, -9), (0, INT_MAX), (-1, INT_MIN)]]),
    'radius0': (1, 4, 5, 7, 2, 0, 1.0, 0.05, [[(0, 0), (1, -1), (0, 2), (-1, 0)]]),
    'rho0': (1, 4, 13, 17, 3, 3, 1.5, 0.0, [[(0, 0), (1, -2), (-2, 1), (16, 0)]]),      # sy = HH + R: the last transition reaches nothing, a reset / a break
    'rho1': (1, 3, 13, 17, 3, 3, 1.5, 1.0, [[(0, 0), (1, -2), (-2, 1)]]),
    'split': (1, 6, 13, 17, 3, 3, 1.5, 0.05, [[(0, 0), (1, 1), (-1, 2), (2, -3), (0, 1), (-2, 0)]]),      # cut before frame 3: its shift is non-zero
}


def case_inputs(name, taps_of):
    """(hm, taps, R, sigma, rho, shift int64 [S,T,2], seed) of CASES[name]; taps_of = predict.seq_taps.  The seed is the first from 0 at which the
    RESTATEMENT's filtered belief has, in every map, a relative top-2 gap above ten times seq_ref.tolerance -- a condition on the inputs that the
    restatement alone decides, so that a coordinate mismatch cannot be blamed on a tie."""
    S, T, HH, WW, K, R_, sigma, rho, shifts = CASES[name]
    shift = np.array(shifts, np.int64).reshape(S, T, 2)
    taps = taps_of(sigma, R_, K)
    for seed in range(100):
        hm = R.random_maps((S, T, HH, WW, K), 2000 + seed)
        if gap_holds(hm, taps, rho, R_, shift):
            return hm, taps, R_, sigma, rho, shift, seed
    raise AssertionError('no seed below 100 gives case %r a top-2 gap' % name)


def gap_holds(hm, taps, rho, R_, shift):
    S, T, HH, WW, K = hm.shape
    gap = R.top2_gap(seq_filter(hm, taps, rho, shift)['belief'])
    need = np.array([10.0 * R.tolerance(t, HH * WW, R_) for t in range(T)])
    return bool((gap > need[None, :, None]).all())


def on_union(hm, shift):
    """The maps of ONE sequence hm [T,HH,WW,K] with shift [T,2], zero-padded at their window offsets into the bounding box of all windows ->
    (union maps [1,T,UH,UW,K], offsets int [T,2] of every frame's window in the union).  Frame t's origin is frame t-1's plus its shift."""
    T, HH, WW, K = hm.shape
    org = np.cumsum(np.concatenate([np.zeros((1, 2), np.int64), np.asarray(shift, np.int64)[1:]]), axis=0)
    org = org - org.min(axis=0)
    UH, UW = int(org[:, 0].max()) + HH, int(org[:, 1].max()) + WW
    out = np.zeros((1, T, UH, UW, K), np.float32)
    for t in range(T):
        out[0, t, org[t, 0]:org[t, 0] + HH, org[t, 1]:org[t, 1] + WW] = hm[t]
    return out, org
