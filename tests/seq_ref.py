"""A numpy float64 restatement of jcm_seq_filter and jcm_seq_viterbi (include/jcm.h): both recurrences with explicit tap loops in the
stated order, one rounded operation per step.  The sum Z is taken in the kernel's documented order (csrc/sequence.hip: 1024 threads, a thread adds
the cells tid, tid + 1024, .. ascending, a butterfly over the 64 lanes of a wave, then the 16 wave sums in wave order), so the restated filter can be
compared bit for bit; kernel_order=False takes numpy's pairwise sum instead, which the derived tolerance of the GPU tests covers.

Also the inputs the CPU and the GPU tests share: CASES and case_inputs()."""
import numpy as np

THREADS = 1024


def kernel_sum(v):
    """The float64 sum of the flat array v in the order of sq_block_sum."""
    v = np.asarray(v, np.float64).reshape(-1)
    n = -(-v.size // THREADS)
    rows = np.zeros((n, THREADS), np.float64)
    rows.reshape(-1)[:v.size] = v
    acc = np.zeros(THREADS, np.float64)
    for r in rows:      # a thread's cells, ascending; the padding adds +0.0 to a non-negative sum
        acc = acc + r
    lanes = np.arange(THREADS)
    for o in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[lanes ^ o]
    z = acc[0]
    for w in range(1, THREADS // 64):
        z = z + acc[64 * w]
    return z


def _total(v, kernel_order):
    return kernel_sum(v) if kernel_order else np.float64(np.sum(v))


def _argmax(a):
    """First-occurrence flat arg-max."""
    return int(np.argmax(a.reshape(-1)))


def _rows(n, d):
    """The cells y of 0..n-1 with 0 <= y - d < n: (y0, y1)."""
    return max(0, d), min(n, n + d)


def blur_sum(a, w, R):
    """m of the filter: the vertical pass, then the horizontal one, terms outside the map skipped, ascending from 0.0."""
    HH, WW = a.shape
    c = np.zeros_like(a)
    for dy in range(-R, R + 1):
        y0, y1 = _rows(HH, dy)
        if y0 < y1:
            c[y0:y1] = c[y0:y1] + w[dy + R] * a[y0 - dy:y1 - dy]
    m = np.zeros_like(a)
    for dx in range(-R, R + 1):
        x0, x1 = _rows(WW, dx)
        if x0 < x1:
            m[:, x0:x1] = m[:, x0:x1] + w[dx + R] * c[:, x0 - dx:x1 - dx]
    return m


def blur_max(d, w, R):
    """m of Viterbi and the flat source cell of every cell: ascending scans, a strictly greater value replaces."""
    HH, WW = d.shape
    c = np.full_like(d, -1.0)
    sdy = np.zeros(d.shape, np.int64)
    for dy in range(-R, R + 1):
        y0, y1 = _rows(HH, dy)
        if y0 < y1:
            v = w[dy + R] * d[y0 - dy:y1 - dy]
            better = v > c[y0:y1]
            c[y0:y1] = np.where(better, v, c[y0:y1])
            sdy[y0:y1] = np.where(better, dy, sdy[y0:y1])
    m = np.full_like(d, -1.0)
    sdx = np.zeros(d.shape, np.int64)
    for dx in range(-R, R + 1):
        x0, x1 = _rows(WW, dx)
        if x0 < x1:
            v = w[dx + R] * c[:, x0 - dx:x1 - dx]
            better = v > m[:, x0:x1]
            m[:, x0:x1] = np.where(better, v, m[:, x0:x1])
            sdx[:, x0:x1] = np.where(better, dx, sdx[:, x0:x1])
    ys, xs = np.mgrid[0:HH, 0:WW]
    via_x = xs - sdx
    src_y = ys - sdy[ys, via_x]
    return m, src_y * WW + via_x


def seq_filter(hm, taps, rho, state=None, kernel_order=True):
    """hm float32 [S,T,HH,WW,K], taps float64 [K,2R+1], state float64 [S,K,HH,WW] or None -> {'belief' float64 [S,T,HH,WW,K] (a_t; 'filtered' is
    its float32 rounding), 'filtered', 'coords' int32 [S,T,2,K], 'norm' float64 [S,T,K], 'reset' int32 [S,T,K], 'state' float64 [S,K,HH,WW]}."""
    hm = np.asarray(hm, np.float32)
    taps = np.asarray(taps, np.float64)
    S, T, HH, WW, K = hm.shape
    R = (taps.shape[1] - 1) // 2
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
                    pred = om * blur_sum(a, taps[k], R) + u
                    b = p * pred
                    Z = _total(b, kernel_order)
                    if not (Z > 0.0 and np.isfinite(Z)):
                        rs = 1
                if a is None or rs == 1:
                    b = p
                    Z = _total(b, kernel_order)
                    if Z == 0.0:
                        rs = 2
                a = np.full((HH, WW), np.float64(1.0) / np.float64(HW)) if rs == 2 else b / Z
                belief[s, t, :, :, k] = a
                i = _argmax(a)
                coords[s, t, :, k] = (i // WW, i % WW)
                norm[s, t, k], reset[s, t, k] = Z, rs
            out_state[s, k] = a
    return {'belief': belief, 'filtered': belief.astype(np.float32), 'coords': coords, 'norm': norm, 'reset': reset, 'state': out_state}


def seq_viterbi(hm, taps, rho):
    """-> {'path' int32 [S,T,2,K], 'maxes' float64 [S,T,K], 'breaks' int32 [S,T,K]}."""
    hm = np.asarray(hm, np.float32)
    taps = np.asarray(taps, np.float64)
    S, T, HH, WW, K = hm.shape
    R = (taps.shape[1] - 1) // 2
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
                    m, from_cell = blur_max(d, taps[k], R)
                    e = om * m
                    jump = u * d.max()
                    jumps = jump > e
                    e = np.where(jumps, jump, e)
                    from_cell = np.where(jumps, _argmax(d), from_cell)
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
                amax[t] = _argmax(d)
                maxes[s, t, k], breaks[s, t, k] = M, brk
            cell = amax[T - 1]
            for t in range(T - 1, -1, -1):
                path[s, t, :, k] = (cell // WW, cell % WW)
                if t > 0:
                    cell = src[t, cell] if src[t, cell] >= 0 else amax[t - 1]
    return {'path': path, 'maxes': maxes, 'breaks': breaks}


def tolerance(t, HW, R):
    """The relative distance the GPU tests allow between the kernel's float64 state / norm at frame t and a restatement that sums in another
    order: the first-order rounding bound of t + 1 steps of positive sums, (t + 1) * (HW + 4R + 8) * 2^-53.  Derived, not measured."""
    return (t + 1) * (HW + 4 * R + 8) * 2.0 ** -53


def top2_gap(belief):
    """belief [S,T,HH,WW,K] -> [S,T,K]: (largest - second largest) / largest of every map."""
    S, T, HH, WW, K = belief.shape
    flat = np.sort(belief.transpose(0, 1, 4, 2, 3).reshape(S, T, K, HH * WW), axis=-1)
    return (flat[..., -1] - flat[..., -2]) / flat[..., -1] if HH * WW > 1 else np.ones((S, T, K))


# ------------------------------------------------------------------ the inputs the CPU and GPU tests share
# name: (S, T, HH, WW, K, R, sigma, rho)
CASES = {
    'real': (1, 4, 60, 90, 9, 5, 1.5, 0.05),            # the geometry of the tower's maps, once
    'one_frame': (1, 1, 5, 7, 1, 2, 1.0, 0.05),
    'clipped': (1, 3, 5, 7, 2, 8, 3.0, 0.05),            # every tap range is clipped on both sides
    'odd': (2, 5, 13, 17, 3, 3, (0.8, 1.5, 2.5), 0.05),  # odd sizes, interleaved channels, two sequences
    'vector': (2, 3, 6, 10, 3, 2, 1.0, 0.05),            # HW * K a multiple of 4: the float4 staging, a float4 straddling pixels
    'radius0': (1, 3, 5, 7, 2, 0, 1.0, 0.05),
    'rho0': (1, 3, 13, 17, 3, 3, 1.5, 0.0),
    'rho1': (1, 3, 13, 17, 3, 3, 1.5, 1.0),
    'split': (1, 6, 13, 17, 3, 3, 1.5, 0.05),
}


def random_maps(shape, seed):
    """Non-negative float32 maps with a few strong modes per map: what a coin flip between modes looks like."""
    rs = np.random.RandomState(seed)
    S, T, HH, WW, K = shape
    hm = (rs.rand(*shape) ** 4 * 0.05).astype(np.float32)
    for s in range(S):
        for t in range(T):
            for k in range(K):
                for _ in range(3):
                    hm[s, t, rs.randint(HH), rs.randint(WW), k] += np.float32(0.5 + rs.rand())
    return hm


def case_inputs(name, taps_of):
    """(hm, taps, R, sigma, rho, seed) of CASES[name]; taps_of = predict.seq_taps.  The seed is the first from 0 at which the REFERENCE's filtered
    belief has, in every map, a relative top-2 gap above ten times the tolerance the GPU tests allow -- a condition on the inputs that the
    reference alone decides, so that a coordinate mismatch cannot be blamed on a tie."""
    S, T, HH, WW, K, R, sigma, rho = CASES[name]
    taps = taps_of(sigma, R, K)
    for seed in range(100):
        hm = random_maps((S, T, HH, WW, K), 1000 + seed)
        if gap_holds(hm, taps, rho, R):
            return hm, taps, R, sigma, rho, seed
    raise AssertionError('no seed below 100 gives case %r a top-2 gap' % name)


def gap_holds(hm, taps, rho, R):
    S, T, HH, WW, K = hm.shape
    gap = top2_gap(seq_filter(hm, taps, rho)['belief'])
    need = np.array([10.0 * tolerance(t, HH * WW, R) for t in range(T)])
    return bool((gap > need[None, :, None]).all())
