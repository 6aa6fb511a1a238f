"""A numpy float64 restatement of jcm_seq_filter_centred and jcm_seq_viterbi_centred (include/jcm.h): the moving recurrences of
tests/seq_moving_ref.py with the shift read per DESTINATION cell from centre int [S,T,HH,WW,2].  A frame is computed the slow, obvious way: for
every distinct (sy, sx) that occurs in the frame's table, seq_moving_ref.blur_sum / blur_max is evaluated on the WHOLE plane with that shift, and the
cells that carry that shift are taken from it.  That is the definition by construction -- the text of the moving entries with (sy, sx) read per
cell -- and it shares not a line of index arithmetic with the kernel, which gathers a (2R+1)^2 window per cell.  Python integers carry the shifts,
so nothing here clamps.  Z is summed in the kernel's order (seq_ref.kernel_sum).

Also the inputs the CPU and the GPU tests share: CASES, case_table() and case_inputs()."""
import numpy as np

import seq_moving_ref as MR
import seq_ref as R

INT_MIN, INT_MAX = -2 ** 31, 2 ** 31 - 1


def per_cell(table, planes_of):
    """table int [HH,WW,2]; planes_of(sy, sx) -> a tuple of [HH,WW] planes computed with that one shift -> the tuple with every cell taken from the
    planes of its own shift."""
    table = np.asarray(table, np.int64)
    out = None
    for sy, sx in np.unique(table.reshape(-1, 2), axis=0):
        planes = planes_of(int(sy), int(sx))
        mine = (table[..., 0] == sy) & (table[..., 1] == sx)
        if out is None:
            out = [np.zeros_like(p) for p in planes]
        for o, p in zip(out, planes):
            o[mine] = p[mine]
    return out


def seq_filter(hm, taps, rho, centre, state=None, kernel_order=True):
    """seq_moving_ref.seq_filter with centre int [S,T,HH,WW,2]; centre[s,0] applies to the transition from `state` and is ignored without one."""
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
                    m, = per_cell(centre[s][t], lambda sy, sx: (MR.blur_sum(a, taps[k], R_, sy, sx),))
                    pred = om * m + u
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


def seq_viterbi(hm, taps, rho, centre):
    """seq_moving_ref.seq_viterbi with centre int [S,T,HH,WW,2] (centre[s,0] is never read); path[s,t] is in frame t's own lattice."""
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
                    m, from_cell = per_cell(centre[s][t], lambda sy, sx: MR.blur_max(d, taps[k], R_, sy, sx))
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


def uniform_table(shift, HH, WW):
    """shift int [S,T,2] -> the table [S,T,HH,WW,2] that carries it in every cell."""
    shift = np.asarray(shift, np.int64)
    return np.ascontiguousarray(np.broadcast_to(shift[:, :, None, None, :], shift.shape[:2] + (HH, WW, 2)))


# ------------------------------------------------------------------ the inputs the CPU and GPU tests share
# name: (S, T, HH, WW, K, R, sigma, rho, the kind of table case_table() builds)
CASES = {
    # odd sizes, interleaved channels, two sequences, a sigma per joint; every cell its own shift, some beyond R = 3
    'odd': (2, 5, 13, 17, 3, 3, (0.8, 1.5, 2.5), 0.05, ('random', 4)),
    # HW * K a multiple of 4: the float4 staging
    'vector': (2, 3, 6, 10, 3, 2, 1.0, 0.05, ('random', 3)),
    # R above both sides and shifts in +-9: every tap range clipped, some cells with every tap clipped on one side, some with no tap inside the map
    'clipped': (1, 3, 5, 7, 2, 8, 3.0, 0.05, ('random', 9, {(4, 6): (9, 9), (0, 0): (-9, 2), (2, 0): (1, -9)})),
    # entries at the ends of int32 among small ones: the clamp is there so that no index sum overflows
    'far': (1, 3, 5, 7, 1, 2, 1.0, 0.05, ('far',)),
    # rho = 0 and frame 2's table sends every cell off the map: the filter resets (1), Viterbi breaks (1)
    'lost': (1, 3, 13, 17, 3, 3, 1.5, 0.0, ('lost', 2)),
    'radius0': (1, 3, 5, 7, 2, 0, 1.0, 0.05, ('random', 2)),
    # 8192 cells, the LDS limit: every thread has eight cells
    'big': (1, 2, 64, 128, 1, 2, 1.0, 0.05, ('blocks', 2, 8)),
    # the geometry of the tower's maps, once, with a block-wise constant table of +-2 (what a flow of moving parts looks like)
    'real': (1, 4, 60, 90, 9, 5, 1.5, 0.05, ('blocks', 2, 10)),
}


def case_table(name):
    """The centre table int64 [S,T,HH,WW,2] of CASES[name], from a seed of its own (the maps' seed is searched for, the table stays)."""
    S, T, HH, WW, K, R_, sigma, rho, kind = CASES[name]
    rs = np.random.RandomState(7000 + sorted(CASES).index(name))
    if kind[0] == 'random':      # every cell its own shift; kind[2]: cells whose shift is set, whatever the draw
        table = rs.randint(-kind[1], kind[1] + 1, (S, T, HH, WW, 2)).astype(np.int64)
        for (y, x), s in (kind[2] if len(kind) > 2 else {}).items():
            table[:, :, y, x] = s
        return table
    if kind[0] == 'blocks':      # one shift per block of kind[2] x kind[2] cells
        side = kind[2]
        coarse = rs.randint(-kind[1], kind[1] + 1, (S, T, -(-HH // side), -(-WW // side), 2))
        return np.repeat(np.repeat(coarse, side, axis=2), side, axis=3)[:, :, :HH, :WW].astype(np.int64)
    if kind[0] == 'far':
        values = np.array([INT_MIN, -INT_MAX, INT_MAX, -1, 0, 1, 2], np.int64)
        table = values[rs.randint(0, len(values), (S, T, HH, WW, 2))]
        table[:, :, 0, 0] = (INT_MIN, INT_MIN)      # every extreme pairing occurs whatever the draw
        table[:, :, 0, 1] = (INT_MAX, INT_MAX)
        table[:, :, 1, 0] = (INT_MIN, INT_MAX)
        table[:, :, 1, 1] = (0, -INT_MAX)
        table[:, :, 2, 2] = (0, 0)
        return table
    if kind[0] == 'lost':
        table = rs.randint(-2, 3, (S, T, HH, WW, 2)).astype(np.int64)
        off = np.array([(HH + R_, 0), (-(HH + R_), 1), (0, WW + R_), (2, -(WW + R_)), (INT_MAX, 0), (0, INT_MIN)], np.int64)
        table[:, kind[1]] = off[rs.randint(0, len(off), (S, HH, WW))]
        return table
    raise KeyError(kind)


def case_inputs(name, taps_of):
    """(hm, taps, R, sigma, rho, centre int64 [S,T,HH,WW,2], seed) of CASES[name]; taps_of = predict.seq_taps.  As seq_moving_ref.case_inputs: the seed
    is the first from 0 at which the RESTATEMENT's filtered belief has, in every map, a relative top-2 gap above ten times seq_ref.tolerance -- a
    condition on the inputs that the restatement alone decides, so that a coordinate mismatch cannot be blamed on a tie."""
    S, T, HH, WW, K, R_, sigma, rho, _ = CASES[name]
    centre = case_table(name)
    taps = taps_of(sigma, R_, K)
    for seed in range(100):
        hm = R.random_maps((S, T, HH, WW, K), 3000 + seed)
        if gap_holds(hm, taps, rho, R_, centre):
            return hm, taps, R_, sigma, rho, centre, seed
    raise AssertionError('no seed below 100 gives case %r a top-2 gap' % name)


def gap_holds(hm, taps, rho, R_, centre):
    S, T, HH, WW, K = hm.shape
    gap = R.top2_gap(seq_filter(hm, taps, rho, centre)['belief'])
    need = np.array([10.0 * R.tolerance(t, HH * WW, R_) for t in range(T)])
    return bool((gap > need[None, :, None]).all())
