"""A numpy restatement of jcm_seq_tracks_viterbi / jcm_seq_tracks_filter (include/jcm.h) on top of tests/seq_ref.py: a loop over
the tracks that zeroes the neighbourhoods of the earlier tracks' cells and calls seq_ref.seq_viterbi / seq_ref.seq_filter(kernel_order=True) at
K = 1.  Nothing of the temporal model is stated here a second time."""
import numpy as np

import seq_ref


def masked(hm, cells, value, D):
    """hm float32 [S,T,HH,WW]; cells int [S,n,T,2] and value [S,n,T] of the n earlier tracks -> the observation of pass n: hm with the cells
    within D (Chebyshev) of an earlier track's cell zeroed, in the frames where that track's value is positive."""
    p = np.array(hm, np.float32)
    S, T, HH, WW = p.shape
    ys, xs = np.mgrid[0:HH, 0:WW]
    for s in range(S):
        for m in range(cells.shape[1]):
            for t in range(T):
                if value[s, m, t] > 0:
                    y, x = cells[s, m, t]
                    p[s, t][np.maximum(np.abs(ys - y), np.abs(xs - x)) <= D] = 0
    return p


def _value(p, cells):
    S, T = p.shape[:2]
    return np.array([[p[s, t, cells[s, t, 0], cells[s, t, 1]] for t in range(T)] for s in range(S)], np.float32)


def seq_tracks_viterbi(hm, M, taps, rho, D):
    """hm float32 [S,T,HH,WW], taps float64 [1,2R+1] -> {'path' int32 [S,M,T,2], 'maxes' float64 [S,M,T], 'breaks' int32 [S,M,T], 'value' float32
    [S,M,T]}."""
    hm = np.asarray(hm, np.float32)
    S, T = hm.shape[:2]
    out = {'path': np.zeros((S, M, T, 2), np.int32), 'maxes': np.zeros((S, M, T)), 'breaks': np.zeros((S, M, T), np.int32),
           'value': np.zeros((S, M, T), np.float32)}
    for n in range(M):
        p = masked(hm, out['path'][:, :n], out['value'][:, :n], D)
        r = seq_ref.seq_viterbi(p[..., None], taps, rho)
        out['path'][:, n], out['maxes'][:, n], out['breaks'][:, n] = r['path'][..., 0], r['maxes'][..., 0], r['breaks'][..., 0]
        out['value'][:, n] = _value(p, out['path'][:, n])
    return out


def seq_tracks_filter(hm, M, taps, rho, D, state=None):
    """state float64 [S,M,HH*WW] or None -> {'coords' int32 [S,M,T,2], 'norm' float64 [S,M,T], 'reset' int32 [S,M,T], 'value' float32 [S,M,T],
    'state' float64 [S,M,HH*WW], 'filtered' float32 [S,M,T,HH,WW]}."""
    hm = np.asarray(hm, np.float32)
    S, T, HH, WW = hm.shape
    out = {'coords': np.zeros((S, M, T, 2), np.int32), 'norm': np.zeros((S, M, T)), 'reset': np.zeros((S, M, T), np.int32),
           'value': np.zeros((S, M, T), np.float32), 'state': np.zeros((S, M, HH * WW)), 'filtered': np.zeros((S, M, T, HH, WW), np.float32)}
    for n in range(M):
        p = masked(hm, out['coords'][:, :n], out['value'][:, :n], D)
        st = None if state is None else np.asarray(state, np.float64)[:, n].reshape(S, 1, HH, WW)
        r = seq_ref.seq_filter(p[..., None], taps, rho, state=st, kernel_order=True)
        out['coords'][:, n], out['norm'][:, n], out['reset'][:, n] = r['coords'][..., 0], r['norm'][..., 0], r['reset'][..., 0]
        out['state'][:, n], out['filtered'][:, n] = r['state'].reshape(S, HH * WW), r['filtered'][..., 0]
        out['value'][:, n] = _value(p, out['coords'][:, n])
    return out
