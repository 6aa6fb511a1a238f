"""The fixed-lag smoother (include/jcm.h: jcm_seq_smooth_lag) restated AS ITS DEFINITION: the outputs of frame s are what the
restatement of the offline smoother (seq_smooth_ref.seq_smooth, pinned by tests/test_seq_smooth_cpu.py) writes for frame s when given frames
0 .. h(s) of the clip, h(s) = s + L, or min(s + L, N - 1) at a flush.  No window, no carried belief and no backward pass of its own: one offline
smoother per truncation.  It follows the push schedule, so the number of frames every push emits is restated too.  Beside it the inputs the CPU
and the GPU tests share."""
import functools

import numpy as np

import seq_ref as R
import seq_smooth_ref as SR

KEYS = ('gamma', 'smoothed', 'coords', 'conf', 'norm', 'reset', 'mass', 'cut')


def seq_smooth_lag(hm, taps, rho, L, splits, flush_last=True, smooth=None):
    """hm float32 [S,T,HH,WW,K], taps float64 [K,2R+1]; splits: the new frames of every push, in order (their sum is T); flush_last: whether the
    last push flushes the clip.  smooth(n): the offline restatement on frames 0 .. n-1 (default: computed here, once per n).
    Returns one dict per push: the outputs of the frames that push emits, stacked on axis 1 ([S,E,...], E may be 0), 'lag' int32 [E] (the lag
    each frame got) and 'frames', the clip's indices of those frames."""
    hm = np.asarray(hm, np.float32)
    S, T, HH, WW, K = hm.shape
    L = int(L)
    assert L >= 1 and sum(splits) == T and all(n >= 0 for n in splits)
    known = {}

    def prefix(n):
        if n not in known:
            known[n] = smooth(n) if smooth else SR.seq_smooth(hm[:, :n], taps, rho)
        return known[n]

    pushes, N, nxt = [], 0, 0
    for i, n_new in enumerate(splits):
        N += n_new
        flush = flush_last and i == len(splits) - 1
        frames, horizon = [], []
        while nxt < N and (flush or nxt + L <= N - 1):
            frames.append(nxt)
            horizon.append(min(nxt + L, N - 1) if flush else nxt + L)
            nxt += 1
        out = {}
        for key in KEYS:
            like = prefix(1)[key]
            rows = [prefix(h + 1)[key][:, s] for s, h in zip(frames, horizon)]
            out[key] = np.stack(rows, axis=1) if rows else np.zeros((S, 0) + like.shape[2:], like.dtype)
        out['lag'] = np.array([h - s for s, h in zip(frames, horizon)], np.int32)
        out['frames'] = np.array(frames, np.int64)
        pushes.append(out)
    return pushes


def emitted_counts(splits, L, flush_last=True):
    """The formula of include/jcm.h, push by push: the window is the P pending frames and the new ones, E = flush ? W : max(0, W - L)."""
    counts, P = [], 0
    for i, n_new in enumerate(splits):
        W = P + n_new
        E = W if flush_last and i == len(splits) - 1 else max(0, W - L)
        counts.append(E)
        P = W - E
    return counts


def joined(pushes, keys=KEYS + ('lag',)):
    """The pushes' outputs one behind the other: what one call over the clip gives when the split does not matter."""
    return {k: np.concatenate([p[k] for p in pushes], axis=0 if k == 'lag' else 1) for k in keys}


# ------------------------------------------------------------------ the inputs the CPU and GPU tests share
CASES = SR.CASES      # seq_ref's geometries and the map at the cell limit


def gaps_hold(prefixes, HW, Rr):
    """Every gamma of every truncation has a relative top-2 gap above ten times the rounding bound of its 2 n steps (seq_ref.tolerance)."""
    return all((R.top2_gap(ref['gamma']) > 10.0 * R.tolerance(2 * n, HW, Rr)).all() for n, ref in prefixes.items())


@functools.lru_cache(maxsize=None)
def case(name):
    """(hm, taps, R, sigma, rho, seed, prefixes) of CASES[name], computed once and never written to; prefixes[n] is the offline restatement on
    frames 0 .. n-1, n = 1 .. T.  The seed is the first from 0 at which EVERY truncated gamma of the reference -- every frame of every prefix,
    so every lag and every schedule -- has a clear first maximum (gaps_hold): a condition the reference alone decides."""
    from joint_cnn_mrf_amd import predict as P
    S, T, HH, WW, K, Rr, sigma, rho = CASES[name]
    taps = P.seq_taps(sigma, Rr, K)
    for seed in range(100):
        hm = R.random_maps((S, T, HH, WW, K), 1000 + seed)
        prefixes = {n: SR.seq_smooth(hm[:, :n], taps, rho) for n in range(1, T + 1)}
        if gaps_hold(prefixes, HH * WW, Rr):
            return hm, taps, Rr, sigma, rho, seed, prefixes
    raise AssertionError('no seed below 100 gives case %r a top-2 gap in every truncation' % name)


def case_lag(name, L, splits=None, flush_last=True):
    """The restatement on case(name) at lag L; splits defaults to one push of the whole clip."""
    hm, taps, Rr, sigma, rho, _, prefixes = case(name)
    return seq_smooth_lag(hm, taps, rho, L, splits or (hm.shape[1],), flush_last, smooth=prefixes.__getitem__)
