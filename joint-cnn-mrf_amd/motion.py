"""The motion model of the sequence stages: a joint moves by a truncated Gaussian step per frame, in heat-map cells, or -- with
mass rho -- jumps anywhere.  Host arithmetic in float64, numpy only: the constants, the taps the library takes (seq_taps), the per-mode keys of what
the scans return (SEQ_KEYS) and the EM fit of sigma and rho to a clip's own maps (seq_fit; the engine is an argument).  engine/sequence.py and the
prediction modules both read this module; it imports neither."""
import numpy as np

# The standard deviation of a joint's motion per frame in heat-map cells, and the mass of the uniform "anywhere" term.  Untuned placeholders: no
# consecutive-frame data is at hand to derive them from.
SEQ_SIGMA = 1.5
SEQ_RHO = 0.05
SEQ_TORSO_SIGMA = 1.5                     # a torso's motion per frame in cells (predict_sequence_people): an untuned placeholder
SEQ_RADIUS_MAX = 16                       # include/jcm.h: R of jcm_seq_filter / jcm_seq_viterbi
SEQ_SIGMA_MAX = 64.0                      # what seq_fit clamps a joint's sigma to when its moment reaches that of flat taps (at R = 16 such taps are flat within 3 %)
SEQ_MODES = ('filter', 'viterbi', 'marginal', 'lag')
SEQ_EXCLUDE = 4                           # the exclusion half-width of Engine.seq_tracks, cells: an untuned placeholder
# Per mode, what the scans of the engine return per frame: the key of the cells, then those of a 'track' beside the points -- (cells, value, flag) but for 'marginal'
# and 'lag' (the fixed-lag smoother, DESIGN.md 4.25: the marginal's keys and the lag the frame got).
SEQ_KEYS = {'filter': ('coords', 'norm', 'reset'), 'viterbi': ('path', 'maxes', 'breaks'), 'marginal': ('coords', 'conf', 'norm', 'reset', 'cut'),
            'lag': ('coords', 'conf', 'norm', 'reset', 'cut', 'lag')}


SEQ_CAMERA_SEARCH = 8                     # the coarse search radius of Engine.frame_shift: reaches +-(4 * 8 + 3) = 35 fitted pixels a frame; an untuned placeholder


def camera_shifts(disp, carry=(0, 0), stride=8):
    """The camera's displacement per frame in fitted-frame pixels (Engine.frame_shift's 'disp', int [T,2] = (dy, dx)) -> (shift int32 [T,2], carry):
    the whole-cell lattice shift per frame that Engine.seq_filter / seq_viterbi(shift=) take.  Exact integer arithmetic:
      c_t = carry + disp_0 + .. + disp_t        the cumulative displacement in pixels
      o_t = (c_t + stride // 2) // stride       floor division: the cumulative displacement in cells, rounded to the nearest
      shift_t = o_t - o_{t-1}                   with o_{-1} = (carry + stride // 2) // stride
    so the shifts of any run of frames add up to the rounded cumulative displacement and rounding never accumulates; what is left, at most half
    a cell, is motion the taps (sigma) have to cover.  carry, a pair of ints, holds the part of the cumulative displacement of all frames so far
    that has not become whole cells: c_{T-1} - stride * o_{T-1}, in [-(stride // 2), stride - stride // 2).  Pass the returned carry to the call
    for the next frames of the clip ((0, 0) at a clip's start): any split of a clip gives the shifts of one call."""
    stride = int(stride)
    if stride < 1:
        raise ValueError('stride must be >= 1, got %r' % (stride,))
    d = np.asarray(disp)
    if d.dtype.kind not in 'iu' or d.ndim != 2 or d.shape[1] != 2:
        raise ValueError('disp must be an integer array [T,2], got %s %s' % (d.dtype, d.shape))
    c0 = np.array([int(carry[0]), int(carry[1])], np.int64)
    c = c0[None, :] + np.cumsum(d.astype(np.int64), axis=0)
    half = stride // 2
    o = np.concatenate([((c0 + half) // stride)[None, :], (c + half) // stride])
    last = c[-1] - stride * o[-1] if len(c) else c0 - stride * o[0]
    return (o[1:] - o[:-1]).astype(np.int32), (int(last[0]), int(last[1]))


SEQ_FLOW_SEARCH = 8                       # the search radius of Engine.frame_flow in fitted pixels, one heat-map cell a frame: an untuned placeholder
SEQ_FLOW_MAX = 4                          # include/jcm.h: N of jcm_hm_flow_pool


def _flow_n(N):
    if isinstance(N, bool) or not isinstance(N, (int, np.integer)) or not 1 <= int(N) <= SEQ_FLOW_MAX:
        raise ValueError('flow must be the neighbours on either side, an integer in 1..4, got %r' % (N,))
    return int(N)


def flow_refs(T, N):
    """The reference frames of Engine.frame_flow in the layout Engine.hm_flow_pool reads: int32 [T,2N], slot 2(n-1) = t - n and
    slot 2(n-1) + 1 = t + n for n = 1 .. N, -1 where that frame is outside the clip."""
    T, N = int(T), _flow_n(N)
    if T < 1:
        raise ValueError('T must be >= 1, got %r' % (T,))
    t, n = np.arange(T, dtype=np.int64)[:, None], np.arange(1, N + 1, dtype=np.int64)[None, :]
    ref = np.stack([t - n, t + n], axis=2).reshape(T, 2 * N)
    return np.where((ref < 0) | (ref >= T), -1, ref).astype(np.int32)


def flow_weights(N):
    """The pooling weights of Engine.hm_flow_pool, float64 [N+1]: uniform -- the frame and every neighbour count alike.  An untuned placeholder."""
    return np.ones(_flow_n(N) + 1, np.float64)


def flow_cell_shifts(flow, stride=8):
    """One slot of Engine.frame_flow's 'flow', int [T,HH,WW,2] = (dy, dx) in fitted-frame pixels -> int32 of the same shape = (sy, sx) in heat-map
    cells: the `centre` of Engine.seq_filter / seq_viterbi.  The rule, per component d:
      s = floor((d + stride // 2) / stride)      floor division in integer arithmetic: the nearest cell, a half rounds up
    so with stride 8: 3 -> 0, 4 -> 1, -4 -> 0, -5 -> -1.  The signs agree as they are: the content at pixel (y, x) of frame t is at (y + dy, x + dx) of
    the reference frame, and cell (y, x) of frame t was cell (y + sy, x + sx) of frame t-1 when the slot's reference is t-1.  flow: a torch tensor
    (the arithmetic runs on its own device, nothing is read back) or a numpy array.  A whole-pixel flow becomes whole cells: what is left, at most
    half a cell, is motion the taps (sigma) have to cover."""
    stride = int(stride)
    if stride < 1:
        raise ValueError('stride must be >= 1, got %r' % (stride,))
    if isinstance(flow, np.ndarray):
        if flow.dtype.kind not in 'iu':
            raise ValueError('flow must be an integer array, got %s' % (flow.dtype,))
        return ((flow.astype(np.int64) + stride // 2) // stride).astype(np.int32)
    if flow.dtype.is_floating_point or flow.dtype.is_complex:      # a torch tensor: this module does not import torch
        raise ValueError('flow must be an integer tensor, got %s' % (flow.dtype,))
    return ((flow.long() + stride // 2) // stride).int()


def _seq_sigma(sigma, K=None):
    sg = np.asarray(sigma, np.float64).reshape(-1)
    if sg.size == 0 or not np.all(np.isfinite(sg)) or np.any(sg <= 0):
        raise ValueError('sigma must be positive and finite, got %r' % (sigma,))
    if K is not None:
        if sg.size not in (1, K):
            raise ValueError('sigma must be a scalar or %d values (one per joint), got %d' % (K, sg.size))
        sg = np.broadcast_to(sg, (K,))
    return sg


def seq_radius(sigma):
    """The default tap radius of the sequence stages: min(16, ceil(3 * max sigma))."""
    return int(min(SEQ_RADIUS_MAX, np.ceil(3.0 * _seq_sigma(sigma).max())))


def seq_taps(sigma, radius, K):
    """The 1-D taps of the motion kernel jcm_seq_filter / jcm_seq_viterbi take: float64 [K, 2 * radius + 1], row k = exp(-d^2 / (2 sigma_k^2)) for
    d = -radius .. radius, divided by its sum.  sigma: a scalar or K values, in heat-map cells per frame.  The one builder: Engine.seq_* and the
    restatement of the tests share it."""
    R = int(radius)
    if R < 0:
        raise ValueError('radius must be >= 0, got %r' % (radius,))
    sg = _seq_sigma(sigma, int(K))
    d = np.arange(-R, R + 1, dtype=np.float64)
    w = np.exp(-(d[None, :] * d[None, :]) / (2.0 * sg[:, None] * sg[:, None]))
    return np.ascontiguousarray(w / w.sum(axis=1, keepdims=True))


def seq_kernel(sigma, radius, K):
    """(R, host taps [K, 2R+1]) of an Engine.seq_* call; radius None is seq_radius(sigma).  R is checked before the taps are built, and again by the library."""
    R = seq_radius(sigma) if radius is None else int(radius)
    if not 0 <= R <= SEQ_RADIUS_MAX:
        raise ValueError('radius must be in 0..16, got %r' % (radius,))
    return R, seq_taps(sigma, R, K)


def seq_pose_tau(cells, count, sigma, rho, radius=None, weight=1.0, hw=5400):
    """The transition tables of the clip decode (Engine.seq_pose_viterbi) from the candidates of a clip: cells int [T,K,P,2] (row, col),
    count int [T,K] as hm_peaks leaves them, host arrays -> float64 [T,K,P,P],
        tau[t,j,a,b] = weight * log(om * w_j[dy + R] * w_j[dx + R] + u),   (dy, dx) = cell_b(t) - cell_a(t-1),
    with (R, w) = seq_kernel(sigma, radius, K), om = 1 - rho and u = rho / hw: the taps and the two constants of Engine.seq_viterbi, so a candidate
    pair scores what that scan's transition gives its two cells.  Outside the radius the product is 0: with rho = 0 the entry is -inf.  tau[0] and
    every slot at or beyond count are 0 and are never read.  weight mixes two log-scores of different origin; 1.0 is an untuned placeholder."""
    cells, count = np.asarray(cells, np.int64), np.asarray(count, np.int64)
    if cells.ndim != 4 or cells.shape[3] != 2 or count.shape != cells.shape[:2]:
        raise ValueError('seq_pose_tau expects cells [T,K,P,2] and count [T,K]; got %s, %s' % (cells.shape, count.shape))
    if not 0.0 <= float(rho) <= 1.0 or not np.isfinite(float(weight)) or float(weight) < 0.0:
        raise ValueError('seq_pose_tau expects rho in [0,1] and a finite weight >= 0; got %r, %r' % (rho, weight))
    T, K, P = cells.shape[:3]
    R, w = seq_kernel(sigma, radius, K)
    om, u = 1.0 - float(rho), float(rho) / float(hw)
    tau = np.zeros((T, K, P, P), np.float64)
    if T < 2:
        return tau
    d = cells[1:, :, None, :, :] - cells[:-1, :, :, None, :]                     # [T-1,K,a,b,2]
    near = (np.abs(d) <= R).all(axis=4)
    tap = lambda k: np.where(near, np.take_along_axis(w[None, :, None, :], np.clip(d[..., k] + R, 0, 2 * R).reshape(T - 1, K, 1, P * P), axis=3).reshape(T - 1, K, P, P), 0.0)
    n = np.clip(count, 0, P)
    live = (np.arange(P)[None, None, :, None] < n[:-1, :, None, None]) & (np.arange(P)[None, None, None, :] < n[1:, :, None, None])
    with np.errstate(divide='ignore', invalid='ignore'):
        val = float(weight) * np.log(om * tap(0) * tap(1) + u)
    if float(weight) == 0.0:
        val = np.where(np.isnan(val), 0.0, val)      # 0 * -inf: a weight of 0 switches the motion term off, also where it forbids
    tau[1:] = np.where(live, val, 0.0)
    return tau


def seq_moment(sigma, radius):
    """sum over d of d^2 w_sigma[d] of the truncated taps seq_taps builds: the 1-D second moment of the motion kernel, float64.  Monotone in sigma,
    from 0 towards the flat taps' R (R + 1) / 3."""
    R = int(radius)
    d = np.arange(-R, R + 1, dtype=np.float64)
    return float(np.sum(d * d * seq_taps(sigma, R, 1)[0]))


def seq_sigma_of_moment(target, radius, sigma_max=SEQ_SIGMA_MAX):
    """The M-step of one joint: the sigma whose truncated taps have seq_moment == target, by bisection in float64 -> (sigma, clamped).  A target at or
    above the flat taps' R (R + 1) / 3 (no sigma reaches it), or one only a sigma above sigma_max reaches, gives (sigma_max, True); a target so small
    that no representable taps have it gives the lower end of the bracket, 2^-6 cells."""
    R = int(radius)
    target = float(target)
    if R < 1:
        raise ValueError('a motion kernel of radius 0 has no sigma to fit')
    if not target < R * (R + 1) / 3.0 or seq_moment(sigma_max, R) <= target:
        return float(sigma_max), True
    lo, hi = 2.0 ** -6, float(sigma_max)
    if seq_moment(lo, R) >= target:
        return lo, False
    for _ in range(200):      # moment(lo) < target <= moment(hi) throughout
        mid = 0.5 * (lo + hi)
        if mid <= lo or mid >= hi:
            break
        if seq_moment(mid, R) < target:
            lo = mid
        else:
            hi = mid
    return (lo if abs(seq_moment(lo, R) - target) <= abs(seq_moment(hi, R) - target) else hi), False


def seq_m_step(trans_sum, sigma, rho, radius, fit_rho=True, sigma_max=SEQ_SIGMA_MAX):
    """trans_sum float64 [K,3] = (moved, jumped, squared displacement) summed over sequences and frames; sigma [K], rho: the current values ->
    (sigma' [K], rho', clamped bool [K]).  rho' = sum jumped / (sum moved + sum jumped) over all joints (rho when that is 0 / 0, or with
    fit_rho=False); sigma_k' solves seq_moment(sigma_k') = squared_k / (2 moved_k) -- the displacement has two axes with the same taps -- and a
    joint with moved_k == 0 keeps its sigma."""
    tr = np.asarray(trans_sum, np.float64)
    sigma = np.array(sigma, np.float64)
    move, jump, sq = tr[:, 0], tr[:, 1], tr[:, 2]
    total = move.sum() + jump.sum()
    new_rho = float(jump.sum() / total) if fit_rho and total > 0 else float(rho)
    new_sigma, clamped = sigma.copy(), np.zeros(sigma.shape, bool)
    for k in range(sigma.size):
        if move[k] > 0:
            new_sigma[k], clamped[k] = seq_sigma_of_moment(sq[k] / (2.0 * move[k]), radius, sigma_max)
    return new_sigma, min(max(new_rho, 0.0), 1.0), clamped


def seq_fit(engine, hm, sigma=SEQ_SIGMA, rho=SEQ_RHO, iters=10, radius=16, fit_rho=True):
    """Fit the motion model to a clip without annotations (Baum-Welch).  hm [T,HH,WW,K] or [S,T,HH,WW,K] device maps as for
    Engine.seq_smooth; sigma (a scalar or K values) and rho are the start.  Each of the `iters` iterations is one Engine.seq_smooth at the current
    values (E-step), whose 'trans' is read back and summed over s and t on the host in float64 (np.sum over the two axes), and seq_m_step
    (M-step).  Returns {'sigma' float64 [K], 'rho' float, 'loglik' float64 [iters + 1] -- the sum over sequences, frames and joints of log norm
    (frames with norm 0, reset 2, left out) at the values BEFORE each iteration and, last, at the returned ones (one more seq_smooth) --,
    'history' [(sigma [K], rho)] * (iters + 1), the values the entries of loglik belong to, 'clamped' bool [K]: the joints whose sigma the last
    M-step held at SEQ_SIGMA_MAX}.
    What is approximate: the motion kernel is not renormalised at the map's border (cells outside contribute nothing), so the transition rows of
    cells within `radius` of the border sum to less than 1 and the M-step -- exact EM for mass away from the border -- slightly overstates rho and
    understates sigma for tracks along it; and the taps are truncated at `radius`, so no sigma explains a mean squared step of R (R + 1) / 3 per
    axis or more: such a joint is clamped and reported.  radius is fixed over the iterations (16, the largest, by default) so that a growing sigma
    is not cut off by the radius its start implied."""
    iters = int(iters)
    if iters < 1:
        raise ValueError('iters must be >= 1, got %r' % (iters,))
    K = int(hm.shape[-1])
    sg = np.array(_seq_sigma(sigma, K), np.float64)
    rho = float(rho)
    R = int(radius)
    loglik, history = [], []
    clamped = np.zeros(K, bool)

    def e_step():
        r = engine.seq_smooth(hm, sg, rho, radius=R, want_smoothed=False)
        norm = r['norm'].cpu().numpy().reshape(-1)
        loglik.append(float(np.sum(np.log(norm[norm > 0]))))
        history.append((sg.copy(), rho))
        return r['trans'].cpu().numpy().reshape(-1, K, 3).sum(axis=0)

    for _ in range(iters):
        sg, rho, clamped = seq_m_step(e_step(), sg, rho, R, fit_rho=fit_rho)
    e_step()
    return {'sigma': sg, 'rho': rho, 'loglik': np.array(loglik, np.float64), 'history': history, 'clamped': clamped}
