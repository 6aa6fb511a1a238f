"""A numpy float64 restatement of jcm_seq_smooth (include/jcm.h): the forward is seq_ref.seq_filter in the kernel's order, the backward
the stated recurrence with explicit tap loops, one rounded operation per step, every sum seq_ref.kernel_sum -- so the device can be compared bit for
bit.  Beside it an INDEPENDENT smoother that builds the joint distribution of all HW^T paths of a tiny chain and reads every marginal and every
transition statistic off it (no forward-backward recursion in it), the EM loop of predict.seq_fit on the restatement, and the planted clip the CPU
and the GPU tests share."""
import functools

import numpy as np

import seq_ref as R


def blur_adjoint(q, w, w2, Rr):
    """(m, sq) of the backward pass: the vertical then the horizontal pass with the adjoint index, terms outside the map skipped, ascending from 0.0."""
    HH, WW = q.shape
    c, c2 = np.zeros_like(q), np.zeros_like(q)
    for dy in range(-Rr, Rr + 1):
        y0, y1 = R._rows(HH, -dy)      # the cells y with 0 <= y + dy < HH
        if y0 < y1:
            c[y0:y1] = c[y0:y1] + w[dy + Rr] * q[y0 + dy:y1 + dy]
            c2[y0:y1] = c2[y0:y1] + w2[dy + Rr] * q[y0 + dy:y1 + dy]
    m, sx, sy = np.zeros_like(q), np.zeros_like(q), np.zeros_like(q)
    for dx in range(-Rr, Rr + 1):
        x0, x1 = R._rows(WW, -dx)
        if x0 < x1:
            m[:, x0:x1] = m[:, x0:x1] + w[dx + Rr] * c[:, x0 + dx:x1 + dx]
            sx[:, x0:x1] = sx[:, x0:x1] + w2[dx + Rr] * c[:, x0 + dx:x1 + dx]
            sy[:, x0:x1] = sy[:, x0:x1] + w[dx + Rr] * c2[:, x0 + dx:x1 + dx]
    return m, sx + sy


def seq_smooth(hm, taps, rho):
    """hm float32 [S,T,HH,WW,K], taps float64 [K,2R+1] -> {'gamma' float64 [S,T,HH,WW,K] ('smoothed' is its float32 rounding), 'smoothed', 'coords'
    int32 [S,T,2,K], 'conf' float32 [S,T,K], 'norm', 'reset' (the filter's), 'mass' float64 [S,T,K], 'cut' int32 [S,T,K], 'trans' float64 [S,T,K,3]}."""
    hm = np.asarray(hm, np.float32)
    taps = np.asarray(taps, np.float64)
    S, T, HH, WW, K = hm.shape
    Rr = (taps.shape[1] - 1) // 2
    HW = HH * WW
    om, u = np.float64(1.0) - np.float64(rho), np.float64(rho) / np.float64(HW)
    fwd = R.seq_filter(hm, taps, rho, kernel_order=True)
    a, norm, reset = fwd['belief'], fwd['norm'], fwd['reset']
    d = np.arange(-Rr, Rr + 1)
    gamma = np.zeros((S, T, HH, WW, K), np.float64)
    coords = np.zeros((S, T, 2, K), np.int32)
    conf = np.zeros((S, T, K), np.float32)
    mass = np.zeros((S, T, K), np.float64)
    cut = np.zeros((S, T, K), np.int32)
    trans = np.zeros((S, T, K, 3), np.float64)
    for s in range(S):
        for k in range(K):
            w = taps[k]
            w2 = (d * d).astype(np.float64) * w
            beta = np.ones((HH, WW), np.float64)
            for t in range(T - 1, -1, -1):
                at = a[s, t, :, :, k]
                g = at * beta
                G = R.kernel_sum(g)
                if G > 0.0 and np.isfinite(G):
                    gam = g / G
                else:
                    gam = at.copy()
                    cut[s, t, k] = 1
                    beta = np.ones((HH, WW), np.float64)
                gamma[s, t, :, :, k] = gam
                i = R._argmax(gam)
                coords[s, t, :, k] = (i // WW, i % WW)
                conf[s, t, k] = np.float32(gam.reshape(-1)[i])
                mass[s, t, k] = G
                if t >= 1:
                    if reset[s, t, k] != 0:
                        beta = np.ones((HH, WW), np.float64)
                    else:
                        Z = norm[s, t, k]
                        q = hm[s, t, :, :, k].astype(np.float64) * beta
                        Q = R.kernel_sum(q)
                        m, sq = blur_adjoint(q, w, w2, Rr)
                        uQ = u * Q
                        prev = a[s, t - 1, :, :, k]
                        trans[s, t, k] = ((om * R.kernel_sum(prev * m)) / Z, uQ / Z, (om * R.kernel_sum(prev * sq)) / Z)
                        beta = (om * m + uQ) / Z
    return {'gamma': gamma, 'smoothed': gamma.astype(np.float32), 'coords': coords, 'conf': conf, 'norm': norm, 'reset': reset, 'mass': mass, 'cut': cut,
            'trans': trans}


def brute_force(hm, taps, rho):
    """The smoother of ONE (sequence, joint) of a tiny chain by enumeration: hm float32 [T,HH,WW], taps float64 [2R+1] -> (gamma float64 [T,HH,WW],
    trans float64 [T,3]).  The joint weight of every path x_0 .. x_{T-1} is p_0(x_0) prod_t (om K(x_t - x_{t-1}) + u) p_t(x_t) with
    K(d) = w[dy+R] w[dx+R] inside the radius and 0 outside; all HW^T of them are held at once.  Needs positive total weight (no reset)."""
    hm = np.asarray(hm, np.float64)
    w = np.asarray(taps, np.float64)
    T, HH, WW = hm.shape
    Rr = (w.size - 1) // 2
    HW = HH * WW
    om, u = 1.0 - float(rho), float(rho) / HW
    ys, xs = np.divmod(np.arange(HW), WW)
    dy, dx = ys[None, :] - ys[:, None], xs[None, :] - xs[:, None]      # [from, to]
    inside = (np.abs(dy) <= Rr) & (np.abs(dx) <= Rr)
    kern = np.where(inside, w[np.clip(dy + Rr, 0, 2 * Rr)] * w[np.clip(dx + Rr, 0, 2 * Rr)], 0.0)
    move, full = om * kern, om * kern + u
    share = np.where(full > 0, move / np.where(full > 0, full, 1.0), 0.0)      # of a transition's weight, the part that moved
    dist2 = (dy * dy + dx * dx).astype(np.float64)
    p = hm.reshape(T, HW)
    joint = p[0].copy()
    for t in range(1, T):      # axis t of `joint` is x_t
        joint = joint[..., None] * full.reshape((1,) * (t - 1) + (HW, HW)) * p[t].reshape((1,) * t + (HW,))
    total = joint.sum()
    gamma = np.stack([joint.sum(axis=tuple(a for a in range(T) if a != t)) for t in range(T)]) / total
    trans = np.zeros((T, 3))
    for t in range(1, T):
        pair = joint.sum(axis=tuple(a for a in range(T) if a not in (t - 1, t))) / total      # [x_{t-1}, x_t]
        trans[t] = ((pair * share).sum(), (pair * (1.0 - share)).sum(), (pair * share * dist2).sum())
    return gamma.reshape(T, HH, WW), trans


def seq_fit(hm, sigma, rho, iters, radius, P, fit_rho=True, smooth=None):
    """predict.seq_fit with the restatement in the engine's place (P = the predict module, whose seq_taps and seq_m_step it shares): the same
    host float64 sums, so it is bit-equal to the device's fit as long as the device's outputs are."""
    K = hm.shape[-1]
    sg = np.array(np.broadcast_to(np.asarray(sigma, np.float64), (K,)))
    rho = float(rho)
    loglik, history = [], []
    clamped = np.zeros(K, bool)

    def e_step():
        r = (smooth or seq_smooth)(hm, P.seq_taps(sg, radius, K), rho)
        norm = r['norm'].reshape(-1)
        loglik.append(float(np.sum(np.log(norm[norm > 0]))))
        history.append((sg.copy(), rho))
        return r['trans'].reshape(-1, K, 3).sum(axis=0)

    for _ in range(iters):
        sg, rho, clamped = P.seq_m_step(e_step(), sg, rho, radius, fit_rho=fit_rho)
    e_step()
    return {'sigma': sg, 'rho': rho, 'loglik': np.array(loglik, np.float64), 'history': history, 'clamped': clamped}


# ------------------------------------------------------------------ the inputs the CPU and GPU tests share
# seq_ref's geometries and one map at the cell limit of jcm_seq_smooth (6144 cells: three float64 planes in LDS)
MAX_HW = 6144
CASES = dict(R.CASES, limit=(1, 2, 64, 96, 1, 3, 1.5, 0.05))


@functools.lru_cache(maxsize=None)
def case(name):
    """(hm, taps, R, sigma, rho, seed, the restatement's result) of CASES[name], computed once and never written to.  The seed is the first from 0
    at which the REFERENCE's gamma has, in every map, a relative top-2 gap above ten times the rounding bound seq_ref.tolerance derives for 2 T
    steps (the forward's and the backward's) -- a condition on the inputs that the reference alone decides, so that a coordinate mismatch cannot
    be blamed on a tie."""
    from joint_cnn_mrf_amd import predict as P
    S, T, HH, WW, K, Rr, sigma, rho = CASES[name]
    taps = P.seq_taps(sigma, Rr, K)
    for seed in range(100):
        hm = R.random_maps((S, T, HH, WW, K), 1000 + seed)
        ref = seq_smooth(hm, taps, rho)
        if (R.top2_gap(ref['gamma']) > 10.0 * R.tolerance(2 * T, HH * WW, Rr)).all():
            return hm, taps, Rr, sigma, rho, seed, ref
    raise AssertionError('no seed below 100 gives case %r a top-2 gap' % name)


# ------------------------------------------------------------------ the planted clip
PLANTED = dict(S=2, T=12, HH=14, WW=19, sigma=(0.9, 1.8), radius=6, rho=0.05, iters=5, start=3.0)


def planted_maps(seed):
    """Maps of random walks of known sigma: per (s, k) a position that takes rounded Gaussian steps of PLANTED['sigma'][k] cells per axis (held
    inside the map), seen as a blob of unit height at it plus a distractor blob of height 0.6 at a fresh random cell in every frame, over a small
    noise floor."""
    c = PLANTED
    rs = np.random.RandomState(4000 + seed)
    S, T, HH, WW, K = c['S'], c['T'], c['HH'], c['WW'], len(c['sigma'])
    ys, xs = np.mgrid[0:HH, 0:WW]
    hm = (rs.rand(S, T, HH, WW, K) * 0.01).astype(np.float32)

    def blob(y, x):
        return np.exp(-((ys - y) ** 2 + (xs - x) ** 2) / 2.0)

    for s in range(S):
        for k in range(K):
            y, x = rs.randint(3, HH - 3), rs.randint(3, WW - 3)
            for t in range(T):
                if t:
                    y = int(np.clip(y + np.rint(rs.randn() * c['sigma'][k]), 0, HH - 1))
                    x = int(np.clip(x + np.rint(rs.randn() * c['sigma'][k]), 0, WW - 1))
                hm[s, t, :, :, k] += (blob(y, x) + 0.6 * blob(rs.randint(HH), rs.randint(WW))).astype(np.float32)
    return hm


def loglik_rounding(hm, radius):
    """What the log-likelihood of a clip can move by through rounding alone: every log norm by the relative error seq_ref.tolerance derives for its
    frame, all S * T * K of them one way."""
    S, T, HH, WW, K = hm.shape
    return S * K * sum(R.tolerance(t, HH * WW, radius) for t in range(T))


def planted_holds(fit, hm):
    c = PLANTED
    planted = np.array(c['sigma'])
    nearer = np.abs(fit['sigma'] - planted) < np.abs(c['start'] * planted - planted)
    rises = np.diff(fit['loglik']) >= -loglik_rounding(hm, c['radius'])
    return bool(nearer.all() and rises.all())


@functools.lru_cache(maxsize=None)
def planted_case():
    """(hm, the restatement's fit, seed): the first seed from 0 at which the REFERENCE's fit -- PLANTED['iters'] EM iterations from three times the
    planted sigma -- ends with every joint's sigma nearer the planted value than the start was and a log-likelihood that never fell by more than
    its rounding.  The condition is on the reference alone."""
    from joint_cnn_mrf_amd import predict as P
    c = PLANTED
    for seed in range(10):
        hm = planted_maps(seed)
        fit = seq_fit(hm, c['start'] * np.array(c['sigma']), c['rho'], c['iters'], c['radius'], P)
        if planted_holds(fit, hm):
            return hm, fit, seed
    raise AssertionError('no seed below 10 gives the planted clip a recovering fit')
