"""Clip pose decoding restated in numpy (include/jcm.h: jcm_seq_pose_viterbi): the nine axis passes in the stated order with the
stated tie rules, float64, one rounded operation per step; E_t is the fixed-order float32 sum of tests/pose_ref.py.  Shares nothing with the kernel.

tests/test_seq_pose_cpu.py pins it against a dense Viterbi on the explicit transition, an enumeration of all paths and answers computed by hand;
tests/test_gpu_seq_pose.py holds the kernel to it bit for bit."""
import numpy as np

import pose_ref

K = 9
NEG = -np.inf


def valid_mask(cn, P):
    v = np.ones((), bool)
    for j in range(K):
        v = v & pose_ref._on((j,), np.arange(P) < cn[j], K)
    return np.broadcast_to(v, (P,) * K)


def all_E(V, M, cn):
    """V [9,P], M [36,P,P] fp32 of one frame, cn [9] clamped counts -> E fp32 [P]*9, -inf where the pose is not valid.  Slots at or beyond the counts
    may hold anything: what the sum makes of them is masked."""
    P = V.shape[1]
    with np.errstate(invalid='ignore'):
        S = pose_ref.all_scores(np.asarray(V, np.float32), np.asarray(M, np.float32))
    return np.where(valid_mask(cn, P), S, np.float32(NEG)).astype(np.float32)


def axis_pass(G, tau_j, j, na, nb):
    """One pass along axis j: G'(.., b, ..) = max over a < na, ascending, of G(.., a, ..) + tau_j[a,b]; a strictly greater value replaces; b >= nb: -inf.
    -> (G', the winners int8)."""
    Gj = np.moveaxis(G, j, -1)
    out = np.full(Gj.shape, NEG)
    ptr = np.zeros(Gj.shape, np.int8)
    for b in range(nb):
        best = np.full(Gj.shape[:-1], NEG)
        arg = np.zeros(Gj.shape[:-1], np.int8)
        for a in range(na):
            v = Gj[..., a] + tau_j[a, b]
            rep = v > best
            best = np.where(rep, v, best)
            arg = np.where(rep, np.int8(a), arg)
        out[..., b] = best
        ptr[..., b] = arg
    return np.moveaxis(out, -1, j), np.moveaxis(ptr, -1, j)


def decode_clip(V, M, count, cells, tau, keep_planes=False):
    """One clip: V [T,9,P] fp32, M [T,36,P,P] fp32, count [T,9], cells [T,9,P,2], tau [T,9,P,P] float64 -> {'index' int32 [T,9], 'coords' int32
    [T,2,9], 'frame_score' fp32 [T], 'maxes' float64 [T], 'breaks' int32 [T]} and with keep_planes 'D', the normalised planes (None without a pose)."""
    T, _, P = V.shape
    shape = (P,) * K
    cn = np.clip(np.asarray(count, np.int64), 0, P)
    maxes, breaks = np.zeros(T), np.zeros(T, np.int32)
    start = np.zeros(T, np.int32)      # 1: no pointers into the frame before; 2: no pose
    amax = np.full(T, -1, np.int64)
    ptrs, planes, Es = [None] * T, [None] * T, [None] * T
    D, fresh = None, True
    for t in range(T):
        if (cn[t] == 0).any():
            breaks[t], start[t], fresh, D = 2, 2, True, None
            continue
        E32 = all_E(V[t], M[t], cn[t])
        Es[t] = E32
        E = E32.astype(np.float64)
        new = E
        if fresh:
            start[t] = 1
        else:
            G, pt = D, []
            for j in range(K):
                G, p = axis_pass(G, tau[t, j], j, int(cn[t - 1, j]), int(cn[t, j]))
                pt.append(p)
            with np.errstate(invalid='ignore'):
                new = E + G
            if new.max() == NEG:      # break 1
                new, breaks[t], start[t] = E, 1, 1
            else:
                ptrs[t] = pt
        m = new.max()
        maxes[t] = m
        amax[t] = int(np.argmax(new.reshape(-1)))
        D = np.where(valid_mask(cn[t], P), new - m, NEG)
        planes[t] = D
        fresh = False
    index = np.full((T, K), -1, np.int32)
    state = None
    for t in range(T - 1, -1, -1):
        if start[t] == 2:
            state = None
            continue
        if t == T - 1 or start[t + 1] != 0:
            state = list(np.unravel_index(amax[t], shape))
        index[t] = state
        if start[t] == 0:
            state = list(state)
            for j in range(K - 1, -1, -1):
                state[j] = int(ptrs[t][j][tuple(state)])
    coords = np.full((T, 2, K), -1, np.int32)
    score = np.full(T, NEG, np.float32)
    for t in range(T):
        if index[t, 0] >= 0:
            coords[t] = np.asarray(cells)[t, np.arange(K), index[t]].T
            score[t] = Es[t][tuple(index[t])]
    out = {'index': index, 'coords': coords, 'frame_score': score, 'maxes': maxes, 'breaks': breaks}
    if keep_planes:
        out['D'] = planes
    return out


def decode(V, M, count, cells, tau):
    """[S,T,...] inputs -> the outputs of jcm_seq_pose_viterbi, stacked over the clips."""
    r = [decode_clip(V[s], M[s], count[s], cells[s], tau[s]) for s in range(V.shape[0])]
    return {k: np.stack([x[k] for x in r]) for k in r[0]}


# ------------------------------------------------------------------ inputs shared by the CPU and the GPU tests
def random_case(S, T, P, seed, integers=False, counts='mixed', neg_inf=0.15, nan_fill=True):
    """Tables of random floats, or of a few small integers so that exact ties occur in every pass; counts mixed in 0..P with both kinds of break
    ('mixed', from T = 3 and T = 4 on), in 1..P ('some') or all P ('full'); a fraction of tau is -inf; slots at or beyond count hold NaN in V, M and tau."""
    rs = np.random.RandomState(seed)
    draw = (lambda *s: rs.randint(-2, 3, s).astype(np.float64)) if integers else (lambda *s: rs.standard_normal(s) * 2.0)
    V = draw(S, T, K, P).astype(np.float32)
    M = draw(S, T, 36, P, P).astype(np.float32)
    tau = draw(S, T, K, P, P)
    tau[rs.random_sample(tau.shape) < neg_inf] = NEG
    if counts == 'full':
        count = np.full((S, T, K), P, np.int32)
    else:
        count = rs.randint(1, P + 1, (S, T, K)).astype(np.int32)
        count[rs.random_sample(count.shape) < 0.5] = P
    if counts == 'mixed' and T >= 3:
        for s in range(S):      # break 2: the last frame of the even clips, frame 0 of the odd ones (what follows it starts afresh)
            count[s, T - 1 if s % 2 == 0 else 0, rs.randint(K)] = 0
    if counts == 'mixed' and T >= 4:
        tau[0, 2, 2] = NEG      # break 1: joint 2 has no transition into frame 2 of clip 0
    cells = np.stack([rs.randint(0, 60, (S, T, K, P)), rs.randint(0, 90, (S, T, K, P))], axis=-1).astype(np.int32)
    if nan_fill:
        dead = np.arange(P)[None, None, None, :] >= np.clip(count, 0, P)[..., None]      # [S,T,K,P]
        V[dead] = np.nan
        for r, (a, b) in enumerate(pose_ref.pairs()):
            M[:, :, r][dead[:, :, a][..., :, None] | dead[:, :, b][..., None, :]] = np.nan
        prev = np.concatenate([np.ones_like(dead[:, :1]), dead[:, :-1]], axis=1)
        tau[prev[..., :, None] | dead[..., None, :]] = np.nan
    return V, M, count, cells, tau
