"""The clip decode without a GPU: the numpy restatement tests/seq_pose_ref.py against a dense Viterbi on the explicit 512 x 512
transition, against an enumeration of all paths, and against answers computed by hand; motion.seq_pose_tau against entries computed by hand; the
rules of --seq_pose."""
import itertools

import numpy as np
import pytest
from numpy.testing import assert_array_equal

import pose_ref
import seq_pose_ref as R
import joint_cnn_mrf_amd  # noqa: F401
from joint_cnn_mrf_amd import main as M
from joint_cnn_mrf_amd import motion

K = 9


def _bits(a):
    return np.asarray(a, np.float64).view(np.int64)


def _digits(P):
    """[P^9, 9]: the digits of every flat state, p_0 most significant."""
    return np.array(list(itertools.product(range(P), repeat=K)), np.int64)


def _dense(V, M_, count, tau):
    """Viterbi on the explicit transition of one clip, P^9 states: every entry summed in the order of the passes, ((G + tau_0) + tau_1) .. + tau_8.
    -> (normalised planes, maxes, breaks, paths as flat states or -1)."""
    T, _, P = V.shape
    dg = _digits(P)
    cn = np.clip(count, 0, P)
    planes, maxes, breaks, starts, amax, back = [], np.zeros(T), np.zeros(T, int), np.zeros(T, int), np.full(T, -1), [None] * T
    D, fresh = None, True
    for t in range(T):
        if (cn[t] == 0).any():
            breaks[t], starts[t], fresh, D = 2, 2, True, None
            planes.append(None)
            continue
        valid = (dg < cn[t]).all(axis=1)
        E = R.all_E(V[t], M_[t], cn[t]).reshape(-1).astype(np.float64)
        new = E
        starts[t] = 1
        if not fresh:
            acc = np.repeat(D[:, None], len(dg), axis=1)      # [from, to]
            for j in range(K):
                tj = np.where(np.isnan(tau[t, j]), -np.inf, tau[t, j])      # slots beyond the counts: masked below either way
                acc = acc + tj[dg[:, j][:, None], dg[:, j][None, :]]
            acc[:, ~valid] = -np.inf
            G = acc.max(axis=0)
            new = E + G
            if new.max() == -np.inf:
                new, breaks[t] = E, 1
            else:
                starts[t], back[t] = 0, acc
        m = new.max()
        maxes[t], amax[t] = m, int(np.argmax(new))
        D = np.where(valid, new - m, -np.inf)
        planes.append(D)
        fresh = False
    path, state = np.full(T, -1), -1
    for t in range(T - 1, -1, -1):
        if starts[t] == 2:
            continue
        if t == T - 1 or starts[t + 1] != 0:
            state = amax[t]
        path[t] = state
        if starts[t] == 0:
            state = int(np.argmax(back[t][:, state]))
    return planes, maxes, breaks, path


def _flat(index, P):
    return np.where(index[:, 0] < 0, -1, (index * P ** np.arange(K - 1, -1, -1)).sum(axis=1))


@pytest.mark.parametrize('seed', [1, 2])
def test_against_dense_viterbi(seed):
    """P = 2, 512 states, T = 6, mixed counts: D and maxes bit for bit (rounding is monotone, so nested maxima equal the maximum of the composed
    sum), and the path on tie-free random data."""
    V, M_, count, cells, tau = R.random_case(1, 6, 2, seed, counts='some' if seed == 1 else 'mixed')
    got = R.decode_clip(V[0], M_[0], count[0], cells[0], tau[0], keep_planes=True)
    planes, maxes, breaks, path = _dense(V[0], M_[0], count[0], tau[0])
    assert_array_equal(_bits(got['maxes']), _bits(maxes))
    assert_array_equal(got['breaks'], breaks)
    for t in range(6):
        if planes[t] is None:
            assert got['D'][t] is None
        else:
            assert_array_equal(_bits(got['D'][t].reshape(-1)), _bits(planes[t]))
    assert_array_equal(_flat(got['index'], 2), path)
    if seed == 2:
        assert (breaks == 2).any()


def test_against_all_paths():
    """P = 2, T = 2: the best of all 512^2 paths by E_0 + sum of tau + E_1, in float64 on a grid of dyadic values so that every order of summation
    is exact; the test asserts that its data are tie-free."""
    rs = np.random.RandomState(5)
    P, T = 2, 2
    V = (rs.randint(-512, 512, (T, K, P)) / 64.0).astype(np.float32)
    M_ = (rs.randint(-512, 512, (T, 36, P, P)) / 64.0).astype(np.float32)
    tau = rs.randint(-4096, 4096, (T, K, P, P)) / 1024.0
    count = np.full((T, K), P, np.int32)
    cells = np.zeros((T, K, P, 2), np.int32)
    got = R.decode_clip(V, M_, count, cells, tau)
    dg = _digits(P)
    E = [R.all_E(V[t], M_[t], count[t]).reshape(-1).astype(np.float64) for t in range(T)]
    trans = sum(tau[1, j][dg[:, j][:, None], dg[:, j][None, :]] for j in range(K))
    total = E[0][:, None] + trans + E[1][None, :]
    best = np.unravel_index(int(np.argmax(total)), total.shape)
    assert (total == total.max()).sum() == 1
    assert_array_equal(_flat(got['index'], P), best)
    assert got['maxes'][0] == E[0].max() and got['maxes'][1] == total.max() - E[0].max()


def test_one_candidate():
    """P = 1: one state; index 0, maxes = E_0, then E_t + tau summed over the joints in pass order."""
    T = 3
    V = np.arange(T * K, dtype=np.float32).reshape(T, K, 1) / 4
    M_ = np.ones((T, 36, 1, 1), np.float32) / 2
    tau = -np.arange(T * K, dtype=np.float64).reshape(T, K, 1, 1) / 8
    cells = np.arange(T * K * 2, dtype=np.int32).reshape(T, K, 1, 2)
    got = R.decode_clip(V, M_, np.ones((T, K), np.int32), cells, tau)
    assert (got['index'] == 0).all() and (got['breaks'] == 0).all()
    E = V.sum(axis=(1, 2)) + 18.0
    assert_array_equal(got['frame_score'], E.astype(np.float32))
    assert_array_equal(got['maxes'], [E[0], E[1] + tau[1].sum(), E[2] + tau[2].sum()])
    assert_array_equal(got['coords'], cells[:, :, 0].transpose(0, 2, 1))


def _flip_flop(T=5):
    """Two poses, all-0 and all-1 (P = 2; M couples every pair so that a mixed pose loses by far): the per-frame arg-max of E alternates between
    them by a margin of 1, and a tau of -1 per joint for changing candidate makes a flip cost 9."""
    V = np.zeros((T, K, 2), np.float32)
    M_ = np.zeros((T, 36, 2, 2), np.float32)
    M_[:, :, 0, 1] = M_[:, :, 1, 0] = -8.0
    V[0::2, 0, 0] = 1.0      # even frames prefer pose 0
    V[1::2, 0, 1] = 1.0      # odd frames pose 1
    V[0, 0, 0] = 2.0         # and frame 0 by more, so that holding pose 0 beats holding pose 1 (T odd helps too)
    tau = np.zeros((T, K, 2, 2))
    tau[:, :, 0, 1] = tau[:, :, 1, 0] = -1.0
    cells = np.zeros((T, K, 2, 2), np.int32)
    return V, M_, np.full((T, K), 2, np.int32), cells, tau


def test_planted_flip_flop():
    V, M_, count, cells, tau = _flip_flop()
    per_frame = np.stack([pose_ref.search_one(V[t], M_[t], count[t])[0] for t in range(5)])
    assert_array_equal(per_frame[:, 0], [0, 1, 0, 1, 0])
    assert (per_frame == per_frame[:, :1]).all()
    held = R.decode_clip(V, M_, count, cells, tau)
    assert (held['index'] == 0).all()
    # by hand: D_0 = (0, -2) after m_0 = 2; frame 1: pose 0 gets 0 + 0, pose 1 gets 1 + max(0 - 9, -2) = -1, m_1 = 0; frame 2: 1 and 0 + max(-9, -1), m_2 = 1; ..
    assert_array_equal(held['maxes'], [2.0, 0.0, 1.0, 0.0, 1.0])
    assert_array_equal(held['frame_score'], [2.0, 0.0, 1.0, 0.0, 1.0])
    off = R.decode_clip(V, M_, count, cells, 0.0 * tau)
    assert_array_equal(off['index'], per_frame)


def test_break_1():
    """One transition all -inf (what rho = 0 makes of candidates further apart than the radius): the chain is cut there, both segments end at their own
    arg-max, the flag is 1 and maxes restarts at max E."""
    V, M_, count, cells, tau = R.random_case(1, 5, 2, 11, counts='full', neg_inf=0.0)
    tau[0, 3] = -np.inf
    got = R.decode_clip(V[0], M_[0], count[0], cells[0], tau[0])
    assert_array_equal(got['breaks'], [0, 0, 0, 1, 0])
    head = R.decode_clip(V[0, :3], M_[0, :3], count[0, :3], cells[0, :3], tau[0, :3])
    tail = R.decode_clip(V[0, 3:], M_[0, 3:], count[0, 3:], cells[0, 3:], tau[0, 3:])
    for k in ('index', 'coords', 'frame_score', 'maxes'):
        assert_array_equal(got[k], np.concatenate([head[k], tail[k]]), err_msg=k)
    cl = np.zeros((2, K, 2, 2), np.int64)
    cl[1, :, :, 1] = 40      # every candidate of frame 1 is 40 cells from every candidate of frame 0
    assert (motion.seq_pose_tau(cl, np.full((2, K), 2), 1.5, 0.0)[1] == -np.inf).all()


def test_break_2():
    """A count of 0 in a middle frame and in frame 0: no pose there (-1, -inf, maxes 0, flag 2), the chain restarts behind it without a flag."""
    V, M_, count, cells, tau = R.random_case(1, 6, 2, 12, counts='full', neg_inf=0.0)
    count[0, 0, 5] = 0
    count[0, 3, 0] = 0
    got = R.decode_clip(V[0], M_[0], count[0], cells[0], tau[0])
    assert_array_equal(got['breaks'], [2, 0, 0, 2, 0, 0])
    for t in (0, 3):
        assert (got['index'][t] == -1).all() and (got['coords'][t] == -1).all() and got['frame_score'][t] == -np.inf and got['maxes'][t] == 0.0
    for lo, hi in ((1, 3), (4, 6)):
        part = R.decode_clip(V[0, lo:hi], M_[0, lo:hi], count[0, lo:hi], cells[0, lo:hi], tau[0, lo:hi])
        for k in ('index', 'coords', 'frame_score', 'maxes', 'breaks'):
            assert_array_equal(got[k][lo:hi], part[k], err_msg=k)


def test_seq_pose_tau_by_hand():
    """sigma 1, radius 1: taps (e, 1, e) / (1 + 2e), e = exp(-1/2); rho 0.1 over 5400 cells; weight 2."""
    e = np.exp(-0.5)
    w = np.array([e, 1.0, e]) / (1.0 + 2.0 * e)
    assert_array_equal(motion.seq_kernel(1.0, 1, K)[1][4], w)
    cells = np.zeros((3, K, 2, 2), np.int64)
    cells[1, :, 0] = (1, -1)      # from (0,0): dy = 1, dx = -1
    cells[1, :, 1] = (0, 2)       # dx = 2: outside the radius
    cells[2, :, 0] = (1, 0)       # from (1,-1): (0, 1); from (0,2): (1,-2) outside
    cells[2, :, 1] = (7, 7)
    count = np.full((3, K), 2)
    count[2, 4] = 1
    tau = motion.seq_pose_tau(cells, count, 1.0, 0.1, radius=1, weight=2.0)
    assert tau.shape == (3, K, 2, 2) and tau.dtype == np.float64 and (tau[0] == 0).all()
    om, u = 0.9, 0.1 / 5400.0
    assert tau[1, 0, 0, 0] == 2.0 * np.log(om * w[2] * w[0] + u)
    assert tau[1, 0, 1, 1] == 2.0 * np.log(u) == tau[1, 3, 0, 1]
    assert tau[2, 0, 0, 0] == 2.0 * np.log(om * w[1] * w[2] + u)
    assert tau[2, 0, 1, 0] == 2.0 * np.log(u)
    assert (tau[2, 4, :, 1] == 0).all() and tau[2, 4, 0, 0] == tau[2, 0, 0, 0]      # a slot at or beyond count
    assert motion.seq_pose_tau(cells, count, 1.0, 0.0, radius=1)[1, 0, 1, 1] == -np.inf
    assert (motion.seq_pose_tau(cells, count, 1.0, 0.0, radius=1, weight=0.0) == 0).all()
    other = motion.seq_pose_tau(cells, count, 1.0, 0.1, radius=1, hw=100)
    assert other[1, 0, 1, 1] == np.log(0.1 / 100.0)
    for bad in (dict(rho=1.5), dict(weight=-1.0), dict(weight=np.inf)):
        with pytest.raises(ValueError):
            motion.seq_pose_tau(cells, count, 1.0, **dict(dict(rho=0.1), **bad))


def _refusal(argv):
    hps = M.hps
    try:
        with pytest.raises(SystemExit) as ei:
            M.main(argv)
    finally:
        M.hps = hps
    return ei.value.code


def test_flag_rules():
    head, pose = ['--gpus', '0'], ['--seq_pose', '2']
    ok = head + ['--predict', 'nowhere', '--predictions', 'nowhere.json', '--use_sm', '--sequence', 'viterbi'] + pose
    cases = [(head + ['--use_sm'] + pose, M.SEQ_POSE_NEEDS_PREDICT),
             (head + ['--predict', 'nowhere', '--predictions', 'nowhere.json', '--sequence', 'viterbi'] + pose, M.SEQ_POSE_NEEDS_USE_SM),
             (head + ['--predict', 'nowhere', '--predictions', 'nowhere.json', '--use_sm'] + pose, M.SEQ_POSE_NEEDS_VITERBI),
             (head + ['--predict', 'nowhere', '--predictions', 'nowhere.json', '--use_sm', '--sequence', 'filter'] + pose, M.SEQ_POSE_NEEDS_VITERBI),
             (ok[:-1] + ['0'], '--seq_pose 0: 1 <= P <= 4'),
             (ok[:-1] + ['5'], '--seq_pose 5: 1 <= P <= 4'),
             (ok + ['--seq_pose_weight', '-1'], '--seq_pose_weight -1.0: W is finite and >= 0'),
             (ok + ['--seq_pose_weight', 'inf'], '--seq_pose_weight inf: W is finite and >= 0'),
             (ok + ['--seq_pose_weight', 'nan'], '--seq_pose_weight nan: W is finite and >= 0'),
             (ok[:-2] + ['--seq_pose_weight', '0.5'], M.SEQ_POSE_WEIGHT_NEEDS_SEQ_POSE),
             (ok + ['--seq_people', '2'], M.SEQ_POSE_NO_PEOPLE),
             (ok + ['--seq_zoom'], M.SEQ_POSE_NO_ZOOM),
             (ok + ['--seq_camera'], M.SEQ_POSE_NO_CAMERA),
             (ok + ['--seq_flow', '2'], M.SEQ_POSE_NO_FLOW),
             (ok + ['--seq_flow_centre'], M.SEQ_POSE_NO_FLOW_CENTRE),
             (ok + ['--seq_fit', '3'], M.SEQ_POSE_NO_FIT)]
    for argv, text in cases:
        assert _refusal(argv) == text, argv


def test_lists_without_the_new_flags_are_refused_as_before():
    """The new table is walked last and every rule of it asks for one of the new flags: without them the refusal is what the other tables give."""
    base = ['--gpus', '0', '--predict', 'nowhere', '--predictions', 'nowhere.json']
    cases = [(base + ['--sequence', 'viterbi', '--seq_flow_centre', '--seq_camera'], M.SEQ_FLOW_CENTRE_NO_CAMERA),
             (base + ['--sequence', 'lag', '--seq_lag', '2', '--seq_flow', '2'], M.SEQ_FLOW_NO_LAG),
             (base + ['--seq_flow_search', '3', '--sequence', 'filter'], M.SEQ_FLOW_SEARCH_NEEDS_SEQ_FLOW),
             (base + ['--seq_flow_centre'], M.SEQ_FLOW_CENTRE_NEEDS_SEQUENCE)]
    for argv, text in cases:
        assert _refusal(argv) == text, argv
        assert _refusal(argv + ['--seq_pose', '2', '--use_sm']) == text, argv      # and an earlier table still speaks first
    blank = M.build_parser().parse_args(base)
    assert blank.seq_pose is None and blank.seq_pose_weight is None
    assert not any(holds(blank) for holds, _ in M.SEQ_POSE_RULES)
