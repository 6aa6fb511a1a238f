"""The restatement of the sequence stages (tests/seq_ref.py) against exhaustive enumeration and hand-made cases, the condition on
the random inputs the GPU tests share, the tap builder, and the refusals of --sequence on the command line.  No device is needed."""
import argparse
import itertools
import json
import os

import numpy as np
import pytest
from numpy.testing import assert_array_equal

import seq_ref as R
import joint_cnn_mrf_amd  # noqa: F401
from joint_cnn_mrf_amd import main as M
from joint_cnn_mrf_amd import predict as P

HERE = os.path.dirname(os.path.abspath(__file__))
W3 = np.array([[0.25, 0.5, 0.25]])      # one joint, R = 1


def _maps(frames):
    """A list of [HH,WW] arrays -> hm [1,T,HH,WW,1]."""
    return np.stack([np.asarray(f, np.float32) for f in frames])[None, :, :, :, None]


def _delta(HH, WW, y, x, v=1.0):
    a = np.zeros((HH, WW), np.float32)
    a[y, x] = v
    return a


# ------------------------------------------------------------------ the tap builder
def test_seq_taps():
    w = P.seq_taps((0.8, 1.5), 3, 2)
    assert w.shape == (2, 7) and w.dtype == np.float64
    d = np.arange(-3, 4, dtype=np.float64)
    for k, s in enumerate((0.8, 1.5)):
        e = np.exp(-(d * d) / (2.0 * s * s))
        assert_array_equal(w[k], e / e.sum())
    assert_array_equal(P.seq_taps(2.0, 0, 3), np.ones((3, 1)))
    assert_array_equal(P.seq_taps(1.5, 2, 4)[0], P.seq_taps(1.5, 2, 4)[3])
    assert P.seq_radius(1.5) == 5 and P.seq_radius((0.5, 2.1)) == 7 and P.seq_radius(40.0) == 16
    for bad in (0.0, -1.0, float('nan'), (1.0, 2.0)):
        with pytest.raises(ValueError):
            P.seq_taps(bad, 2, 3)
    with pytest.raises(ValueError):
        P.seq_taps(1.0, -1, 3)


# ------------------------------------------------------------------ against enumeration
def _enumeration_world():
    rs = np.random.RandomState(5)
    HH, WW, T, rho = 2, 3, 3, 0.1
    hm = (rs.rand(1, T, HH, WW, 1) + 0.05).astype(np.float32)
    taps = P.seq_taps(0.9, 1, 1)
    cells = [(y, x) for y in range(HH) for x in range(WW)]
    om, u = 1.0 - rho, rho / (HH * WW)

    def kern(a, b):      # the separable truncated kernel between two cells, 0 beyond the radius
        dy, dx = b[0] - a[0], b[1] - a[1]
        return taps[0, dy + 1] * taps[0, dx + 1] if abs(dy) <= 1 and abs(dx) <= 1 else 0.0
    return hm, taps, rho, cells, om, u, kern, T


def test_viterbi_is_the_best_of_all_enumerated_paths():
    hm, taps, rho, cells, om, u, kern, T = _enumeration_world()
    best, best_path = -1.0, None
    for path in itertools.product(range(len(cells)), repeat=T):      # 6^3 paths; a step is the better of the move and the jump
        score = float(hm[0, 0][cells[path[0]]][0])
        for t in range(1, T):
            score *= max(om * kern(cells[path[t - 1]], cells[path[t]]), u) * float(hm[0, t][cells[path[t]]][0])
        if score > best:
            best, best_path = score, path
    got = R.seq_viterbi(hm, taps, rho)
    assert_array_equal(got['path'][0, :, :, 0], np.array([cells[i] for i in best_path]))
    assert_array_equal(got['breaks'], 0)
    assert abs(np.prod(got['maxes']) * 1.0 - best) <= 1e-13 * best      # the maxima multiply up to the best path's score


def test_filter_is_the_enumerated_forward_marginal():
    hm, taps, rho, cells, om, u, kern, T = _enumeration_world()
    n = len(cells)
    got = R.seq_filter(hm, taps, rho)
    for t in range(T):
        marg = np.zeros(n)
        for path in itertools.product(range(n), repeat=t + 1):
            pr = float(hm[0, 0][cells[path[0]]][0])
            for q in range(1, t + 1):
                pr *= (om * kern(cells[path[q - 1]], cells[path[q]]) + u) * float(hm[0, q][cells[path[q]]][0])
            marg[path[-1]] += pr
        marg /= marg.sum()
        assert np.abs(got['belief'][0, t, :, :, 0].reshape(-1) - marg).max() <= 1e-13
    for order in (True, False):      # the order of Z moves nothing beyond rounding
        assert np.abs(R.seq_filter(hm, taps, rho, kernel_order=order)['belief'] - got['belief']).max() <= 1e-15


def test_rho0_uniform_observations_blur_a_delta():
    HH, WW, T, Rr = 9, 11, 3, 2
    taps = P.seq_taps(1.2, Rr, 1)
    state = np.zeros((1, 1, HH, WW))
    state[0, 0, 2, 9] = 1.0      # near the right edge: mass leaves the map and the renormalisation shows
    got = R.seq_filter(np.ones((1, T, HH, WW, 1), np.float32), taps, 0.0, state=state)
    a = state[0, 0]
    for t in range(T):
        a = np.apply_along_axis(lambda v: np.convolve(v, taps[0], mode='same'), 0, a)
        a = np.apply_along_axis(lambda v: np.convolve(v, taps[0], mode='same'), 1, a)
        assert np.abs(got['belief'][0, t, :, :, 0] - a / a.sum()).max() <= 1e-15
        assert got['reset'][0, t, 0] == 0
    assert a.sum() < 0.99


def test_kernel_sum_is_a_sum():
    rs = np.random.RandomState(2)
    for n in (1, 35, 1024, 5400, 8192):
        v = rs.rand(n)
        assert abs(R.kernel_sum(v) - v.sum()) <= n * 2.0 ** -53 * v.sum()
    assert R.kernel_sum(np.zeros(35)) == 0.0


# ------------------------------------------------------------------ hand-made cases, the expected cells written out
def test_tie_goes_to_the_lowest_offset():
    # d_0 has equal maxima at x = 0 and x = 2; the delta of frame 1 at x = 1 reaches both with one product.  dx ascends from -1, and
    # dx = -1 reads the cell x - dx = 2: the lowest dx wins the tie, so the track comes from x = 2.
    got = R.seq_viterbi(_maps([[[1, 0, 1, 0, 0]], [[0, 1, 0, 0, 0]]]), W3, 0.0)
    assert_array_equal(got['path'][0, :, :, 0], [[0, 2], [0, 1]])
    # the same along y: dy = -1 reads the row y + 1
    got = R.seq_viterbi(_maps([[[1], [0], [1], [0], [0]], [[0], [1], [0], [0], [0]]]), W3, 0.0)
    assert_array_equal(got['path'][0, :, :, 0], [[2, 0], [1, 0]])
    assert_array_equal(got['breaks'], 0)


def test_equal_maxima_resolve_to_the_lower_index():
    hm = _maps([[[0, 3, 0], [3, 0, 3]]])
    assert_array_equal(R.seq_filter(hm, W3, 0.05)['coords'][0, 0, :, 0], [0, 1])
    assert_array_equal(R.seq_viterbi(hm, W3, 0.05)['path'][0, 0, :, 0], [0, 1])


def test_far_delta_is_a_jump_with_rho_and_a_break_without():
    hm = _maps([_delta(1, 9, 0, 0), _delta(1, 9, 0, 8)])
    u = 0.5 / 9
    v = R.seq_viterbi(hm, W3, 0.5)      # the move cannot reach x = 8: the jump wins, its source is the arg-max of d_0
    assert_array_equal(v['path'][0, :, :, 0], [[0, 0], [0, 8]])
    assert_array_equal(v['breaks'][0, :, 0], [0, 0])
    assert_array_equal(v['maxes'][0, :, 0], [1.0, u])
    f = R.seq_filter(hm, W3, 0.5)
    assert_array_equal(f['coords'][0, :, :, 0], [[0, 0], [0, 8]])
    assert_array_equal(f['reset'][0, :, 0], [0, 0])
    assert_array_equal(f['norm'][0, :, 0], [1.0, u])
    v = R.seq_viterbi(hm, W3, 0.0)      # no jump: M == 0, a break; the earlier segment ends at the arg-max of d_0
    assert_array_equal(v['path'][0, :, :, 0], [[0, 0], [0, 8]])
    assert_array_equal(v['breaks'][0, :, 0], [0, 1])
    assert_array_equal(v['maxes'][0, :, 0], [1.0, 1.0])
    f = R.seq_filter(hm, W3, 0.0)
    assert_array_equal(f['coords'][0, :, :, 0], [[0, 0], [0, 8]])
    assert_array_equal(f['reset'][0, :, 0], [0, 1])
    assert_array_equal(f['norm'][0, :, 0], [1.0, 1.0])


def test_break_cuts_the_track():
    # frame 1 is out of reach of frame 0 (a break with rho = 0); frame 0 has its maximum at x = 6 and a lower bump at x = 8.
    # The earlier segment ends at ITS arg-max, x = 6, whatever the later frames hold.
    f0 = np.zeros((1, 9), np.float32)
    f0[0, 6], f0[0, 8] = 2.0, 1.0
    got = R.seq_viterbi(_maps([f0, _delta(1, 9, 0, 0), _delta(1, 9, 0, 1)]), W3, 0.0)
    assert_array_equal(got['breaks'][0, :, 0], [0, 1, 0])
    assert_array_equal(got['path'][0, :, :, 0], [[0, 6], [0, 0], [0, 1]])


def test_zero_frame_mid_sequence():
    hm = _maps([_delta(1, 9, 0, 2), np.zeros((1, 9)), _delta(1, 9, 0, 5)])
    f = R.seq_filter(hm, W3, 0.05)
    assert_array_equal(f['reset'][0, :, 0], [0, 2, 0])
    assert_array_equal(f['belief'][0, 1, 0, :, 0], np.full(9, 1.0 / 9.0))
    assert_array_equal(f['coords'][0, :, :, 0], [[0, 2], [0, 0], [0, 5]])
    assert f['norm'][0, 1, 0] == 0.0
    v = R.seq_viterbi(hm, W3, 0.05)
    assert_array_equal(v['breaks'][0, :, 0], [0, 2, 0])
    assert v['maxes'][0, 1, 0] == 0.0
    # d_1 = 1 everywhere: the delta of frame 2 is reached best by staying (w[1] = 0.5 beats 0.25), from x = 5; frame 0 ends at its own arg-max
    assert_array_equal(v['path'][0, :, :, 0], [[0, 2], [0, 5], [0, 5]])
    # an all-zero frame 0: reset / breaks 2 there too
    hm0 = _maps([np.zeros((1, 9)), _delta(1, 9, 0, 5)])
    assert_array_equal(R.seq_filter(hm0, W3, 0.05)['reset'][0, :, 0], [2, 0])
    assert_array_equal(R.seq_viterbi(hm0, W3, 0.05)['breaks'][0, :, 0], [2, 0])


def test_state_carries_a_split():
    hm, taps, _, _, rho, _ = R.case_inputs('split', P.seq_taps)
    whole = R.seq_filter(hm, taps, rho)
    first = R.seq_filter(hm[:, :3], taps, rho)
    second = R.seq_filter(hm[:, 3:], taps, rho, state=first['state'])
    assert_array_equal(np.concatenate([first['belief'], second['belief']], axis=1), whole['belief'])
    assert_array_equal(second['state'], whole['state'])


# ------------------------------------------------------------------ the inputs the GPU tests use
@pytest.mark.parametrize('name', sorted(R.CASES))
def test_gpu_inputs_have_a_top2_gap(name):
    """A condition on the inputs, decided by the reference alone: in every map of every random input the GPU tests use, the filtered belief's
    best cell leads the second best by more than the tolerance those tests allow (ten times it), so a coordinate mismatch is no tie."""
    hm, taps, Rr, _, rho, seed = R.case_inputs(name, P.seq_taps)
    S, T, HH, WW, K = hm.shape
    gap = R.top2_gap(R.seq_filter(hm, taps, rho)['belief'])
    for t in range(T):
        assert (gap[:, t] > 10.0 * R.tolerance(t, HH * WW, Rr)).all(), (name, seed, t, gap[:, t].min())
    assert (hm >= 0).all() and np.isfinite(hm).all()


# ------------------------------------------------------------------ the command line
REFUSALS = (
    (['--sequence', 'filter'], 'SEQUENCE_NEEDS_PREDICT'),
    (['--sequence', 'viterbi', '--predict', 'x', '--predictions', 'o.json', '--use_sm', '--zoom'], 'SEQUENCE_NO_ZOOM'),
    (['--sequence', 'viterbi', '--predict', 'x', '--predictions', 'o.json', '--use_sm', '--people', '2'], 'SEQUENCE_ONE_PERSON'),
    (['--seq_sigma', '2.0', '--predict', 'x', '--predictions', 'o.json'], 'SEQ_OPTION_NEEDS_SEQUENCE'),
    (['--seq_rho', '0.1'], 'SEQ_OPTION_NEEDS_SEQUENCE'),
)


@pytest.mark.parametrize('argv,name', REFUSALS)
def test_cli_refusals(argv, name):
    keep = argparse.Namespace(**vars(M.hps))
    try:
        with pytest.raises(SystemExit) as ei:
            M.main(list(argv) + ['--gpus', '99'])
    finally:
        M.hps = keep
    assert ei.value.code == getattr(M, name)


def test_new_rules_follow_the_recorded_ones():
    """The four new rules are walked behind every rule tests/golden/cli_refusals.json was recorded from (main.SEQUENCE_RULES, after FLAG_RULES,
    which ends where it ended), so none of its cases can change its message."""
    new = [M.SEQUENCE_NEEDS_PREDICT, M.SEQUENCE_NO_ZOOM, M.SEQUENCE_ONE_PERSON, M.SEQ_OPTION_NEEDS_SEQUENCE]
    assert [m for _, m in M.SEQUENCE_RULES] == new
    assert M.FLAG_RULES[-1][1] == M.RENDER_HEAT_SM_NEEDS_USE_SM and not set(new) & {m for _, m in M.FLAG_RULES}
    with open(os.path.join(HERE, 'golden', 'cli_refusals.json')) as fh:
        recorded = json.load(fh)['messages']
    assert not set(new) & set(recorded)
    # an earlier rule still wins over a new one
    keep = argparse.Namespace(**vars(M.hps))
    try:
        with pytest.raises(SystemExit) as ei:
            M.main(['--sequence', 'filter', '--render', 'out', '--gpus', '99'])
    finally:
        M.hps = keep
    assert ei.value.code == M.RENDER_NEEDS_PREDICT


def test_defaults_are_declared_placeholders():
    assert (P.SEQ_SIGMA, P.SEQ_RHO) == (1.5, 0.05)
    text = M.build_parser().format_help()
    assert 'untuned placeholder' in ' '.join(text.split())
    assert 'has not been measured' in ' '.join(P.predict_sequence.__doc__.split())
