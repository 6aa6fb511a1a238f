"""Flow-centred scans without a device: the numpy restatement of the centred recurrences (tests/seq_centred_ref.py) is pinned --
against tests/seq_moving_ref.py on uniform tables, against tests/seq_ref.py on zero tables and, independently of both, against the enumeration
of all paths on a map small enough for it --, then motion.flow_cell_shifts, the refusals of the host layers and of the command line, which are
raised before a device is touched, and the two exported symbols."""
import argparse
import itertools

import numpy as np
import pytest
import torch
from numpy.testing import assert_array_equal

import seq_centred_ref as CR
import seq_moving_ref as MR
import seq_ref as R
import joint_cnn_mrf_amd  # noqa: F401
from joint_cnn_mrf_amd import _lib
from joint_cnn_mrf_amd import main as M
from joint_cnn_mrf_amd import motion
from joint_cnn_mrf_amd import predict as P


def _bits(a):
    return np.asarray(a, np.float64).view(np.int64)


def _same(got, want):
    assert sorted(got) == sorted(want)
    for k in want:
        if want[k].dtype == np.float64:
            assert_array_equal(_bits(got[k]), _bits(want[k]), err_msg=k)
        else:
            assert_array_equal(got[k], want[k], err_msg=k)


# ------------------------------------------------------------------ the restatement
@pytest.mark.parametrize('name', sorted(CR.CASES))
def test_shared_cases_have_a_clear_arg_max(name):
    hm, taps, Rr, sigma, rho, centre, seed = CR.case_inputs(name, P.seq_taps)
    S, T, HH, WW, K = hm.shape
    assert centre.shape == (S, T, HH, WW, 2)
    gap = R.top2_gap(CR.seq_filter(hm, taps, rho, centre)['belief'])
    for t in range(T):
        assert (gap[:, t] > 10.0 * R.tolerance(t, HH * WW, Rr)).all(), (name, t, seed)


def test_cases_cover_what_the_index_arithmetic_can_get_wrong():
    C = CR.CASES
    assert {n: C[n][:6] for n in C} == {'odd': (2, 5, 13, 17, 3, 3), 'vector': (2, 3, 6, 10, 3, 2), 'clipped': (1, 3, 5, 7, 2, 8), 'far': (1, 3, 5, 7, 1, 2),
                                        'lost': (1, 3, 13, 17, 3, 3), 'radius0': (1, 3, 5, 7, 2, 0), 'big': (1, 2, 64, 128, 1, 2), 'real': (1, 4, 60, 90, 9, 5)}
    assert len(set(C['odd'][6])) == 3 and np.abs(CR.case_table('odd')).max() == 4 and len(np.unique(CR.case_table('odd').reshape(-1, 2), axis=0)) > 40
    assert (C['vector'][2] * C['vector'][3] * C['vector'][4]) % 4 == 0
    # clipped: every tap range is clipped; centres outside the map whose taps still reach it; cells no tap of which is inside the map, by rows and by columns
    S, T, HH, WW, K, Rr = C['clipped'][:6]
    t = CR.case_table('clipped')
    assert Rr >= HH and Rr >= WW and np.abs(t).max() == 9
    ys, xs = np.arange(HH)[None, None, :, None] + t[..., 0], np.arange(WW)[None, None, None, :] + t[..., 1]
    no_row, no_col = (ys - Rr > HH - 1) | (ys + Rr < 0), (xs - Rr > WW - 1) | (xs + Rr < 0)
    assert no_row[:, 1:].any() and no_col[:, 1:].any() and (((ys > HH - 1) | (ys < 0)) & ~no_row).any() and not (no_row | no_col).all()
    far = CR.case_table('far')
    assert {CR.INT_MIN, CR.INT_MAX, -CR.INT_MAX} <= set(far.reshape(-1).tolist()) and (far[:, :, 2, 2] == 0).all()
    HH, WW, Rr = C['lost'][2], C['lost'][3], C['lost'][5]
    lost = CR.case_table('lost')[0, 2]
    assert C['lost'][7] == 0.0 and ((np.abs(lost[..., 0]) >= HH + Rr) | (np.abs(lost[..., 1]) >= WW + Rr)).all()
    assert C['big'][2] * C['big'][3] == 8192
    real = CR.case_table('real')
    assert np.abs(real).max() == 2 and (real[:, :, :10, :10] == real[:, :, :1, :1]).all() and len(np.unique(real[0, 1].reshape(-1, 2), axis=0)) > 10


def test_lost_resets_and_breaks():
    hm, taps, Rr, sigma, rho, centre, _ = CR.case_inputs('lost', P.seq_taps)
    assert (CR.seq_filter(hm, taps, rho, centre)['reset'][0, :, 0] == (0, 0, 1)).all()
    assert (CR.seq_viterbi(hm, taps, rho, centre)['breaks'][0, :, 0] == (0, 0, 1)).all()


@pytest.mark.parametrize('name', sorted(MR.CASES))
def test_uniform_table_is_the_moving_recurrence(name):
    hm, taps, Rr, sigma, rho, shift, _ = MR.case_inputs(name, P.seq_taps)
    table = CR.uniform_table(shift, hm.shape[2], hm.shape[3])
    _same(CR.seq_filter(hm, taps, rho, table), MR.seq_filter(hm, taps, rho, shift))
    _same(CR.seq_viterbi(hm, taps, rho, table), MR.seq_viterbi(hm, taps, rho, shift))


@pytest.mark.parametrize('name', sorted(R.CASES))
def test_zero_table_is_the_plain_recurrence(name):
    hm, taps, Rr, sigma, rho, _ = R.case_inputs(name, P.seq_taps)
    zero = np.zeros(hm.shape[:4] + (2,), np.int64)
    _same(CR.seq_filter(hm, taps, rho, zero), R.seq_filter(hm, taps, rho))
    _same(CR.seq_viterbi(hm, taps, rho, zero), R.seq_viterbi(hm, taps, rho))


def test_state_carries_the_first_table():
    hm, taps, Rr, sigma, rho, centre, _ = CR.case_inputs('odd', P.seq_taps)
    whole = CR.seq_filter(hm, taps, rho, centre)
    first = CR.seq_filter(hm[:, :2], taps, rho, centre[:, :2])
    second = CR.seq_filter(hm[:, 2:], taps, rho, centre[:, 2:], state=first['state'])
    assert centre[:, 2].any()
    for k in ('belief', 'coords', 'norm', 'reset'):
        assert_array_equal(np.concatenate([first[k], second[k]], axis=1), whole[k])
    assert_array_equal(_bits(second['state']), _bits(whole['state']))


def test_enumeration_of_all_paths():
    """A 3 x 4 map, T = 3, R = 1, a table with a shift of its own per cell, some off the map: the weight of a path x_0 .. x_t is written down from the
    header's sentence -- cell (y, x) of frame t was cell (y + sy, x + sx) of frame t-1, so the step from (y', x') to (y, x) has the taps at
    dy = y + sy - y', dx = x + sx - x' -- and all 12^3 paths are enumerated: the filter's belief is the normalised sum over the paths that end in a
    cell, Viterbi's track the path of the largest weight, the products of norm / maxes the total / largest weight.  Within seq_ref.tolerance."""
    HH, WW, T, Rr, K, rho = 3, 4, 3, 1, 1, 0.05
    HW = HH * WW
    rs = np.random.RandomState(11)
    hm = (rs.rand(1, T, HH, WW, K) * 0.9 + 0.1).astype(np.float32)
    centre = rs.randint(-2, 3, (1, T, HH, WW, 2)).astype(np.int64)
    centre[0, 1, 0, 0] = (HH + Rr, 0)      # no tap reaches the map: the uniform term alone
    centre[0, 2, 2, 3] = (0, -(WW + Rr))
    taps = P.seq_taps(0.9, Rr, K)
    w, om, u = taps[0], 1.0 - rho, rho / HW
    p = hm[0, :, :, :, 0].astype(np.float64).reshape(T, HW)
    step = np.zeros((T, HW, HW))      # step[t, to, from]: the motion kernel alone
    for t, y, x, y_, x_ in itertools.product(range(1, T), range(HH), range(WW), range(HH), range(WW)):
        dy, dx = y + int(centre[0, t, y, x, 0]) - y_, x + int(centre[0, t, y, x, 1]) - x_
        if abs(dy) <= Rr and abs(dx) <= Rr:
            step[t, y * WW + x, y_ * WW + x_] = w[dy + Rr] * w[dx + Rr]
    f, v = CR.seq_filter(hm, taps, rho, centre), CR.seq_viterbi(hm, taps, rho, centre)
    assert not f['reset'].any() and not v['breaks'].any()
    tol = R.tolerance(T - 1, HW, Rr)
    # paths[x0, x1, x2]
    sums = p[0][:, None, None] * (om * step[1].T + u)[:, :, None] * p[1][None, :, None] * (om * step[2].T + u)[None, :, :] * p[2][None, None, :]
    two = p[0][:, None] * (om * step[1].T + u) * p[1][None, :]
    for t, marg in ((0, p[0]), (1, two.sum(axis=0)), (2, sums.sum(axis=(0, 1)))):
        want = marg / marg.sum()
        got = f['belief'][0, t, :, :, 0].reshape(-1)
        assert (np.abs(got - want) <= tol * want).all(), t
        assert tuple(f['coords'][0, t, :, 0]) == divmod(int(np.argmax(want)), WW)
    assert abs(np.prod(f['norm']) - sums.sum()) <= 3 * tol * sums.sum()
    maxs = p[0][:, None, None] * np.maximum(om * step[1].T, u)[:, :, None] * p[1][None, :, None] * np.maximum(om * step[2].T, u)[None, :, :] * p[2][None, None, :]
    best = np.unravel_index(int(np.argmax(maxs)), maxs.shape)
    flat = np.sort(maxs.reshape(-1))
    assert flat[-1] - flat[-2] > 10 * tol * flat[-1]      # the best path is not a tie
    assert_array_equal(v['path'][0, :, :, 0], [divmod(int(c), WW) for c in best])
    assert abs(np.prod(v['maxes']) - maxs.max()) <= 3 * tol * maxs.max()


# ------------------------------------------------------------------ pixels to cells
def test_flow_cell_shifts_is_the_stated_rule():
    d = np.arange(-17, 18)
    want = np.array([int(np.floor((int(v) + 4) / 8.0)) for v in d])      # round half up, in cells
    assert dict(zip(d.tolist(), want.tolist()))[4] == 1 and want[d == -4] == 0 and want[d == -5] == -1 and want[d == 3] == 0 and want[d == -12] == -1
    flow = np.stack([d, d[::-1]], axis=1).reshape(1, 5, 7, 2).astype(np.int32)
    both = np.stack([want, want[::-1]], axis=1).reshape(1, 5, 7, 2)
    got = motion.flow_cell_shifts(torch.from_numpy(flow))
    assert isinstance(got, torch.Tensor) and got.dtype == torch.int32 and got.device == torch.device('cpu')
    assert_array_equal(got.numpy(), both)
    got = motion.flow_cell_shifts(flow)
    assert got.dtype == np.int32
    assert_array_equal(got, both)
    assert P.flow_cell_shifts is motion.flow_cell_shifts
    for line in ('floor((d + stride // 2) / stride)', '4 -> 1', '-4 -> 0', '-5 -> -1'):
        assert line in motion.flow_cell_shifts.__doc__
    with pytest.raises(ValueError, match='integer'):
        motion.flow_cell_shifts(torch.zeros(1, 2, 2, 2))
    with pytest.raises(ValueError, match='integer'):
        motion.flow_cell_shifts(np.zeros((1, 2, 2, 2)))


# ------------------------------------------------------------------ the host layers refuse before a device is touched
def test_entry_points_refuse_what_is_out_of_scope():
    frames = [np.zeros((4, 4, 3), np.uint8)]
    for kw, match in ((dict(camera=True), 'camera=True'), (dict(mode='marginal'), "'filter' or 'viterbi'"), (dict(mode='lag', lag=2), "'filter' or 'viterbi'"),
                      (dict(fit_iters=3), 'fit_iters'), (dict(flow_search=0), 'flow_search'), (dict(flow_search=17), 'flow_search'),
                      (dict(flow=1, mode='marginal'), "'filter' or 'viterbi'")):
        with pytest.raises(ValueError, match=match):
            P.predict_sequence(None, frames, flow_centre=True, **kw)
    with pytest.raises(ValueError, match='flow_centre'):
        P.predict_sequence_zoom(None, frames, flow_centre=True)
    with pytest.raises(ValueError, match='flow_centre'):
        P.predict_sequence_people(None, frames, 2, flow_centre=True)
    with pytest.raises(ValueError, match='camera=True'):
        P.SequenceTracker(None, flow_centre=True, camera=True)
    with pytest.raises(ValueError, match='flow_search'):
        P.SequenceTracker(None, flow_centre=True, flow_search=0)
    tracker = P.SequenceTracker(None, flow_centre=True, flow_search=5)
    assert tracker.flow_centre and tracker.flow_search == 5 and tracker.pass1['keep_frames'] and tracker.last_frame is None
    tracker.last_frame = 'a frame'
    tracker.reset()
    assert tracker.last_frame is None and tracker.state is None
    assert not P.SequenceTracker(None).flow_centre and 'keep_frames' not in P.SequenceTracker(None).pass1
    assert P.SEQ_FLOW_CENTRE_MODES == ('filter', 'viterbi')


def test_docstrings_state_the_limits():
    doc = ' '.join(P.predict_sequence.__doc__.split())
    assert 'flow_centre=True' in doc and 'no gating' in doc and 'has not been measured' in doc
    assert 'any split gives the bits of the one call' in ' '.join(P.SequenceTracker.__doc__.split())


PREDICT = ['--predict', 'x', '--predictions', 'o.json']
REFUSALS = (
    (['--seq_flow_centre'] + PREDICT, 'SEQ_FLOW_CENTRE_NEEDS_SEQUENCE'),
    (['--seq_flow_centre', '--sequence', 'marginal'] + PREDICT, 'SEQ_FLOW_CENTRE_NO_SMOOTHER'),
    (['--seq_flow_centre', '--sequence', 'lag', '--seq_lag', '2'] + PREDICT, 'SEQ_FLOW_CENTRE_NO_SMOOTHER'),
    (['--seq_flow_centre', '--sequence', 'filter', '--seq_fit', '3'] + PREDICT, 'SEQ_FLOW_CENTRE_NO_FIT'),
    (['--seq_flow_centre', '--sequence', 'filter', '--seq_camera'] + PREDICT, 'SEQ_FLOW_CENTRE_NO_CAMERA'),
    (['--seq_flow_centre', '--sequence', 'viterbi', '--use_sm', '--seq_zoom'] + PREDICT, 'SEQ_FLOW_CENTRE_NO_ZOOM'),
    (['--seq_flow_centre', '--sequence', 'viterbi', '--use_sm', '--seq_people', '2'] + PREDICT, 'SEQ_FLOW_CENTRE_NO_PEOPLE'),
    # what was refused stays refused, with its message
    (['--seq_flow_search', '4', '--sequence', 'filter'] + PREDICT, 'SEQ_FLOW_SEARCH_NEEDS_SEQ_FLOW'),
    (['--seq_flow_centre', '--seq_flow', '2', '--sequence', 'lag', '--seq_lag', '2'] + PREDICT, 'SEQ_FLOW_NO_LAG'),      # an earlier table wins
)


def _refusal(argv):
    keep = argparse.Namespace(**vars(M.hps))
    try:
        with pytest.raises(SystemExit) as ei:
            M.main(list(argv) + ['--gpus', '99'])
    finally:
        M.hps = keep
    return ei.value.code


@pytest.mark.parametrize('argv,name', REFUSALS)
def test_cli_refusals(argv, name):
    assert _refusal(argv) == getattr(M, name)


def test_new_rules_are_a_table_behind_the_others():
    new = [M.SEQ_FLOW_CENTRE_NEEDS_SEQUENCE, M.SEQ_FLOW_CENTRE_NO_SMOOTHER, M.SEQ_FLOW_CENTRE_NO_FIT, M.SEQ_FLOW_CENTRE_NO_CAMERA, M.SEQ_FLOW_CENTRE_NO_ZOOM,
           M.SEQ_FLOW_CENTRE_NO_PEOPLE]
    assert [m for _, m in M.SEQ_FLOW_CENTRE_RULES] == new and len(set(new)) == 6
    earlier = (M.FLAG_RULES + M.SEQUENCE_RULES + M.AUGM_RULES + M.SEQ_PEOPLE_RULES + M.SYNTH_PEOPLE_RULES + M.SEQ_SMOOTH_RULES + M.SEQ_ZOOM_RULES + M.SEQ_LAG_RULES +
               M.SEQ_CAMERA_RULES + M.EVAL_SCALE_RULES + M.SEQ_FLOW_RULES)
    assert not set(new) & {m for _, m in earlier if not callable(m)}
    assert len(M.SEQ_FLOW_RULES) == 7 and len(M.SEQ_CAMERA_RULES) == 7
    assert not M.build_parser().parse_args([]).seq_flow_centre
    # an accepted combination passes every rule and stops at the device check
    for extra in ([], ['--seq_flow', '2'], ['--seq_flow_search', '4'], ['--seq_flow', '1', '--seq_flow_search', '16'], ['--render', 'out']):
        for mode in ('filter', 'viterbi'):
            assert '--gpus' in str(_refusal(['--seq_flow_centre', '--sequence', mode] + extra + PREDICT)), (extra, mode)


def test_entry_points_are_bound_and_exported():
    lib = _lib.load()
    for name in ('jcm_seq_filter_centred', 'jcm_seq_viterbi_centred'):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert len(_lib.SIGNATURES['jcm_seq_filter_centred'][1]) == len(_lib.SIGNATURES['jcm_seq_filter_moving'][1])
    assert len(_lib.SIGNATURES['jcm_seq_viterbi_centred'][1]) == len(_lib.SIGNATURES['jcm_seq_viterbi_moving'][1])
