"""Zoomed clips without a device: the numpy restatement of the moving recurrences (tests/seq_moving_ref.py) is pinned -- against
tests/seq_ref.py at zero shift, and, independently of any kernel, against the plain recurrences on the UNION lattice, which fixes the sign
convention of the shift --, the one-lattice windows of predict.zoom_window_track, and the rules of --seq_zoom."""
import argparse

import numpy as np
import pytest
from numpy.testing import assert_array_equal

import seq_moving_ref as MR
import seq_ref as R
import joint_cnn_mrf_amd  # noqa: F401
from joint_cnn_mrf_amd import main as M
from joint_cnn_mrf_amd import predict as P
from joint_cnn_mrf_amd.evaluation import fit_geometry


def _bits(a):
    return np.asarray(a, np.float64).view(np.int64)


# ------------------------------------------------------------------ the restatement
@pytest.mark.parametrize('name', sorted(MR.CASES))
def test_shared_cases_have_a_clear_arg_max(name):
    hm, taps, Rr, sigma, rho, shift, seed = MR.case_inputs(name, P.seq_taps)
    S, T, HH, WW, K = hm.shape
    assert shift.shape == (S, T, 2)
    gap = R.top2_gap(MR.seq_filter(hm, taps, rho, shift)['belief'])
    for t in range(T):
        assert (gap[:, t] > 10.0 * R.tolerance(t, HH * WW, Rr)).all(), (name, t, seed)


def test_cases_cover_what_the_index_arithmetic_can_get_wrong():
    C = MR.CASES
    S, T, HH, WW, K, Rr = C['clipped'][:6]
    assert Rr >= HH and Rr >= WW and {(abs(a), abs(b)) for a, b in C['clipped'][8][0][1:]} == {(1, 2)}
    assert C['odd'][0] == 2 and C['odd'][8][0] != C['odd'][8][1] and max(max(abs(a), abs(b)) for a, b in C['odd'][8][0]) > C['odd'][5]
    assert (C['vector'][2] * C['vector'][3] * C['vector'][4]) % 4 == 0
    HH, WW, Rr = C['far_rows'][2], C['far_rows'][3], C['far_rows'][5]
    assert any(abs(a) >= HH + Rr for a, _ in C['far_rows'][8][0]) and any(HH <= abs(a) < HH + Rr for a, _ in C['far_rows'][8][0])
    assert any(abs(b) >= WW + Rr for _, b in C['far_cols'][8][0]) and any(WW <= abs(b) < WW + Rr for _, b in C['far_cols'][8][0])
    assert C['rho0'][7] == 0.0 and C['rho1'][7] == 1.0 and C['radius0'][5] == 0 and C['one_frame'][1] == 1
    assert C['real'][:5] == (1, 4, 60, 90, 9) and C['split'][8][0][3] != (0, 0)


@pytest.mark.parametrize('name', sorted(R.CASES))
def test_zero_shift_is_the_plain_recurrence(name):
    hm, taps, Rr, sigma, rho, _ = R.case_inputs(name, P.seq_taps)
    S, T = hm.shape[:2]
    zero = np.zeros((S, T, 2), np.int64)
    f0, f1 = R.seq_filter(hm, taps, rho), MR.seq_filter(hm, taps, rho, zero)
    for k in f0:
        assert_array_equal(f1[k], f0[k])
    assert_array_equal(_bits(f1['belief']), _bits(f0['belief']))
    assert_array_equal(_bits(f1['norm']), _bits(f0['norm']))
    v0, v1 = R.seq_viterbi(hm, taps, rho), MR.seq_viterbi(hm, taps, rho, zero)
    assert_array_equal(v1['path'], v0['path'])
    assert_array_equal(v1['breaks'], v0['breaks'])
    assert_array_equal(_bits(v1['maxes']), _bits(v0['maxes']))


UNION = (  # (T, HH, WW, K, R, sigma, shifts): rho is 0, so that the uniform term does not depend on the size of the lattice
    (5, 7, 9, 2, 2, 1.0, [(0, 0), (1, -2), (-2, 1), (3, 2), (-1, -1)]),
    (4, 5, 7, 1, 3, 1.5, [(0, 0), (2, 0), (0, -3), (-1, 1)]),
    (3, 6, 5, 2, 1, 0.7, [(0, 0), (-1, -1), (1, 2)]),
)


@pytest.mark.parametrize('case', range(len(UNION)))
def test_moving_equals_plain_on_the_union_lattice(case):
    """The same maps zero-padded at their window offsets into the bounding box of all windows, through the PLAIN restatement: with rho = 0 the
    moving Viterbi path, mapped to union cells, is the plain path exactly and maxes are the same bits (products, quotients and maxima only; the
    zeros around a window add nothing to a maximum), and the moving filter's beliefs agree within seq_ref.tolerance (the order of Z differs)."""
    T, HH, WW, K, Rr, sigma, shifts = UNION[case]
    taps = P.seq_taps(sigma, Rr, K)
    shift = np.array(shifts, np.int64)
    hm = None
    for seed in range(100):      # dense maps, so that no frame breaks: a break's arg-max of an all-ones d would depend on the lattice
        rs = np.random.RandomState(4000 + seed)
        cand = (rs.rand(1, T, HH, WW, K) * 0.9 + 0.1).astype(np.float32)
        mv = MR.seq_viterbi(cand, taps, 0.0, shift[None])
        mf = MR.seq_filter(cand, taps, 0.0, shift[None], kernel_order=False)
        if not mv['breaks'].any() and not mf['reset'].any() and (R.top2_gap(mf['belief']) > 1e-6).all():
            hm = cand
            break
    assert hm is not None
    union, org = MR.on_union(hm[0], shift)
    assert union.shape[2] > HH and union.shape[3] > WW
    pv = R.seq_viterbi(union, taps, 0.0)
    assert not pv['breaks'].any()
    assert_array_equal(mv['path'][0] + org[:, :, None], pv['path'][0])
    assert_array_equal(_bits(mv['maxes']), _bits(pv['maxes']))
    pf = R.seq_filter(union, taps, 0.0, kernel_order=False)
    assert not pf['reset'].any()
    assert_array_equal(mf['coords'][0] + org[:, :, None], pf['coords'][0])
    for t in range(T):
        inner = pf['belief'][0, t, org[t, 0]:org[t, 0] + HH, org[t, 1]:org[t, 1] + WW]
        want = mf['belief'][0, t]
        tol = R.tolerance(t, union.shape[2] * union.shape[3], Rr)
        assert (np.abs(inner - want) <= tol * np.abs(want)).all()
        outer = pf['belief'][0, t].copy()
        outer[org[t, 0]:org[t, 0] + HH, org[t, 1]:org[t, 1] + WW] = 0
        assert not outer.any()


def test_a_delta_follows_the_shift():
    """The sign convention in one line: a delta at (2, 3) of frame 0, seen from a frame whose lattice lies (+1, -2) on it, is at (1, 5)."""
    hm = np.zeros((1, 2, 5, 8, 1), np.float32)
    hm[0, 0, 2, 3, 0] = 1.0
    hm[0, 1] = 1.0
    taps = np.array([[1.0]])
    shift = np.array([[(0, 0), (1, -2)]])
    f, v = MR.seq_filter(hm, taps, 0.0, shift), MR.seq_viterbi(hm, taps, 0.0, shift)
    assert_array_equal(f['coords'][0, :, :, 0], [[2, 3], [1, 5]])
    assert_array_equal(v['path'][0, :, :, 0], [[2, 3], [1, 5]])


def test_state_carries_the_first_shift():
    hm, taps, Rr, sigma, rho, shift, _ = MR.case_inputs('split', P.seq_taps)
    whole = MR.seq_filter(hm, taps, rho, shift)
    first = MR.seq_filter(hm[:, :3], taps, rho, shift[:, :3])
    second = MR.seq_filter(hm[:, 3:], taps, rho, shift[:, 3:], state=first['state'])
    assert shift[0, 3].any()
    for k in ('belief', 'coords', 'norm', 'reset'):
        assert_array_equal(np.concatenate([first[k], second[k]], axis=1), whole[k])
    assert_array_equal(_bits(second['state']), _bits(whole['state']))


# ------------------------------------------------------------------ one lattice per clip
def _person(T, cy, cx, tlen, K=9):
    """Joints whose shoulders lie tlen above the hips, around (cy, cx): points [T,K,2], inside [T,K]."""
    pts = np.zeros((T, K, 2))
    for t in range(T):
        pts[t, :, 0], pts[t, :, 1] = cy[t], cx[t]
        for j in (0, 3):
            pts[t, j, 0] = cy[t] - tlen[t] / 2
        for j in (6, 7):
            pts[t, j, 0] = cy[t] + tlen[t] / 2
    return pts, np.ones((T, K), bool)


GEOM = (0, 0, 480, 720, 1080, 1620)


def test_window_track_is_one_lattice():
    T = 6
    cy = np.array([500.2, 503.9, 520.0, 519.4, 480.7, 470.1])
    cx = np.array([800.0, 811.3, 835.8, 860.2, 858.9, 840.0])
    tlen = np.array([198.0, 202.0, 200.0, 204.0, 196.0, 201.0])
    pts, inside = _person(T, cy, cx, tlen)
    torso = np.stack([cy, cx], axis=1)
    wins, cells, shift, p, valid = P.zoom_window_track(pts, inside, torso, GEOM)
    assert valid.all() and wins.dtype == np.int64 and cells.dtype == np.int32 and shift.dtype == np.int32
    assert p == max(1, int(np.floor(np.median(tlen) * 8 / P.ZOOM_TORSO_PIXELS + 0.5))) == 12
    assert_array_equal(wins[:, 0], np.arange(T))
    assert (wins[:, 3] == 60 * p).all() and (wins[:, 4] == 90 * p).all()
    assert not (wins[:, 1:3] % p).any()
    assert_array_equal(shift[0], (0, 0))
    assert_array_equal(shift[1:] * p, wins[1:, 1:3] - wins[:-1, 1:3])
    assert_array_equal(np.cumsum(shift, axis=0) * p, wins[:, 1:3] - wins[0, 1:3])      # the shifts telescope to the origin differences
    assert shift[1:].any()
    # the window is centred on the torso point within half a pitch, and the blob goes to the middle of the map
    assert (np.abs(wins[:, 1] + 30 * p - cy) <= p / 2).all() and (np.abs(wins[:, 2] + 45 * p - cx) <= p / 2).all()
    assert (np.abs(cells - (30, 45)) <= 1).all()
    # a [T,6] geom is the same call
    again = P.zoom_window_track(pts, inside, torso, np.tile(GEOM, (T, 1)))
    for a, b in zip(again, (wins, cells, shift, p, valid)):
        assert_array_equal(a, b)


def test_every_pitch_fits_the_whole_frame():
    for p in range(1, 183):
        assert fit_geometry(60 * p, 90 * p, 480, 720) == (0, 0, 480, 720)
    assert 90 * 182 <= P.FIT_SIDE_MAX < 90 * 183


def test_window_track_median_validity_and_refusals():
    T = 5
    cy, cx = np.full(T, 300.0), np.full(T, 400.0)
    tlen = np.array([100.0, 10.0, 140.0, 120.0, 3000.0])      # frame 1 is below two pass-1 cells (2 * 8 * 1080 / 480 = 36 pixels)
    pts, inside = _person(T, cy, cx, tlen)
    inside[4, 6] = False                                          # frame 4 lacks a hip
    wins, cells, shift, p, valid = P.zoom_window_track(pts, inside, np.stack([cy, cx], 1), GEOM)
    assert_array_equal(valid, [True, False, True, True, False])
    assert p == int(np.floor(120.0 * 8 / P.ZOOM_TORSO_PIXELS + 0.5))      # the median of the valid frames: 120
    assert (wins[:, 3] == 60 * p).all()                                   # every frame gets a window, a valid one or not
    # no valid frame: the clip is not zoomed
    wins, cells, shift, p, valid = P.zoom_window_track(pts, np.zeros_like(inside), np.stack([cy, cx], 1), GEOM)
    assert p == 0 and not valid.any() and not wins[:, 1:].any() and not cells.any() and not shift.any() and wins.shape == (T, 5)
    # a torso that would need a window beyond what a fit takes
    big, inside = _person(1, [300.0], [400.0], [3000.0])
    with pytest.raises(ValueError, match='16384'):
        P.zoom_window_track(big, inside, np.array([[300.0, 400.0]]), GEOM)
    with pytest.raises(ValueError, match='expects'):
        P.zoom_window_track(big[:, :4], inside[:, :4], np.array([[300.0, 400.0]]), GEOM)


def test_window_track_clamps_to_the_nearest_origin_that_holds_a_pixel():
    T = 4
    h, w = GEOM[4], GEOM[5]
    cy = np.array([-5000.0, 9000.0, 500.0, 500.0])
    cx = np.array([700.0, 700.0, -9000.0, 90000.0])
    pts, inside = _person(T, np.full(T, 500.0), np.full(T, 700.0), np.full(T, 200.0))
    wins, cells, shift, p, valid = P.zoom_window_track(pts, inside, np.stack([cy, cx], 1), GEOM)
    assert p == 12
    assert wins[0, 1] == -59 * p and wins[1, 1] == p * ((h - 1) // p) and wins[2, 2] == -89 * p and wins[3, 2] == p * ((w - 1) // p)
    for t in range(T):
        y0, x0, wh, ww = wins[t, 1:]
        assert y0 < h and y0 + wh > 0 and x0 < w and x0 + ww > 0                          # the window holds a pixel of the frame ...
        assert not (wins[t, 1:3] % p).any()
    assert wins[0, 1] - p + wins[0, 3] <= 0 and wins[1, 1] + p >= h                       # ... and the next origin outwards holds none
    assert wins[2, 2] - p + wins[2, 4] <= 0 and wins[3, 2] + p >= w
    assert (cells >= 0).all() and (cells[:, 0] <= 59).all() and (cells[:, 1] <= 89).all()
    assert_array_equal(np.cumsum(shift, axis=0) * p, wins[:, 1:3] - wins[0, 1:3])


def test_docstrings_state_the_limits():
    for doc in (P.zoom_window_track.__doc__, P.predict_sequence_zoom.__doc__):
        assert 'One pitch per clip is a stated limit' in ' '.join(doc.split())
    assert 'has not been measured' in ' '.join(P.predict_sequence_zoom.__doc__.split())


# ------------------------------------------------------------------ the command line and the entry points
PREDICT = ['--predict', 'x', '--predictions', 'o.json']
REFUSALS = (
    (['--seq_zoom', '--use_sm'] + PREDICT, 'SEQ_ZOOM_NEEDS_SEQUENCE'),
    (['--seq_zoom', '--sequence', 'viterbi'] + PREDICT, 'SEQ_ZOOM_NEEDS_USE_SM'),
    (['--seq_zoom', '--sequence', 'marginal', '--use_sm'] + PREDICT, 'SEQ_ZOOM_NO_MARGINAL'),
    (['--seq_zoom', '--sequence', 'filter', '--use_sm', '--seq_fit', '3'] + PREDICT, 'SEQ_ZOOM_NO_FIT'),
    (['--seq_zoom', '--sequence', 'viterbi', '--use_sm', '--seq_people', '2'] + PREDICT, 'SEQ_ZOOM_NO_PEOPLE'),
    # what was refused stays refused, with its message
    (['--sequence', 'viterbi', '--use_sm', '--zoom'] + PREDICT, 'SEQUENCE_NO_ZOOM'),
    (['--sequence', 'viterbi', '--use_sm', '--zoom', '--seq_zoom'] + PREDICT, 'SEQUENCE_NO_ZOOM'),
    # an earlier table wins over the new one
    (['--seq_zoom', '--seq_fit', '3'], 'SEQ_FIT_NEEDS_SEQUENCE'),
    (['--seq_zoom', '--sequence', 'viterbi'], 'SEQUENCE_NEEDS_PREDICT'),
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
    new = [M.SEQ_ZOOM_NEEDS_SEQUENCE, M.SEQ_ZOOM_NEEDS_USE_SM, M.SEQ_ZOOM_NO_MARGINAL, M.SEQ_ZOOM_NO_FIT, M.SEQ_ZOOM_NO_PEOPLE]
    assert [m for _, m in M.SEQ_ZOOM_RULES] == new and len(set(new)) == 5
    earlier = M.FLAG_RULES + M.SEQUENCE_RULES + M.AUGM_RULES + M.SEQ_PEOPLE_RULES + M.SYNTH_PEOPLE_RULES + M.SEQ_SMOOTH_RULES
    assert not set(new) & {m for _, m in earlier if not callable(m)}
    assert (len(M.SEQUENCE_RULES), len(M.AUGM_RULES), len(M.SEQ_PEOPLE_RULES), len(M.SYNTH_PEOPLE_RULES), len(M.SEQ_SMOOTH_RULES)) == (4, 5, 6, 5, 4)
    assert M.FLAG_RULES[-1][1] == M.RENDER_HEAT_SM_NEEDS_USE_SM and M.SEQUENCE_RULES[1][1] == M.SEQUENCE_NO_ZOOM
    assert not M.build_parser().parse_args([]).seq_zoom
    # an accepted combination passes every rule and stops at the device check
    for mode in ('filter', 'viterbi'):
        assert '--gpus' in str(_refusal(['--seq_zoom', '--sequence', mode, '--use_sm'] + PREDICT))


def test_entry_points_refuse_what_is_out_of_scope():
    frames = [np.zeros((4, 4, 3), np.uint8)]
    with pytest.raises(ValueError, match='zoom'):
        P.predict_sequence(None, frames, zoom=True)
    with pytest.raises(ValueError, match='marginal'):
        P.predict_sequence_zoom(None, frames, mode='marginal')
    with pytest.raises(ValueError, match='fit_iters'):
        P.predict_sequence_zoom(None, frames, fit_iters=3)
    with pytest.raises(ValueError, match='people'):
        P.predict_sequence_zoom(None, frames, people=2)
    with pytest.raises(ValueError, match='track_zoom'):
        P.skeleton_primitives([{'size': (4, 4), 'sm': None}], which='track_zoom')
    with pytest.raises(ValueError, match="'track_zoom'"):
        P.skeleton_primitives([], which='zoom_track')


def test_track_zoom_is_drawn():
    pts = np.array([[10.0 + j, 20.0 + 2 * j] for j in range(9)])
    r = {'size': (100, 200), 'sm': pts + 30, 'sm_inside': np.ones(9, bool), 'track': {'points': pts + 5, 'inside': np.ones(9, bool)},
         'track_zoom': {'points': pts, 'inside': np.ones(9, bool)}}
    prims = P.skeleton_primitives([r], which='track_zoom')
    want = P.skeleton_primitives([dict(r, sm=pts)], which='sm', zoom=False)
    assert_array_equal(prims, want)
    assert len(prims) == 18
