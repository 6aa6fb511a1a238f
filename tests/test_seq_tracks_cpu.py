"""Several torso tracks without a GPU: the restatement tests/seq_tracks_ref.py -- what tests/test_gpu_seq_tracks.py holds the
kernels to, bit for bit -- on a case worked out by hand, on the properties the definition promises, and the new command-line rules."""
import argparse

import numpy as np
import pytest
from numpy.testing import assert_array_equal

import seq_ref as R
import seq_tracks_ref as TR
import joint_cnn_mrf_amd  # noqa: F401
from joint_cnn_mrf_amd import main as M
from joint_cnn_mrf_amd import predict as P

W3 = np.array([[0.25, 0.5, 0.25]])


def test_hand_case():
    """3 x 4 cells, T = 3, M = 2, D = 1, taps (1/4, 1/2, 1/4), rho = 0; every value a power of two.  Person A (value 1) sits at (0,0) and steps to
    (0,1); person B (value 1/2) sits at (2,3) and is gone in frame 2, where a cell (2,0) of value 1/4 appears.
    Track 0: d_0 = p_0.  Frame 1: the way into (0,1) is dx = 1 from (0,0): m = w[2] * (w[1] * 1) = 1/8, b = 1/8; into (2,3): m = 1/2 * 1/2 * 1/2 =
    1/8, b = 1/16; M = 1/8.  Frame 2: (0,1) stays, m = 1/4 = b = M; (2,0) has no source within one cell, b = 0.  Path A, values 1.
    Track 1 sees the maps without rows 0-1 x columns 0-1 (frame 0) and rows 0-1 x columns 0-2 (frames 1, 2): B alone, M = 1/2, then it stays,
    m = 1/4, b = M = 1/8; in frame 2 only (2,0) is left, three columns away: every b is 0, a break (code 1), b = p, M = 1/4; the earlier segment
    ends at the arg-max of d_1, B's cell."""
    hm = np.zeros((1, 3, 3, 4), np.float32)
    hm[0, 0, 0, 0] = hm[0, 1, 0, 1] = hm[0, 2, 0, 1] = 1.0
    hm[0, 0, 2, 3] = hm[0, 1, 2, 3] = 0.5
    hm[0, 2, 2, 0] = 0.25
    r = TR.seq_tracks_viterbi(hm, 2, W3, 0.0, 1)
    assert_array_equal(r['path'][0], [[[0, 0], [0, 1], [0, 1]], [[2, 3], [2, 3], [2, 0]]])
    assert_array_equal(r['value'][0], [[1.0, 1.0, 1.0], [0.5, 0.5, 0.25]])
    assert_array_equal(r['breaks'][0], [[0, 0, 0], [0, 0, 1]])
    assert_array_equal(r['maxes'][0], [[1.0, 0.125, 0.25], [0.5, 0.125, 0.25]])
    f = TR.seq_tracks_filter(hm, 2, W3, 0.0, 1)
    assert_array_equal(f['coords'][0], r['path'][0])
    assert_array_equal(f['value'][0], r['value'][0])
    assert_array_equal(f['reset'][0], r['breaks'][0])


@pytest.mark.parametrize('rho', [0.0, 0.05])
def test_one_track_is_the_single_track(rho):
    hm = R.random_maps((2, 4, 7, 9, 1), 11)
    taps = P.seq_taps(1.5, 3, 1)
    v, f = TR.seq_tracks_viterbi(hm[..., 0], 1, taps, rho, 2), TR.seq_tracks_filter(hm[..., 0], 1, taps, rho, 2)
    v1, f1 = R.seq_viterbi(hm, taps, rho), R.seq_filter(hm, taps, rho)
    for k in v1:
        assert_array_equal(v[k][:, 0], v1[k][..., 0])
    for k in ('coords', 'norm', 'reset', 'filtered'):
        assert_array_equal(f[k][:, 0], f1[k][..., 0])
    assert_array_equal(f['state'][:, 0], f1['state'].reshape(2, 63))
    # more tracks leave track 0 as it is
    v3 = TR.seq_tracks_viterbi(hm[..., 0], 3, taps, rho, 2)
    for k in v:
        assert_array_equal(v3[k][:, :1], v[k])


def _crossing():
    """9 x 15 cells, T = 7: A walks along row 2 from column 1 to column 13, B along row 6 from column 13 to column 1, two cells a frame, so they
    pass each other four rows apart.  A is the brighter one (1) for four frames and the dimmer one (1/2 against B's 0.6) after that."""
    T = 7
    a = [(2, 1 + 2 * t) for t in range(T)]
    b = [(6, 13 - 2 * t) for t in range(T)]
    hm = np.zeros((1, T, 9, 15), np.float32)
    for t in range(T):
        hm[0, t][a[t]] = 1.0 if t < 4 else 0.5
        hm[0, t][b[t]] = 0.6
    return hm, np.array(a), np.array(b)


@pytest.mark.parametrize('mode', ['viterbi', 'filter'])
def test_crossing_people_keep_their_identity(mode):
    hm, a, b = _crossing()
    taps = P.seq_taps(1.5, 5, 1)
    # the per-frame order, what --people gives, swaps: the brightest cell is A's in the first four frames and B's in the last three
    first = np.array([np.unravel_index(np.argmax(hm[0, t]), (9, 15)) for t in range(7)])
    assert_array_equal(first[:4], a[:4])
    assert_array_equal(first[4:], b[4:])
    r = (TR.seq_tracks_viterbi if mode == 'viterbi' else TR.seq_tracks_filter)(hm, 2, taps, 0.05, 1)
    cells = r['path' if mode == 'viterbi' else 'coords']
    assert_array_equal(cells[0, 0], a)
    assert_array_equal(cells[0, 1], b)
    assert_array_equal(r['value'][0, 1], np.full(7, np.float32(0.6)))


def test_exclusion_of_the_whole_map():
    """D reaches every cell: nothing is left for the tracks after the first, which have value 0 and code 2 in every frame -- and, having no
    support, exclude nothing themselves: track 2 sees what track 1 saw."""
    hm = R.random_maps((2, 4, 7, 9, 1), 12)[..., 0]
    taps = P.seq_taps(1.5, 3, 1)
    v, f = TR.seq_tracks_viterbi(hm, 3, taps, 0.05, 64), TR.seq_tracks_filter(hm, 3, taps, 0.05, 64)
    for r, flag, num in ((v, 'breaks', 'maxes'), (f, 'reset', 'norm')):
        assert (r['value'][:, 0] > 0).all()
        assert (r['value'][:, 1:] == 0).all() and (r[flag][:, 1:] == 2).all() and (r[num][:, 1:] == 0).all()
    cells = v['path']
    assert_array_equal(TR.masked(hm, cells[:, :2], v['value'][:, :2], 64), TR.masked(hm, cells[:, :1], v['value'][:, :1], 64))


def test_a_track_without_support_excludes_nothing():
    hm = R.random_maps((1, 3, 7, 9, 1), 13)[..., 0]
    cells = np.array([[[[3, 4], [3, 4], [3, 4]]]])
    value = np.array([[[0.5, 0.0, 0.25]]], np.float32)
    p = TR.masked(hm, cells, value, 1)
    assert_array_equal(p[0, 1], hm[0, 1])
    for t in (0, 2):
        assert (p[0, t, 2:5, 3:6] == 0).all()
        keep = np.ones((7, 9), bool)
        keep[2:5, 3:6] = False
        assert_array_equal(p[0, t][keep], hm[0, t][keep])
    # at the border the square is clipped, not wrapped
    p = TR.masked(hm, np.array([[[[0, 8]] * 3]]), np.ones((1, 1, 3), np.float32), 2)
    assert (p[0, :, 0:3, 6:9] == 0).all() and int((p != hm).sum()) <= 27 and (p[0, :, :, 0:6] == hm[0, :, :, 0:6]).all()


# ------------------------------------------------------------------ the command line
PREDICT = ['--predict', 'x', '--predictions', 'o.json']
REFUSALS = (
    (['--seq_people', '2'] + PREDICT + ['--use_sm'], 'SEQ_PEOPLE_NEEDS_SEQUENCE'),
    (['--seq_people', '2', '--sequence', 'viterbi'] + PREDICT, 'SEQ_PEOPLE_NEEDS_USE_SM'),
    (['--seq_people', '5', '--sequence', 'viterbi', '--use_sm'] + PREDICT, '--seq_people 5: 1 <= M <= 4'),
    (['--seq_people', '0', '--sequence', 'filter', '--use_sm'] + PREDICT, '--seq_people 0: 1 <= M <= 4'),
    (['--seq_exclude', '3', '--sequence', 'filter', '--use_sm'] + PREDICT, 'SEQ_PEOPLE_OPTION_NEEDS_SEQ_PEOPLE'),
    (['--seq_torso_sigma', '2.0'], 'SEQ_PEOPLE_OPTION_NEEDS_SEQ_PEOPLE'),
    (['--seq_people', '2', '--seq_torso_sigma', '0', '--sequence', 'filter', '--use_sm'] + PREDICT, '--seq_torso_sigma 0: CELLS > 0'),
    (['--seq_people', '2', '--seq_exclude', '65', '--sequence', 'filter', '--use_sm'] + PREDICT, '--seq_exclude 65: 0 <= CELLS <= 64'),
    # what was refused stays refused, with its message: --people is not the way to several people in a clip
    (['--sequence', 'viterbi', '--use_sm', '--people', '2'] + PREDICT, 'SEQUENCE_ONE_PERSON'),
    (['--sequence', 'viterbi', '--use_sm', '--people', '2', '--seq_people', '2'] + PREDICT, 'SEQUENCE_ONE_PERSON'),
    # an earlier table wins over the new one
    (['--augm_affine', '--seq_people', '2'], 'AUGM_AFFINE_NEEDS_TRAIN'),
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
    assert _refusal(argv) == getattr(M, name, name)


def test_new_rules_are_a_table_behind_the_others():
    new = [M.SEQ_PEOPLE_NEEDS_SEQUENCE, M.SEQ_PEOPLE_NEEDS_USE_SM, M.SEQ_PEOPLE_OPTION_NEEDS_SEQ_PEOPLE]
    fixed = [m for _, m in M.SEQ_PEOPLE_RULES if not callable(m)]
    assert fixed == new and len(M.SEQ_PEOPLE_RULES) == 6
    earlier = {m for _, m in M.FLAG_RULES + M.SEQUENCE_RULES + M.AUGM_RULES if not callable(m)}
    assert not set(new) & earlier
    assert len(M.SEQUENCE_RULES) == 4 and len(M.AUGM_RULES) == 5 and M.FLAG_RULES[-1][1] == M.RENDER_HEAT_SM_NEEDS_USE_SM
    # an accepted combination passes every rule and stops at the device check
    assert '--gpus' in str(_refusal(['--seq_people', '2', '--seq_exclude', '3', '--seq_torso_sigma', '2', '--sequence', 'viterbi', '--use_sm'] + PREDICT))


def test_defaults_are_declared_placeholders():
    assert (P.SEQ_EXCLUDE, P.SEQ_TORSO_SIGMA) == (4, 1.5)
    text = ' '.join(M.build_parser().format_help().split())
    assert text.count('untuned placeholder') >= 4
    for doc in (P.predict_sequence_people.__doc__, ):
        doc = ' '.join(doc.split())
        assert 'untuned placeholders' in doc and 'has not been measured' in doc


def test_people_entry_points_refuse_what_is_out_of_scope():
    with pytest.raises(ValueError, match='1..4'):
        P.predict_sequence_people(None, [np.zeros((4, 4, 3), np.uint8)], 5)
    with pytest.raises(ValueError, match='zoom'):
        P.predict_sequence_people(None, [np.zeros((4, 4, 3), np.uint8)], 2, zoom=True)
    with pytest.raises(ValueError, match='one size'):
        P.predict_sequence_people(None, [np.zeros((4, 4, 3), np.uint8), np.zeros((4, 5, 3), np.uint8)], 2)
    with pytest.raises(ValueError, match='one person'):
        P.predict_sequence(None, [np.zeros((4, 4, 3), np.uint8)], people=2)


def test_skeletons_of_tracks():
    """With 'tracks' in a result, which='track' draws one skeleton per track present in the frame, in pass order; without it, the one of 'track'."""
    K = 9
    pts = np.arange(3 * K * 2, dtype=np.float64).reshape(3, K, 2)
    r = {'size': (480, 720), 'track': {'points': pts[0], 'inside': np.ones(K, bool)},
         'tracks': {'present': np.array([True, False, True]), 'points': pts, 'inside': np.ones((3, K), bool)}}
    one = P.skeleton_primitives([{'size': (480, 720), 'track': r['track']}], which='track')
    two = P.skeleton_primitives([r], which='track')
    assert len(two) == 2 * len(one) and len(one) == len(P.SKELETON) + K
    assert_array_equal(two[:len(one)], one)
    assert_array_equal(two[len(one):], P.skeleton_primitives([{'size': (480, 720), 'track': {'points': pts[2], 'inside': np.ones(K, bool)}}], which='track'))
    doc = P.predictions_document(['f'], [dict(r, joint_names=list(P.JOINT_NAMES))])
    assert doc['images'][0]['tracks']['present'] == [True, False, True]
