"""The fixed-lag smoother without a device: the restatement of its definition (tests/seq_lag_ref.py) is pinned -- against the
enumeration of all paths of the TRUNCATED chain, which knows no recursion and no window, and against the offline restatement where the lag spans
the clip --, the emitted counts of the push schedules, the inputs the GPU tests share, and the rules of --sequence lag on the command line."""
import argparse
import ctypes

import numpy as np
import pytest
from numpy.testing import assert_array_equal

import seq_lag_ref as LR
import seq_ref as R
import seq_smooth_ref as SR
import joint_cnn_mrf_amd  # noqa: F401
from joint_cnn_mrf_amd import _lib
from joint_cnn_mrf_amd import main as M
from joint_cnn_mrf_amd import predict as P

TINY = (1, 4, 2, 3, 1)      # T = 4, 2 x 3 cells: 6^4 paths


def _tiny(seed):
    return (np.random.RandomState(seed).rand(*TINY) + 0.05).astype(np.float32)


@pytest.mark.parametrize('L', (1, 2))
@pytest.mark.parametrize('taps', ('gauss', 'asymmetric'))
def test_against_all_paths_of_the_truncated_chain(L, taps):
    hm = _tiny(5)
    w = P.seq_taps(0.8, 1, 1) if taps == 'gauss' else np.array([[0.1, 0.3, 0.6]])
    T = TINY[1]
    got = LR.joined(LR.seq_smooth_lag(hm, w, 0.05, L, (T,)))
    assert_array_equal(got['lag'], [min(L, T - 1 - s) for s in range(T)])
    for s in range(T):
        h = min(s + L, T - 1)
        gamma, _ = SR.brute_force(hm[0, :h + 1, :, :, 0], w[0], 0.05)
        assert np.abs(got['gamma'][0, s, :, :, 0] - gamma[s]).max() < 1e-12, (s, h)
    if L == 1:      # the lag matters: frame 0 given frames 0 .. 1 is not frame 0 given the clip
        full, _ = SR.brute_force(hm[0, :, :, :, 0], w[0], 0.05)
        assert np.abs(got['gamma'][0, 0, :, :, 0] - full[0]).max() > 1e-4


@pytest.mark.parametrize('L', (3, 4, 9))
def test_a_lag_that_spans_the_clip_is_the_offline_smoother(L):
    hm = _tiny(6)
    w = P.seq_taps(0.8, 1, 1)
    want = SR.seq_smooth(hm, w, 0.05)
    got = LR.joined(LR.seq_smooth_lag(hm, w, 0.05, L, (TINY[1],)))
    for k in LR.KEYS:
        assert_array_equal(got[k], want[k], err_msg=k)


SCHEDULES = ((1, 1, 1, 1, 1, 1), (2, 4), (4, 2), (6,), (1, 5), (3, 0, 3))


@pytest.mark.parametrize('L', (1, 2, 5, 9))
@pytest.mark.parametrize('splits', SCHEDULES)
def test_emitted_counts_and_split_invariance(splits, L):
    hm = R.random_maps((1, 6, 3, 4, 2), 11)
    w = P.seq_taps(1.0, 1, 2)
    pushes = LR.seq_smooth_lag(hm, w, 0.05, L, splits)
    assert [len(p['frames']) for p in pushes] == LR.emitted_counts(splits, L)
    assert sum(len(p['frames']) for p in pushes) == 6
    # without a flush a push emits the frames that are L frames old, no more
    open_end = LR.seq_smooth_lag(hm, w, 0.05, L, splits, flush_last=False)
    assert [len(p['frames']) for p in open_end] == LR.emitted_counts(splits, L, flush_last=False)
    assert sum(len(p['frames']) for p in open_end) == max(0, 6 - L)
    one = LR.joined(LR.seq_smooth_lag(hm, w, 0.05, L, (6,)))
    got = LR.joined(pushes)
    for k in LR.KEYS + ('lag',):
        assert_array_equal(got[k], one[k], err_msg=k)


def test_counts_by_hand():
    assert LR.emitted_counts((1, 1, 1, 1, 1, 1), 2) == [0, 0, 1, 1, 1, 3]
    assert LR.emitted_counts((2, 4), 2) == [0, 6]
    assert LR.emitted_counts((4, 2), 2) == [2, 4]
    assert LR.emitted_counts((4, 2), 2, flush_last=False) == [2, 2]
    assert LR.emitted_counts((1, 5), 7) == [0, 6]


@pytest.mark.parametrize('name', sorted(set(LR.CASES) - {'real', 'limit'}))
def test_shared_cases_have_a_clear_arg_max_in_every_truncation(name):
    hm, taps, Rr, sigma, rho, seed, prefixes = LR.case(name)
    S, T, HH, WW, K = hm.shape
    assert sorted(prefixes) == list(range(1, T + 1))
    for n, ref in prefixes.items():
        assert ref['gamma'].shape[1] == n
        assert (R.top2_gap(ref['gamma']) > 10.0 * R.tolerance(2 * n, HH * WW, Rr)).all(), (name, seed, n)
    assert_array_equal(hm, R.random_maps(hm.shape, 1000 + seed))


# ------------------------------------------------------------------ the command line and the entry points
PREDICT = ['--predict', 'x', '--predictions', 'o.json']
REFUSALS = (
    (['--seq_lag', '2', '--sequence', 'marginal'] + PREDICT, 'SEQ_LAG_NEEDS_SEQUENCE_LAG'),
    (['--seq_lag', '2'] + PREDICT, 'SEQ_LAG_NEEDS_SEQUENCE_LAG'),
    (['--sequence', 'lag'] + PREDICT, 'SEQ_LAG_NEEDS_SEQ_LAG'),
    (['--sequence', 'lag', '--seq_lag', '0'] + PREDICT, '--seq_lag 0: L >= 1 (lag 0 is --sequence filter)'),
    (['--sequence', 'lag', '--seq_lag', '-3'] + PREDICT, '--seq_lag -3: L >= 1 (lag 0 is --sequence filter)'),
    (['--sequence', 'lag', '--seq_lag', '2', '--use_sm', '--seq_people', '2'] + PREDICT, 'SEQ_LAG_NO_PEOPLE'),
    (['--sequence', 'lag', '--seq_lag', '2', '--use_sm', '--seq_zoom'] + PREDICT, 'SEQ_LAG_NO_ZOOM'),
    # an earlier table's message still comes first
    (['--sequence', 'lag', '--seq_lag', '2'], 'SEQUENCE_NEEDS_PREDICT'),
    (['--sequence', 'lag', '--seq_zoom'] + PREDICT, 'SEQ_ZOOM_NEEDS_USE_SM'),
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
    fixed = [m for _, m in M.SEQ_LAG_RULES if not callable(m)]
    assert fixed == [M.SEQ_LAG_NEEDS_SEQUENCE_LAG, M.SEQ_LAG_NEEDS_SEQ_LAG, M.SEQ_LAG_NO_PEOPLE, M.SEQ_LAG_NO_ZOOM] and len(M.SEQ_LAG_RULES) == 5
    earlier = M.FLAG_RULES + M.SEQUENCE_RULES + M.AUGM_RULES + M.SEQ_PEOPLE_RULES + M.SYNTH_PEOPLE_RULES + M.SEQ_SMOOTH_RULES + M.SEQ_ZOOM_RULES
    assert not set(fixed) & {m for _, m in earlier if not callable(m)}
    assert M.build_parser().parse_args([]).seq_lag is None
    # accepted combinations pass every rule and stop at the device check
    for extra in ([], ['--seq_fit', '3'], ['--render', 'out'], ['--use_sm']):
        assert '--gpus' in str(_refusal(['--sequence', 'lag', '--seq_lag', '2'] + extra + PREDICT))


def test_modes_and_keys():
    assert P.SEQ_MODES == ('filter', 'viterbi', 'marginal', 'lag')
    assert P.SEQ_KEYS['lag'] == ('coords', 'conf', 'norm', 'reset', 'cut', 'lag')
    assert P.SEQ_KEYS['marginal'] == ('coords', 'conf', 'norm', 'reset', 'cut')


def test_entry_points_refuse_what_is_out_of_scope():
    frames = [np.zeros((4, 4, 3), np.uint8)]
    with pytest.raises(ValueError, match='lag'):
        P.predict_sequence(None, frames, mode='lag')                  # the lag is required
    with pytest.raises(ValueError, match='lag'):
        P.predict_sequence(None, frames, mode='marginal', lag=2)      # and belongs to that mode alone
    with pytest.raises(ValueError, match='filter'):
        P.predict_sequence(None, frames, mode='lag', lag=0)
    with pytest.raises(ValueError, match='SequenceTracker'):
        P.LagTracker(None, 0)
    with pytest.raises(ValueError, match="'filter' or 'viterbi'"):
        P.predict_sequence_zoom(None, frames, mode='lag')
    with pytest.raises(ValueError, match="'filter' or 'viterbi'"):
        P.predict_sequence_people(None, frames, 2, mode='lag')


def test_entry_point_is_bound_exported_and_rejects_a_null_handle():
    lib = _lib.load()
    assert 'jcm_seq_smooth_lag' in _lib.SIGNATURES and hasattr(lib, 'jcm_seq_smooth_lag')
    taps = (ctypes.c_double * 3)(0.25, 0.5, 0.25)
    assert lib.jcm_seq_smooth_lag(None, None, 1, 2, 0, 5, 7, 1, taps, 1, 0.05, 1, 0, None, None, None, None, None, None, None, None) == 1      # JCM_ERR_ARG
