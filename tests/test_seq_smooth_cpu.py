"""The restatement of the smoother (tests/seq_smooth_ref.py) against the enumeration of all paths and hand-made cases, the M-step of
predict.seq_fit, and the condition on the planted clip the GPU test shares.  No device is needed."""
import numpy as np
import pytest
from numpy.testing import assert_array_equal

import seq_ref as R
import seq_smooth_ref as SR
import joint_cnn_mrf_amd  # noqa: F401
from joint_cnn_mrf_amd import predict as P


def _rel(got, want):
    return float(np.max(np.abs(got - want) / np.maximum(np.abs(want), 1e-300)))


def _tiny(seed=3, T=4, HH=3, WW=4):
    rs = np.random.RandomState(seed)
    return (rs.rand(1, T, HH, WW, 1) + 0.05).astype(np.float32)


def _against_enumeration(hm, taps, rho):
    got = SR.seq_smooth(hm, taps, rho)
    gamma, trans = SR.brute_force(hm[0, :, :, :, 0], taps[0], rho)
    assert not got['reset'].any() and not got['cut'].any()
    # the restatement may differ from the enumeration only by summation order
    assert _rel(got['gamma'][0, :, :, :, 0], gamma) <= 1e-12
    want = trans.sum(axis=0)
    have = got['trans'][0, :, 0].sum(axis=0)
    assert np.all(np.abs(have - want) <= 1e-12 * np.abs(want)), (have, want)
    assert np.abs(got['mass'] - 1.0).max() <= 1e-12
    assert_array_equal(got['trans'][0, 0, 0], [0.0, 0.0, 0.0])
    return got


@pytest.mark.parametrize('radius', [1, 2])
@pytest.mark.parametrize('rho', [0.05, 0.0])
def test_against_all_paths(radius, rho):
    got = _against_enumeration(_tiny(), P.seq_taps(0.9, radius, 1), rho)
    moved, jumped = got['trans'][0, 1:, 0, 0], got['trans'][0, 1:, 0, 1]
    assert np.abs(moved + jumped - 1.0).max() <= 1e-12      # every transition either moved or jumped
    if rho == 0.0:
        assert_array_equal(jumped, np.zeros(3))


def test_asymmetric_taps_against_all_paths():
    """Taps that prefer motion towards larger rows and columns: a backward pass that indexed like the forward one would move the other way."""
    taps = np.array([[0.05, 0.25, 0.70]])
    got = _against_enumeration(_tiny(seed=4), taps, 0.05)
    mirrored = SR.brute_force(_tiny(seed=4)[0, :, :, :, 0], taps[0, ::-1], 0.05)[0]
    assert _rel(got['gamma'][0, :, :, :, 0], mirrored) > 1e-3      # the case does tell the two apart


def test_one_frame():
    hm = _tiny(T=1)
    got = SR.seq_smooth(hm, P.seq_taps(1.0, 1, 1), 0.05)
    assert_array_equal(got['gamma'], R.seq_filter(hm, P.seq_taps(1.0, 1, 1), 0.05)['belief'])
    assert_array_equal(got['trans'], np.zeros((1, 1, 1, 3)))
    assert got['cut'][0, 0, 0] == 0


def test_rho_one_forgets():
    """With rho = 1 the frames are independent: gamma_t is the normalised p_t and nothing has moved."""
    hm = _tiny()
    got = SR.seq_smooth(hm, P.seq_taps(1.0, 1, 1), 1.0)
    p = hm[0, :, :, :, 0].astype(np.float64)
    assert _rel(got['gamma'][0, :, :, :, 0], p / p.sum(axis=(1, 2), keepdims=True)) <= 1e-12
    assert_array_equal(got['trans'][0, :, 0, 0], np.zeros(4))
    assert_array_equal(got['trans'][0, :, 0, 2], np.zeros(4))
    assert np.abs(got['trans'][0, 1:, 0, 1] - 1.0).max() <= 1e-12


def test_zero_frame_splits_the_chain():
    hm = _tiny(T=5)
    hm[0, 2] = 0.0
    taps = P.seq_taps(1.0, 1, 1)
    got = SR.seq_smooth(hm, taps, 0.05)
    assert_array_equal(got['reset'][0, :, 0], [0, 0, 2, 0, 0])
    assert_array_equal(got['trans'][0, 2, 0], [0.0, 0.0, 0.0])
    assert got['trans'][0, 1, 0, 0] > 0 and got['trans'][0, 3, 0, 0] > 0
    # beta = 1 behind the zero frame: the frames before it are the smoother of their own clip
    head = SR.seq_smooth(hm[:, :2], taps, 0.05)
    assert_array_equal(got['gamma'][:, :2], head['gamma'])
    assert_array_equal(got['trans'][:, :2], head['trans'])
    assert_array_equal(got['cut'], np.zeros((1, 5, 1), np.int32))


def test_shared_cases_have_a_clear_arg_max():
    """seq_smooth_ref.case finds, for the small geometries here (the GPU test runs them all), a seed whose smoothed posteriors have a clear first
    maximum, and the limit case sits exactly at the cell limit."""
    for name in ('clipped', 'vector', 'radius0', 'rho1'):
        hm, taps, Rr, sigma, rho, seed, ref = SR.case(name)
        S, T, HH, WW, K = hm.shape
        assert (R.top2_gap(ref['gamma']) > 10.0 * R.tolerance(2 * T, HH * WW, Rr)).all() and seed < 100, name
    S, T, HH, WW = SR.CASES['limit'][:4]
    assert HH * WW == SR.MAX_HW and 60 * 90 <= SR.MAX_HW


# ------------------------------------------------------------------ the M-step
def test_m_step_solves_the_moment_equation():
    for radius, target in ((16, 2.25), (16, 0.3), (16, 60.0), (5, 4.0), (1, 0.4)):
        sigma, clamped = P.seq_sigma_of_moment(target, radius)
        assert not clamped
        assert abs(P.seq_moment(sigma, radius) - target) <= 1e-12 * target, (radius, target, sigma)
    assert abs(P.seq_sigma_of_moment(P.seq_moment(1.5, 16), 16)[0] - 1.5) <= 1e-12
    d = np.arange(-3, 4, dtype=np.float64)
    assert P.seq_moment(0.8, 3) == float(np.sum(d * d * P.seq_taps(0.8, 3, 1)[0]))


def test_m_step_clamp_and_kept_sigma():
    flat = 16 * 17 / 3.0
    for target in (flat, flat + 1.0, 0.5 * (P.seq_moment(P.SEQ_SIGMA_MAX, 16) + flat)):
        assert P.seq_sigma_of_moment(target, 16) == (P.SEQ_SIGMA_MAX, True)
    trans = np.array([[4.0, 1.0, 4.0 * 2 * P.seq_moment(2.0, 16)], [0.0, 0.5, 0.0], [2.0, 0.5, 2.0 * 2 * (flat + 3.0)]])
    sigma, rho, clamped = P.seq_m_step(trans, [1.0, 1.3, 1.0], 0.05, 16)
    assert abs(sigma[0] - 2.0) <= 1e-12 and sigma[1] == 1.3 and sigma[2] == P.SEQ_SIGMA_MAX      # a joint that never moved keeps its sigma
    assert_array_equal(clamped, [False, False, True])
    assert rho == 2.0 / 8.0
    assert P.seq_m_step(trans, [1.0, 1.3, 1.0], 0.05, 16, fit_rho=False)[1] == 0.05


# ------------------------------------------------------------------ the planted clip
def test_planted_clip_recovers():
    hm, fit, seed = SR.planted_case()
    c = SR.PLANTED
    planted, start = np.array(c['sigma']), c['start'] * np.array(c['sigma'])
    print('seed %d: sigma %s -> %s (planted %s), rho %.4f, loglik %s' % (seed, start, fit['sigma'], planted, fit['rho'], fit['loglik']))
    assert (np.abs(fit['sigma'] - planted) < np.abs(start - planted)).all()
    assert (np.diff(fit['loglik']) >= -SR.loglik_rounding(hm, c['radius'])).all()
    assert fit['loglik'].shape == (c['iters'] + 1,) and len(fit['history']) == c['iters'] + 1 and not fit['clamped'].any()
    assert 0.0 < fit['rho'] < 1.0


# ------------------------------------------------------------------ rendered clips (synth.people_clip)
@pytest.fixture(scope='module')
def poses():
    import os
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'flic_train_xy.npy'))


def test_people_clip_frame_0_is_people_scene(poses):
    from joint_cnn_mrf_amd import synth
    a, b = np.random.RandomState(4), np.random.RandomState(4)
    rec, prims, xy = synth.people_scene(a, poses[10], poses[20])
    recs, cprims, cxy = synth.people_clip(b, poses[10], poses[11], 5, poses[20])
    n = int(recs[0, 16])
    assert_array_equal(recs[0], rec)
    assert_array_equal(cprims[:n], prims)
    assert_array_equal(cxy[0], xy)
    assert a.randint(0, 2 ** 31 - 1) == b.randint(0, 2 ** 31 - 1)      # the generator is left where people_scene leaves it
    assert recs.shape == (5, synth.SYNTH_REC_INTS) and cxy.shape == (5, 2, 9) and cprims.shape == (int(recs[:, 16].sum()), synth.SYNTH_PRIM_INTS)
    assert_array_equal(recs[:, 17], np.concatenate([[0], np.cumsum(recs[:-1, 16])]))


def test_people_clip_moves_one_person_and_nothing_else(poses):
    from joint_cnn_mrf_amd import synth
    T = 6
    recs, prims, xy = synth.people_clip(np.random.RandomState(7), poses[100], poses[2000], T, poses[30])
    frames = [prims[int(r[17]):int(r[17]) + int(r[16])] for r in recs]
    person = 13      # _figure lists 13 primitives; the annotated person is listed last
    assert (xy[1:] != xy[0]).any()
    for t in range(1, T):
        assert_array_equal(np.delete(recs[t], 17), np.delete(recs[0], 17))      # the background and the sensor noise are the scene's
        assert frames[t].shape == frames[0].shape
        assert_array_equal(frames[t][:-person], frames[0][:-person])      # the second person and the clutter stand still
        assert_array_equal(frames[t][-person:, 0], frames[0][-person:, 0])      # the look: kinds (the listing order), colours, texture
        assert_array_equal(frames[t][-person:, 9:15], frames[0][-person:, 9:15])
    assert (frames[T - 1][-person:, 1:9] != frames[0][-person:, 1:9]).any()
    # the joints are collinear in t, equally spaced, and inside the frame
    step = xy[1] - xy[0]
    for t in range(T):
        assert np.abs(xy[t] - (xy[0] + t * step)).max() <= 1e-9
        assert (xy[t][0] >= 0).all() and (xy[t][0] <= 719).all() and (xy[t][1] >= 0).all() and (xy[t][1] <= 479).all()


def test_people_clip_cut_starts_a_new_scene(poses):
    from joint_cnn_mrf_amd import synth
    recs, prims, xy = synth.people_clip(np.random.RandomState(9), poses[5], poses[6], 6, poses[40], cuts=(3,))
    same = synth.people_clip(np.random.RandomState(9), poses[5], poses[6], 6, poses[40])
    for t in range(3):      # up to the cut the clip is the clip without it
        assert_array_equal(np.delete(recs[t], 17), np.delete(same[0][t], 17))
        assert_array_equal(xy[t], same[2][t])
    assert (recs[3, :16] != recs[2, :16]).any() and (xy[3] != same[2][3]).any()
    assert_array_equal(recs[4, :16], recs[3, :16])
    assert_array_equal(np.delete(recs[5], 17)[:16], recs[3, :16])
    for bad in ((0,), (6,), (-1,)):
        with pytest.raises(ValueError):
            synth.people_clip(np.random.RandomState(9), poses[5], poses[6], 6, cuts=bad)
    with pytest.raises(TypeError):
        synth.people_clip(np.random.RandomState(9), poses[5], poses[6], 2, colour=3)
    one = synth.people_clip(np.random.RandomState(9), poses[5], poses[6], 1)
    assert one[0].shape[0] == 1
