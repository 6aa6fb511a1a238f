"""Camera pans without a device: the numpy restatement of jcm_frame_shift (tests/frame_shift_ref.py) is held to a second,
independent formulation -- plain Python loops over candidates and pixels, on tiny frames -- and to the pans it must recover exactly;
motion.camera_shifts, the rules of --seq_camera and the geometry of dataset.render_clip_pan's crops are checked on host arrays."""
import argparse

import numpy as np
import pytest
from numpy.testing import assert_array_equal

import frame_shift_ref as FR
import joint_cnn_mrf_amd  # noqa: F401
from joint_cnn_mrf_amd import _lib, dataset, motion
from joint_cnn_mrf_amd import main as M
from joint_cnn_mrf_amd import predict as P


# ------------------------------------------------------------------ the restatement against brute force
def _brute(cur, prv, rect, D):
    """jcm_frame_shift of one pair as include/jcm.h words it, in Python loops on lists of ints."""
    y0, x0, ch, cw = rect
    lum = lambda f: [[int(f[y][x][0]) + 2 * int(f[y][x][1]) + int(f[y][x][2]) for x in range(f.shape[1])] for y in range(f.shape[0])]
    Lt, Lp = lum(cur), lum(prv)
    Hc, Wc = ch // 4, cw // 4
    blocks = lambda L: [[sum(L[y0 + 4 * Y + j][x0 + 4 * X + i] for j in range(4) for i in range(4)) for X in range(Wc)] for Y in range(Hc)]
    Ct, Cp = blocks(Lt), blocks(Lp)
    best = None
    for dy in range(-D, D + 1):
        for dx in range(-D, D + 1):
            s = sum(abs(Ct[Y][X] - Cp[Y + dy][X + dx]) for Y in range(D, Hc - D) for X in range(D, Wc - D))
            key = (s, dy * dy + dx * dx, dy, dx)
            best = key if best is None or key < best else best
    cy, cx = best[2], best[3]
    m = 4 * D + 3

    def fine(dy, dx):
        return sum(abs(Lt[y][x] - Lp[y + dy][x + dx]) for y in range(y0 + m, y0 + ch - m) for x in range(x0 + m, x0 + cw - m))

    best = None
    for ey in range(-3, 4):
        for ex in range(-3, 4):
            dy, dx = 4 * cy + ey, 4 * cx + ex
            key = (fine(dy, dx), dy * dy + dx * dx, dy, dx)
            best = key if best is None or key < best else best
    return (best[2], best[3]), (best[0], fine(0, 0))


@pytest.mark.parametrize('D,H,W,rect', [(1, 24, 40, (3, 5, 15, 29)), (1, 20, 22, (0, 0, 20, 22)), (2, 30, 33, (2, 3, 25, 27))])
def test_restatement_equals_brute_force(D, H, W, rect):
    rng = np.random.default_rng(D * 100 + H)
    m = 4 * D + 3
    canvas = FR.pan_canvas(rng, H + 4 * m, W + 4 * m, box=3)
    pans = [(0, 0), (1, -2), (-3, 0), (m, -m)]
    x = FR.pan_frames(canvas, H, W, (2 * m, 2 * m), pans)
    noise = rng.integers(0, 256, size=x.shape).astype(np.uint8)      # and frames that match nowhere: the tie rules and the coarse winner decide
    for frames in (x, noise):
        disp, sad = FR.frame_shift(frames, rect, D)
        assert tuple(disp[0]) == (0, 0) and tuple(sad[0]) == (0, 0)
        for t in range(1, len(frames)):
            d, s = _brute(frames[t], frames[t - 1], rect, D)
            assert (tuple(disp[t]), tuple(sad[t])) == (d, s), t
    assert disp.dtype == np.int32 and sad.dtype == np.int64


@pytest.mark.parametrize('D,H,W,rect', [(1, 48, 60, (3, 5, 41, 50)), (2, 64, 80, (0, 0, 64, 80)), (4, 96, 128, (6, 9, 85, 111))])
def test_restatement_recovers_every_known_pan(D, H, W, rect):
    x, pans = FR.pan_clip(D, H, W)
    disp, sad = FR.frame_shift(x, rect, D)
    assert_array_equal(disp[1:], np.array(pans))
    assert (sad[1:, 0] == 0).all() and (sad[2:, 1] > 0).all() and tuple(sad[1]) == (0, 0)


def test_ties_split_and_refusals():
    flat = np.full((3, 24, 40, 3), 77, np.uint8)
    disp, sad = FR.frame_shift(flat, (3, 5, 15, 29), 1)
    assert not disp.any() and not sad.any()
    x, _ = FR.pan_clip(1, 32, 40)
    whole = FR.frame_shift(x[:5], (1, 2, 30, 37), 1)
    a, b = FR.frame_shift(x[:2], (1, 2, 30, 37), 1), FR.frame_shift(x[2:5], (1, 2, 30, 37), 1, prev=x[1])
    assert_array_equal(np.concatenate([a[0], b[0]]), whole[0])
    assert_array_equal(np.concatenate([a[1], b[1]]), whole[1])
    for T, H, W, rect, D in ((0, 24, 40, (3, 5, 15, 29), 1), (1, 24, 40, (3, 5, 15, 29), 0), (1, 24, 40, (3, 5, 15, 29), 17), (1, 24, 40, (3, 5, 14, 29), 1),
                             (1, 24, 40, (3, 5, 15, 14), 1), (1, 24, 40, (10, 5, 15, 29), 1), (1, 24, 40, (3, 12, 15, 29), 1), (1, 24, 40, (-1, 5, 15, 29), 1),
                             (1, 4097, 40, (3, 5, 15, 29), 1), (1, 2100, 2100, (3, 5, 15, 29), 1)):
        with pytest.raises(ValueError):
            FR.check_args(T, H, W, rect, D)
    FR.check_args(1, 2048, 2048, (0, 0, 2048, 2048), 16)      # 2048 * 2048 * 1020 < 2^32
    assert 'jcm_frame_shift' in _lib.SIGNATURES and hasattr(_lib.load(), 'jcm_frame_shift')


# ------------------------------------------------------------------ motion.camera_shifts
def test_camera_shifts_round_the_cumulative_displacement():
    rng = np.random.default_rng(3)
    disp = rng.integers(-35, 36, size=(40, 2))
    shift, carry = motion.camera_shifts(disp)
    c = np.cumsum(disp, axis=0)
    o = np.floor((c + 4) / 8.0).astype(np.int64)
    assert shift.dtype == np.int32 and shift.shape == (40, 2)
    assert_array_equal(np.cumsum(shift, axis=0), o)                       # never more than half a cell off, however long the clip
    assert (np.abs(c - 8 * o) <= 4).all() and carry == tuple(int(v) for v in (c[-1] - 8 * o[-1]))
    for cut in (1, 7, 39):                                                # any split, the carry handed on
        a, ca = motion.camera_shifts(disp[:cut])
        b, cb = motion.camera_shifts(disp[cut:], ca)
        assert_array_equal(np.concatenate([a, b]), shift)
        assert cb == carry
    one = []
    cr = (0, 0)
    for d in disp:
        s, cr = motion.camera_shifts(d[None, :], cr)
        one.append(s[0])
    assert_array_equal(np.array(one), shift)
    # a steady pan of 3 pixels a frame: 3 cells in 8 frames, not 0 (each frame rounded alone) and not 8
    s, _ = motion.camera_shifts(np.array([[3, -3]] * 8))
    assert tuple(s.sum(axis=0)) == (3, -3) and set(np.unique(s)) <= {-1, 0, 1}
    assert_array_equal(motion.camera_shifts(np.array([[-4, 4], [-1, 0]]))[0], [[0, 1], [-1, 0]])      # floor division below zero: -4 -> cell 0, -5 -> cell -1
    assert_array_equal(motion.camera_shifts(np.array([[16, -24]]), stride=8)[0], [[2, -3]])
    assert motion.camera_shifts(np.zeros((0, 2), np.int64), (3, -2)) [1] == (3, -2)
    with pytest.raises(ValueError):
        motion.camera_shifts(np.zeros((3, 2)))
    with pytest.raises(ValueError):
        motion.camera_shifts(np.zeros((3, 3), np.int64))
    assert P.camera_shifts is motion.camera_shifts and P.SEQ_CAMERA_SEARCH == 8 and P.SEQ_CAMERA_MODES == ('filter', 'viterbi')


# ------------------------------------------------------------------ the command line
PREDICT = ['--synthetic', '--debug', '--predict', 'a.npy', '--predictions', 'o.json']
REFUSALS = (
    (['--seq_camera'] + PREDICT, 'SEQ_CAMERA_NEEDS_SEQUENCE'),
    (['--seq_camera', '--sequence', 'marginal'] + PREDICT, 'SEQ_CAMERA_NO_SMOOTHER'),
    (['--seq_camera', '--sequence', 'lag', '--seq_lag', '2'] + PREDICT, 'SEQ_CAMERA_NO_SMOOTHER'),
    (['--seq_camera', '--sequence', 'filter', '--seq_fit', '3'] + PREDICT, 'SEQ_CAMERA_NO_FIT'),
    (['--seq_camera', '--sequence', 'viterbi', '--use_sm', '--seq_zoom'] + PREDICT, 'SEQ_CAMERA_NO_ZOOM'),
    (['--seq_camera', '--sequence', 'viterbi', '--use_sm', '--seq_people', '2'] + PREDICT, 'SEQ_CAMERA_NO_PEOPLE'),
    (['--seq_camera_search', '4', '--sequence', 'filter'] + PREDICT, 'SEQ_CAMERA_SEARCH_NEEDS_SEQ_CAMERA'),
    # an earlier table wins over the new one, with its message
    (['--seq_camera', '--sequence', 'viterbi'], 'SEQUENCE_NEEDS_PREDICT'),
    (['--seq_camera', '--sequence', 'lag'] + PREDICT, 'SEQ_LAG_NEEDS_SEQ_LAG'),
    (['--seq_camera', '--seq_zoom', '--use_sm'] + PREDICT, 'SEQ_ZOOM_NEEDS_SEQUENCE'),
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


def test_camera_rules_are_a_table_behind_the_others():
    new = [m for _, m in M.SEQ_CAMERA_RULES if not callable(m)]
    assert len(new) == len(set(new)) == 6 and len(M.SEQ_CAMERA_RULES) == 7
    earlier = M.FLAG_RULES + M.SEQUENCE_RULES + M.AUGM_RULES + M.SEQ_PEOPLE_RULES + M.SYNTH_PEOPLE_RULES + M.SEQ_SMOOTH_RULES + M.SEQ_ZOOM_RULES + M.SEQ_LAG_RULES
    assert not set(new) & {m for _, m in earlier if not callable(m)}
    args = M.build_parser().parse_args([])
    assert not args.seq_camera and args.seq_camera_search is None
    for bad in ('0', '17'):
        assert _refusal(['--seq_camera', '--seq_camera_search', bad, '--sequence', 'filter'] + PREDICT) == '--seq_camera_search %s: 1 <= D <= 16' % bad
    for mode in ('filter', 'viterbi'):      # an accepted combination passes every rule and stops at the device check
        assert '--gpus' in str(_refusal(['--seq_camera', '--seq_camera_search', '4', '--sequence', mode] + PREDICT))


def test_entry_points_refuse_what_has_no_moving_form():
    frames = [np.zeros((4, 4, 3), np.uint8)]
    for kw in ({'mode': 'marginal'}, {'mode': 'lag', 'lag': 2}, {'fit_iters': 3}):
        with pytest.raises(ValueError, match='moving form'):
            P.predict_sequence(None, frames, camera=True, **kw)
    for search in (0, 17):
        with pytest.raises(ValueError, match='camera_search'):
            P.predict_sequence(None, frames, camera=True, camera_search=search)
        with pytest.raises(ValueError, match='camera_search'):
            P.SequenceTracker(None, camera=True, camera_search=search)
    with pytest.raises(ValueError, match='camera'):
        P.predict_sequence_zoom(None, frames, camera=True)
    with pytest.raises(ValueError, match='camera'):
        P.predict_sequence_people(None, frames, 2, camera=True)
    with pytest.raises(ValueError, match='keep_maps'):
        P.predict_images(None, frames, keep_frames=True)


# ------------------------------------------------------------------ the crops of a panned clip
def test_pan_crops_geometry():
    T, my, mx = 5, 6, 9
    pan = np.array([[0, 0], [2, -3], [-5, 6], [0, 0], [3, 3]])
    o = dataset.pan_origins(pan, (my, mx), T)
    assert_array_equal(o, [[6, 9], [8, 6], [3, 12], [3, 12], [6, 15]])
    assert o.dtype == np.int64
    for bad in ([[7, 0]] + [[0, 0]] * 4, [[0, -10]] + [[0, 0]] * 4, [[3, 0], [3, 0], [1, 0], [0, 0], [0, 0]]):
        with pytest.raises(ValueError, match='leaves the canvas'):
            dataset.pan_origins(np.array(bad), (my, mx), T)
    with pytest.raises(ValueError):
        dataset.pan_origins(pan[:4], (my, mx), T)
    with pytest.raises(ValueError):
        dataset.pan_origins(pan.astype(np.float64), (my, mx), T)
    dataset.pan_origins(np.array([[my, mx]] + [[0, 0]] * 4), (my, mx), T)      # the last origin that fits
    H, W = 20, 30
    canvas = np.random.default_rng(5).integers(0, 256, size=(T, H + 2 * my, W + 2 * mx, 3)).astype(np.uint8)
    xy = np.zeros((T, 2, 9))
    xy[:, 0], xy[:, 1] = 12.5 + np.arange(9)[None, :] * 4, 7.25 + np.arange(9)[None, :] * 2      # (x, y) on the canvas, standing still
    x, moved, inside = dataset.crop_pan(canvas, xy, o, H, W)
    assert x.shape == (T, H, W, 3) and x.flags['C_CONTIGUOUS']
    for t in range(T):
        assert_array_equal(x[t], canvas[t, o[t, 0]:o[t, 0] + H, o[t, 1]:o[t, 1] + W])
        assert_array_equal(moved[t, 0], xy[t, 0] - o[t, 1])
        assert_array_equal(moved[t, 1], xy[t, 1] - o[t, 0])
        assert_array_equal(inside[t], (moved[t, 0] >= 0) & (moved[t, 0] <= W - 1) & (moved[t, 1] >= 0) & (moved[t, 1] <= H - 1))
    assert inside.any() and not inside.all()
    # the crops of one still canvas are frames whose displacement is the pan, with the sign of jcm_frame_shift
    still = np.broadcast_to(FR.pan_canvas(np.random.default_rng(6), 48 + 2 * my, 64 + 2 * mx, box=9), (T, 48 + 2 * my, 64 + 2 * mx, 3))
    frames, _, _ = dataset.crop_pan(still, xy, o, 48, 64)
    disp, sad = FR.frame_shift(frames, (0, 0, 48, 64), 2)
    assert_array_equal(disp[1:], pan[1:])
    assert not sad[1:, 0].any()
