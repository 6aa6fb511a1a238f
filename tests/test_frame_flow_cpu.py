"""Local motion without a device: the numpy restatements of jcm_frame_flow and jcm_hm_flow_pool (tests/frame_flow_ref.py) are held
to second, independent formulations -- plain Python loops over cells, candidates and pixels -- and to what they must recover exactly: a planted
motion, rest on uniform and identical frames, bars without a say, and the pooling's closed cases.  motion.flow_refs / flow_weights, the rules of
--seq_flow and the refusals of the prediction layer are checked on host values."""
import argparse

import numpy as np
import pytest
from numpy.testing import assert_array_equal

import frame_flow_ref as FF
import joint_cnn_mrf_amd  # noqa: F401
from joint_cnn_mrf_amd import _lib, motion
from joint_cnn_mrf_amd import main as M
from joint_cnn_mrf_amd import predict as P


# ------------------------------------------------------------------ the restatement against brute force
def _brute_flow(x, rect, D, ref):
    """jcm_frame_flow as include/jcm.h words it: per slot, cell and candidate a sum over the pixels of P, the winner by min() on tuples."""
    T, H, W = x.shape[:3]
    y0, x0, ch, cw = rect
    HH, WW, R = H // 8, W // 8, ref.shape[1]
    lum = [[[int(f[y][q][0]) + 2 * int(f[y][q][1]) + int(f[y][q][2]) for q in range(W)] for y in range(H)] for f in x]
    flow, sad = np.zeros((T, R, HH, WW, 2), np.int32), np.zeros((T, R, HH, WW, 2), np.int32)
    for t in range(T):
        for r in range(R):
            s = int(ref[t, r])
            if not 0 <= s < T:
                continue
            for Y in range(HH):
                for X in range(WW):
                    ys = [y for y in range(8 * Y - 4, 8 * Y + 12) if y0 <= y < y0 + ch]
                    xs = [q for q in range(8 * X - 4, 8 * X + 12) if x0 <= q < x0 + cw]
                    if not ys or not xs:
                        continue
                    cands = []
                    for dy in range(-D, D + 1):
                        for dx in range(-D, D + 1):
                            if ys[0] + dy < y0 or ys[-1] + dy >= y0 + ch or xs[0] + dx < x0 or xs[-1] + dx >= x0 + cw:
                                continue
                            S = sum(abs(lum[t][y][q] - lum[s][y + dy][q + dx]) for y in ys for q in xs)
                            cands.append((S, dy * dy + dx * dx, dy, dx))
                    best = min(cands)
                    flow[t, r, Y, X] = best[2:]
                    sad[t, r, Y, X] = (best[0], next(c[0] for c in cands if c[2] == 0 and c[3] == 0))
    return flow, sad


@pytest.mark.parametrize('kind', ['noise', 'smooth'])
def test_restatement_equals_brute_force(kind):
    """24 x 32 frames (3 x 4 cells), a rectangle that cuts cells on every side and leaves a column of cells in a bar, D = 2, an absent slot."""
    x = FF.noise_clip(3, 24, 32, 1) if kind == 'noise' else FF.smooth_clip(3, 24, 32, 2)
    rect, ref = (2, 3, 19, 17), np.array([[1, -1], [2, 0], [3, 1]], np.int32)
    got, want = FF.frame_flow(x, rect, 2, ref), _brute_flow(x, rect, 2, ref)
    assert_array_equal(got[0], want[0])
    assert_array_equal(got[1], want[1])
    assert got[0].dtype == np.int32 and got[1].dtype == np.int32 and got[0].shape == (3, 2, 3, 4, 2)
    assert not got[0][:, :, :, 3].any() and not got[1][:, :, :, 3].any()      # cells wholly in the bar
    assert not got[0][0, 1].any() and not got[0][2, 0].any()                  # ref < 0 and ref >= T
    assert got[1][1, 0].any()


def test_planted_motion_is_recovered():
    x = FF.planted_pair()
    flow, sad = FF.frame_flow(x, FF.PLANT_RECT, FF.PLANT_D, np.array([[1], [0]], np.int32))
    inside, far = FF.planted_cells()
    assert inside[0].sum() >= 4 and inside[1].sum() >= 4 and far[0].sum() >= 8
    for f, sign in ((0, 1), (1, -1)):
        assert (flow[f, 0][inside[f]] == sign * np.array(FF.PLANT_MOVE)).all()
        assert not sad[f, 0][inside[f]][:, 0].any() and sad[f, 0][inside[f]][:, 1].all()
        assert not flow[f, 0][far[f]].any() and not sad[f, 0][far[f]].any()


def test_uniform_and_identical_frames_rest():
    flat = np.full((2, 40, 56, 3), 77, np.uint8)
    flat[:, :3] = 200
    ref = np.array([[1], [0]], np.int32)
    for x in (flat, np.stack([FF.noise_clip(1, 40, 56, 3)[0]] * 2)):
        flow, sad = FF.frame_flow(x, (3, 5, 30, 41), 3, ref)
        assert not flow.any() and not sad.any()


def test_bars_have_no_say():
    x, rect, D, ref = FF.flow_case('cut on every side')
    want = FF.flow_case_expected('cut on every side')
    y = np.random.default_rng(4).integers(0, 256, size=x.shape).astype(np.uint8)
    y0, x0, ch, cw = rect
    y[:, y0:y0 + ch, x0:x0 + cw] = x[:, y0:y0 + ch, x0:x0 + cw]
    got = FF.frame_flow(y, rect, D, ref)
    assert_array_equal(got[0], want[0])
    assert_array_equal(got[1], want[1])


def test_case_table_reaches_the_paths_it_names():
    """What the shared cases are there for, asserted on the restatement so that a change of the table cannot quietly lose it."""
    flow, sad = FF.flow_case_expected('cut on every side')
    assert sad[0, 0, 4, :, 1].all() and sad[0, 0, :, 6, 1].all()      # cells wholly in a bar whose blocks still reach into the rectangle: 5 rows, 2 columns
    assert len({tuple(v) for v in flow.reshape(-1, 2)}) > 8
    flow, sad = FF.flow_case_expected('only (0,0) is valid')
    assert sad[:, :, 2, 3, 0].all() and not flow[:, :, 2, 3].any() and not sad[:, :, 0].any() and not sad[:, :, :, 5:].any()      # and cells with no pixel at all
    flow, _ = FF.flow_case_expected('a column of valid dx')
    assert (flow[:, :, 1, :, 0] >= 0).all() and (flow[:, :, 2, :, 0] <= 0).all() and flow[..., 1].any()
    for name, D in (('D = 1', 1), ('D = 16', 16)):
        flow, _ = FF.flow_case_expected(name)
        assert np.abs(flow).max() <= D
    assert np.abs(FF.flow_case_expected('D = 16')[0]).max() > 8
    flow, sad = FF.flow_case_expected('a ref entry >= T is absent')
    assert not flow[0, 0].any() and not sad[0, 0].any() and not sad[1, 1].any() and not sad[2, 0].any() and sad[0, 1].any()
    assert not FF.flow_case_expected('T = 1, every ref negative')[1].any()
    for bad in (dict(T=0), dict(T=65535), dict(D=0), dict(D=17), dict(R=0), dict(R=9), dict(H=44), dict(W=60), dict(H=4104), dict(rect=(0, 0, 41, 56)),
                dict(rect=(-1, 0, 8, 8)), dict(rect=(0, 50, 8, 8)), dict(rect=(0, 0, 0, 8))):
        kw = dict(dict(T=2, H=40, W=56, rect=(3, 5, 30, 41), D=3, R=2), **bad)
        with pytest.raises(ValueError):
            FF.check_args(**kw)


# ------------------------------------------------------------------ the pooling
def _brute_pool(hm, flow, w):
    """jcm_hm_flow_pool as include/jcm.h words it, one Python float (float64) operation per step."""
    T, HH, WW, K = hm.shape
    N = len(w) - 1
    out = np.empty_like(hm)
    for t in range(T):
        for y in range(HH):
            for x in range(WW):
                for k in range(K):
                    acc, ws = float(w[0]) * float(hm[t, y, x, k]), float(w[0])
                    for n in range(1, N + 1):
                        for side, s in enumerate((t - n, t + n)):
                            if s < 0 or s >= T:
                                continue
                            dy, dx = (int(v) for v in flow[t, 2 * (n - 1) + side, y, x])
                            py, px = min(max(y + dy / 8.0, 0.0), HH - 1.0), min(max(x + dx / 8.0, 0.0), WW - 1.0)
                            ya, xa = int(np.floor(py)), int(np.floor(px))
                            yb, xb, fy, fx = min(ya + 1, HH - 1), min(xa + 1, WW - 1), py - ya, px - xa
                            top = (1.0 - fx) * float(hm[s, ya, xa, k]) + fx * float(hm[s, ya, xb, k])
                            bot = (1.0 - fx) * float(hm[s, yb, xa, k]) + fx * float(hm[s, yb, xb, k])
                            acc = acc + float(w[n]) * ((1.0 - fy) * top + fy * bot)
                            ws = ws + float(w[n])
                    out[t, y, x, k] = np.float32(acc / ws)
    return out


@pytest.mark.parametrize('N,T', [(1, 1), (1, 3), (2, 2), (2, 5)])
def test_pool_restatement_equals_brute_force(N, T):
    hm, flow = FF.pool_maps(T, 5, 7, 2, 10 + N), FF.pool_flow(T, N, 5, 7, 20 + T)
    w = (0.9, 0.8, 0.35)[:N + 1]
    got = FF.hm_flow_pool(hm, flow, w)
    assert got.dtype == np.float32
    assert_array_equal(got.view(np.uint32), _brute_pool(hm, flow, w).view(np.uint32))


def test_pool_closed_cases():
    T, HH, WW, K, N = 5, 5, 7, 3, 2
    hm = FF.pool_maps(T, HH, WW, K, 31)
    zero = np.zeros((T, 2 * N, HH, WW, 2), np.int32)
    w = np.array([0.5, 0.25, 2.0])
    got = FF.hm_flow_pool(hm, zero, w)
    h = hm.astype(np.float64)
    want2 = (((((w[0] * h[2] + w[1] * h[1]) + w[1] * h[3]) + w[2] * h[0]) + w[2] * h[4]) / ((((w[0] + w[1]) + w[1]) + w[2]) + w[2])).astype(np.float32)
    assert_array_equal(got[2], want2)                                   # zero flow: the weighted mean, in the stated order
    want0 = (((w[0] * h[0] + w[1] * h[1]) + w[2] * h[2]) / ((w[0] + w[1]) + w[2])).astype(np.float32)
    assert_array_equal(got[0], want0)                                   # the neighbours before frame 0 are skipped, weights and all
    assert_array_equal(FF.hm_flow_pool(hm, FF.pool_flow(T, N, HH, WW, 32), (1.0, 0.0, 0.0)).view(np.uint32), hm.view(np.uint32))      # w = [1, 0, ..]: hm's bits
    # a one-cell delta that moves by one cell a frame: a flow of exactly 8 pixels pools it onto the frame's own cell
    delta = np.zeros((3, HH, WW, 1), np.float32)
    for t in range(3):
        delta[t, 2, 2 + t, 0] = 1.0
    flow = np.zeros((3, 2, HH, WW, 2), np.int32)
    flow[:, 0, :, :, 1], flow[:, 1, :, :, 1] = -8, 8                    # the content of frame t is one cell to the left in t-1, to the right in t+1
    got = FF.hm_flow_pool(delta, flow, (1.0, 1.0))
    assert got[1, 2, 3, 0] == 1.0 and got[1].sum() == 1.0
    flow[:, 0, :, :, 1], flow[:, 1, :, :, 1] = -4, 4                    # four pixels: half a cell, the sample splits half and half
    got = FF.hm_flow_pool(delta, flow, (1.0, 1.0))
    assert got[1, 2, 3, 0] == np.float32((1.0 + 0.5 + 0.5) / 3.0) and got[1, 2, 2, 0] == np.float32(0.5 / 3.0) and got[1, 2, 4, 0] == np.float32(0.5 / 3.0)
    # the upper neighbour index is clamped: at the last row and column the sample is the edge value itself
    edge = FF.pool_maps(2, HH, WW, 1, 33)
    flow = np.full((2, 2, HH, WW, 2), 1000, np.int32)
    got = FF.hm_flow_pool(edge, flow, (1.0, 1.0))
    e = edge.astype(np.float64)
    assert_array_equal(got[0], np.broadcast_to(((e[0] + e[1, HH - 1, WW - 1]) / 2.0).astype(np.float32), got[0].shape))
    # the order of the sum, t - n before t + n, decides the result where one term cancels another that absorbs the third
    hm, flow, w = FF.order_case()
    got = FF.hm_flow_pool(hm, flow, w)
    assert (got[1] == np.float32(1.0 / 3.0)).all()
    assert_array_equal(got.view(np.uint32), _brute_pool(hm, flow, w).view(np.uint32))
    for bad in ((0.0, 1.0), (1.0, -0.5), (1.0, float('nan')), (1.0, float('inf')), (1.0,), (1.0,) * 6):
        with pytest.raises(ValueError):
            FF.check_weights(bad)


# ------------------------------------------------------------------ motion.flow_refs, motion.flow_weights, the binding
def test_flow_refs_and_weights():
    for T, N in ((1, 1), (2, 4), (9, 4), (5, 2)):
        ref = motion.flow_refs(T, N)
        assert ref.dtype == np.int32 and ref.shape == (T, 2 * N)
        assert_array_equal(ref, FF.flow_refs(T, N))
    assert_array_equal(motion.flow_refs(3, 1), [[-1, 1], [0, 2], [1, -1]])
    assert_array_equal(motion.flow_weights(3), np.ones(4))
    assert motion.flow_weights(3).dtype == np.float64
    for bad in (0, 5, True, 1.0):
        with pytest.raises(ValueError):
            motion.flow_refs(4, bad)
        with pytest.raises(ValueError):
            motion.flow_weights(bad)
    with pytest.raises(ValueError):
        motion.flow_refs(0, 1)
    assert P.flow_refs is motion.flow_refs and P.flow_weights is motion.flow_weights and P.SEQ_FLOW_SEARCH == motion.SEQ_FLOW_SEARCH == 8
    assert P.SEQ_FLOW_MAX == 4 and P.SEQ_FLOW_MODES == ('filter', 'viterbi', 'marginal')
    assert len(_lib.SIGNATURES['jcm_frame_flow'][1]) == 14 and len(_lib.SIGNATURES['jcm_hm_flow_pool'][1]) == 10


# ------------------------------------------------------------------ the command line
PREDICT = ['--synthetic', '--debug', '--predict', 'a.npy', '--predictions', 'o.json']
REFUSALS = (
    (['--seq_flow', '2'] + PREDICT, 'SEQ_FLOW_NEEDS_SEQUENCE', ('--seq_flow', '--sequence')),
    (['--seq_flow', '2', '--sequence', 'lag', '--seq_lag', '2'] + PREDICT, 'SEQ_FLOW_NO_LAG', ('--seq_flow', '--sequence lag')),
    (['--seq_flow', '2', '--sequence', 'viterbi', '--use_sm', '--seq_zoom'] + PREDICT, 'SEQ_FLOW_NO_ZOOM', ('--seq_flow', '--seq_zoom')),
    (['--seq_flow', '2', '--sequence', 'viterbi', '--use_sm', '--seq_people', '2'] + PREDICT, 'SEQ_FLOW_NO_PEOPLE', ('--seq_flow', '--seq_people')),
    (['--seq_flow_search', '4', '--sequence', 'filter'] + PREDICT, 'SEQ_FLOW_SEARCH_NEEDS_SEQ_FLOW', ('--seq_flow_search', '--seq_flow N')),
    # an earlier table wins over the new one, with its message
    (['--seq_flow', '2', '--sequence', 'viterbi'], 'SEQUENCE_NEEDS_PREDICT', ()),
    (['--seq_flow', '2', '--sequence', 'lag'] + PREDICT, 'SEQ_LAG_NEEDS_SEQ_LAG', ()),
    (['--seq_flow', '2', '--seq_camera'] + PREDICT, 'SEQ_CAMERA_NEEDS_SEQUENCE', ()),
)


def _refusal(argv):
    keep = argparse.Namespace(**vars(M.hps))
    try:
        with pytest.raises(SystemExit) as ei:
            M.main(list(argv) + ['--gpus', '99'])
    finally:
        M.hps = keep
    return ei.value.code


@pytest.mark.parametrize('argv,name,flags', REFUSALS)
def test_cli_refusals(argv, name, flags):
    message = _refusal(argv)
    assert message == getattr(M, name)
    for flag in flags:      # the message names both flags
        assert flag in message


def test_flow_rules_are_a_table_behind_the_others():
    new = [m for _, m in M.SEQ_FLOW_RULES if not callable(m)]
    assert len(new) == len(set(new)) == 5 and len(M.SEQ_FLOW_RULES) == 7
    earlier = (M.FLAG_RULES + M.SEQUENCE_RULES + M.AUGM_RULES + M.SEQ_PEOPLE_RULES + M.SYNTH_PEOPLE_RULES + M.SEQ_SMOOTH_RULES + M.SEQ_ZOOM_RULES + M.SEQ_LAG_RULES +
               M.SEQ_CAMERA_RULES + M.EVAL_SCALE_RULES)
    assert not set(new) & {m for _, m in earlier if not callable(m)}
    args = M.build_parser().parse_args([])
    assert args.seq_flow is None and args.seq_flow_search is None      # no default: none has been tuned
    for bad in ('0', '5'):
        assert _refusal(['--seq_flow', bad, '--sequence', 'filter'] + PREDICT) == '--seq_flow %s: 1 <= N <= 4' % bad
    for bad in ('0', '17'):
        assert _refusal(['--seq_flow', '1', '--seq_flow_search', bad, '--sequence', 'filter'] + PREDICT) == '--seq_flow_search %s: 1 <= D <= 16' % bad
    accepted = [['--sequence', 'filter'], ['--sequence', 'viterbi', '--seq_camera'], ['--sequence', 'marginal', '--seq_fit', '3'], ['--sequence', 'filter', '--seq_fit', '2']]
    for extra in accepted:      # an accepted combination passes every rule and stops at the device check
        assert '--gpus' in str(_refusal(['--seq_flow', '2', '--seq_flow_search', '4'] + extra + PREDICT))


def test_entry_points_refuse_what_flow_cannot_take():
    frames = [np.zeros((4, 4, 3), np.uint8)]
    with pytest.raises(ValueError, match='lag has not yet seen'):
        P.predict_sequence(None, frames, mode='lag', lag=2, flow=1)
    for bad in (5, -1, True, 1.5):
        with pytest.raises(ValueError, match='flow must be'):
            P.predict_sequence(None, frames, flow=bad)
    for search in (0, 17):
        with pytest.raises(ValueError, match='flow_search'):
            P.predict_sequence(None, frames, flow=2, flow_search=search)
    for w in ((1.0, 1.0), (0.0, 1.0, 1.0), (1.0, -1.0, 1.0), (1.0, float('nan'), 1.0)):
        with pytest.raises(ValueError, match='flow_weights'):
            P.predict_sequence(None, frames, flow=2, flow_weights=w)
    with pytest.raises(ValueError, match='flow_weights'):
        P.predict_sequence(None, frames, flow_weights=(1.0, 1.0))
    from joint_cnn_mrf_amd.predict.clips import _check_flow
    assert _check_flow(0, 0, None) == (0, None, None)      # off: the radius belongs to flow = N >= 1 and is not looked at
    N, D, w = _check_flow(2, 16, None)
    assert (N, D) == (2, 16) and w.tolist() == [1.0, 1.0, 1.0]
    with pytest.raises(ValueError, match='flow'):
        P.predict_sequence_zoom(None, frames, flow=1)
    with pytest.raises(ValueError, match='flow'):
        P.predict_sequence_people(None, frames, 2, flow=1)
    for tracker in (P.SequenceTracker, P.LagTracker, P.PeopleTracker):      # the online forms do not take it
        import inspect
        assert 'flow' not in inspect.signature(tracker.__init__).parameters
