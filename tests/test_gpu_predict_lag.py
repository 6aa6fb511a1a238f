"""The fixed-lag smoother in --predict (predict.predict_sequence(mode='lag'), predict.LagTracker, main.py --sequence lag --seq_lag)
on the six synthetic 96x128 frames the sequence tests use."""
import json
import os

import numpy as np
import pytest
import torch
from numpy.testing import assert_array_equal

from cli_util import run_cli
import joint_cnn_mrf_amd  # noqa: F401
from joint_cnn_mrf_amd import synth
from joint_cnn_mrf_amd import predict as P
from joint_cnn_mrf_amd.evaluation import fit_to_source

pytestmark = pytest.mark.gpu
KEYS = {'size', 'joint_names', 'geom', 'pd', 'pd_inside', 'sm', 'sm_inside', 'torso_cell'}
TRACK = {'mode', 'points', 'inside', 'conf', 'norm', 'reset', 'cut', 'lag'}
LAG = 2


def _frames():
    """Six frames of one clip: a bright square drifting over a noisy background (those of test_gpu_predict_marginal.py)."""
    rs = np.random.RandomState(77)
    frames = []
    for t in range(6):
        im = rs.randint(0, 96, (96, 128, 3)).astype(np.uint8)
        im[30 + 4 * t:50 + 4 * t, 20 + 10 * t:44 + 10 * t] = 230
        frames.append(im)
    return frames


@pytest.fixture(scope='module')
def world():
    from joint_cnn_mrf_amd.engine import Engine
    p = synth.make_pd_params(debug=True)
    p.update(synth.make_sm_params(synth.synthetic_priors(), kind='init'))
    eng = Engine(device=0).load_params(p)
    frames = _frames()
    yield eng, frames, P.predict_sequence(eng, frames, mode='lag', lag=LAG, sigma=2.0, rho=0.1, batch_size=4, keep_maps=True)
    eng.close()


def _same_tracks(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert set(g['track']) == TRACK and g['track']['mode'] == 'lag'
        for k in ('points', 'inside', 'conf', 'cut', 'lag', 'norm', 'reset'):
            assert_array_equal(g['track'][k], w['track'][k], err_msg=k)


def test_lag_track_is_seq_smooth_lag_on_the_kept_maps(world):
    eng, frames, whole = world
    hm = torch.stack([r['maps']['sm'] for r in whole]).contiguous()
    seq = eng.seq_smooth_lag(hm, 2.0, 0.1, LAG, flush=True)
    torch.cuda.synchronize()
    cells = seq['coords'].cpu().numpy().transpose(0, 2, 1).astype(np.float64)
    pts, inside = fit_to_source(cells * P.STRIDE, np.array([r['geom'] for r in whole], np.int64))
    for t, g in enumerate(whole):
        assert set(g) == KEYS | {'track', 'maps'} and set(g['track']) == TRACK and g['track']['mode'] == 'lag'
        assert_array_equal(g['track']['points'], pts[t])
        assert_array_equal(g['track']['inside'], inside[t])
        for k in ('conf', 'norm', 'reset', 'cut'):
            assert_array_equal(g['track'][k], seq[k][t].cpu().numpy())
        assert g['track']['lag'] == min(LAG, 5 - t) and g['track']['conf'].shape == (9,)
    json.dumps(P.predictions_document(['f%d' % i for i in range(6)], whole))      # the document takes the track


@pytest.mark.parametrize('step', (1, 3))
def test_tracker_pushes_and_a_flush_are_one_predict_sequence(world, step):
    eng, frames, whole = world
    tracker = P.LagTracker(eng, LAG, sigma=2.0, rho=0.1, batch_size=4)
    got, counts = [], []
    for lo in range(0, 6, step):
        done = tracker.push(frames[lo:lo + step])
        counts.append(len(done))
        got += done
    assert counts == ([0, 0, 1, 1, 1, 1] if step == 1 else [1, 3]) and len(tracker.pending) == LAG
    rest = tracker.flush()
    assert len(rest) == LAG and tracker.state is None and tracker.pending == [] and tracker.flush() == []
    got += rest
    assert all('maps' not in g and set(g) == KEYS | {'track'} for g in got)
    _same_tracks(got, whole)
    for g, w in zip(got, whole):      # every earlier key keeps its value
        for k in KEYS:
            assert_array_equal(np.asarray(g[k]), np.asarray(w[k]))
    # the tracker starts a new clip after the flush
    assert tracker.push(frames[:1]) == [] and len(tracker.flush()) == 1


def test_a_spanning_lag_is_the_marginal(world):
    eng, frames, _ = world
    marg = P.predict_sequence(eng, frames, mode='marginal', sigma=2.0, rho=0.1, batch_size=4)
    for L in (5, 9):
        whole = P.predict_sequence(eng, frames, mode='lag', lag=L, sigma=2.0, rho=0.1, batch_size=4)
        tracker = P.LagTracker(eng, L, sigma=2.0, rho=0.1, batch_size=4)
        pushed = tracker.push(frames[:4]) + tracker.push(frames[4:]) + tracker.flush()
        for got in (whole, pushed):
            assert len(got) == 6
            for g, m in zip(got, marg):
                for k in ('points', 'inside', 'conf', 'cut', 'norm', 'reset'):
                    assert_array_equal(g['track'][k], m['track'][k], err_msg=k)
        assert [g['track']['lag'] for g in whole] == [5, 4, 3, 2, 1, 0]


def test_a_frame_of_another_size_raises(world):
    eng, frames, _ = world
    tracker = P.LagTracker(eng, LAG, sigma=2.0, rho=0.1, batch_size=4)
    tracker.push(frames[:2])
    with pytest.raises(ValueError, match='one size'):
        tracker.push([np.zeros((64, 128, 3), np.uint8)])
    with pytest.raises(ValueError, match='lag'):
        P.predict_sequence(eng, frames, mode='lag')
    with pytest.raises(ValueError, match='lag'):
        P.predict_sequence(eng, frames, mode='filter', lag=2)


def test_cli_lag_with_render(world, tmp_path):
    eng, frames, whole = world
    d = tmp_path / 'clip'
    d.mkdir()
    for i, im in enumerate(frames):
        np.save(str(d / ('frame%02d.npy' % i)), im)
    out, pics = str(tmp_path / 'track.json'), str(tmp_path / 'pics')
    res = run_cli(['--synthetic', '--debug', '--use_sm', '--gpus', '0', '--batch_size', '4', '--predict', str(d), '--predictions', out, '--sequence', 'lag',
                   '--seq_lag', str(LAG), '--seq_sigma', '2.0', '--seq_rho', '0.1', '--render', pics], str(tmp_path))
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    line = json.loads(res.stdout.strip().splitlines()[-1])
    assert line['sequence'] == 'lag' and line['seq_lag'] == LAG and line['n_images'] == 6 and line['render_ms'] > 0
    doc = json.load(open(out))
    for e, w in zip(doc['images'], whole):
        assert e['track']['mode'] == 'lag' and e['track']['lag'] == int(w['track']['lag'])
        assert_array_equal(np.array(e['track']['points']), w['track']['points'])
        assert_array_equal(np.array(e['track']['cut']), w['track']['cut'])
        assert_array_equal(np.array(e['track']['conf'], np.float32), w['track']['conf'])
    assert sorted(os.listdir(pics)) == ['%05d_frame%02d.png' % (i, i) for i in range(6)]
