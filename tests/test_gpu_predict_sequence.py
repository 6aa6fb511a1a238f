"""Frame sequences of --predict (predict.predict_sequence, predict.SequenceTracker, main.py --sequence) on six synthetic 96x128
byte frames with the narrow parameters and generated priors of --synthetic --debug: the track against Engine.seq_* on the kept maps, every
earlier key against predict_images, the online tracker against the one-call filter, and the command line with --render."""
import json
import os

import numpy as np
import pytest
import torch
from numpy.testing import assert_array_equal

from cli_util import run_cli
import joint_cnn_mrf_amd  # noqa: F401
from joint_cnn_mrf_amd import predict as P
from joint_cnn_mrf_amd import synth
from joint_cnn_mrf_amd.evaluation import fit_to_source

pytestmark = pytest.mark.gpu
KEYS = {'size', 'joint_names', 'geom', 'pd', 'pd_inside', 'sm', 'sm_inside', 'torso_cell'}      # predict_images(use_sm=True)
TRACK = {'filter': {'mode', 'points', 'inside', 'norm', 'reset'}, 'viterbi': {'mode', 'points', 'inside', 'maxes', 'breaks'}}


def _frames():
    """Six frames of one clip: a bright square drifting over a noisy background."""
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
    yield eng, frames, P.predict_images(eng, frames, use_sm=True, batch_size=4, keep_maps=True)
    eng.close()


@pytest.mark.parametrize('mode', ['filter', 'viterbi'])
def test_track_is_the_sequence_call_on_the_kept_maps(world, mode):
    eng, frames, plain = world
    got = P.predict_sequence(eng, frames, mode=mode, sigma=2.0, rho=0.1, batch_size=4)
    hm = torch.stack([r['maps']['sm'] for r in plain]).contiguous()
    seq = (eng.seq_filter if mode == 'filter' else eng.seq_viterbi)(hm, 2.0, 0.1)
    torch.cuda.synchronize()
    cells = seq['coords' if mode == 'filter' else 'path'].cpu().numpy().transpose(0, 2, 1).astype(np.float64)
    pts, inside = fit_to_source(cells * P.STRIDE, np.array([r['geom'] for r in plain], np.int64))
    value, flag = ('norm', 'reset') if mode == 'filter' else ('maxes', 'breaks')
    for t, (g, a) in enumerate(zip(got, plain)):
        assert set(g) == KEYS | {'track'} and set(g['track']) == TRACK[mode] and g['track']['mode'] == mode
        for k in KEYS:      # every earlier key keeps its value
            assert_array_equal(np.asarray(g[k]), np.asarray(a[k]))
        assert_array_equal(g['track']['points'], pts[t])
        assert_array_equal(g['track']['inside'], inside[t])
        assert_array_equal(g['track'][value], seq[value][t].cpu().numpy())
        assert_array_equal(g['track'][flag], seq[flag][t].cpu().numpy())
        assert g['track']['points'].shape == (9, 2) and g['track']['inside'].shape == (9,)
    kept = P.predict_sequence(eng, frames, mode=mode, sigma=2.0, rho=0.1, batch_size=4, keep_maps=True, use_sm=False)
    assert set(kept[0]) == (KEYS - {'sm', 'sm_inside', 'torso_cell'}) | {'track', 'maps'} and set(kept[0]['maps']) == {'pd'}
    json.dumps(P.predictions_document(['f%d' % i for i in range(6)], got))      # the document takes the track


def test_tracker_in_two_halves_is_one_filter_call(world):
    eng, frames, _ = world
    whole = P.predict_sequence(eng, frames, mode='filter', batch_size=3)      # the same batches of three either way
    tracker = P.SequenceTracker(eng, batch_size=3)
    halves = tracker.push(frames[:3]) + tracker.push(frames[3:])
    for a, b in zip(halves, whole):
        assert set(a) == set(b)
        for k in ('points', 'inside', 'norm', 'reset'):
            assert_array_equal(a['track'][k], b['track'][k])
    with pytest.raises(ValueError, match='one size'):
        tracker.push([np.zeros((64, 64, 3), np.uint8)])
    tracker.reset()
    again = tracker.push(frames[:1])
    assert_array_equal(again[0]['track']['points'], whole[0]['track']['points'])


def test_refused_requests(world):
    eng, frames, _ = world
    with pytest.raises(ValueError, match='one size'):
        P.predict_sequence(eng, frames[:2] + [np.zeros((64, 64, 3), np.uint8)])
    with pytest.raises(ValueError, match='people'):
        P.predict_sequence(eng, frames, people=2)
    with pytest.raises(ValueError, match='zoom'):
        P.predict_sequence(eng, frames, zoom=True)
    with pytest.raises(ValueError, match='mode'):
        P.predict_sequence(eng, frames, mode='smooth')


def test_track_is_drawn(world):
    eng, frames, _ = world
    res = P.predict_sequence(eng, frames, mode='viterbi', batch_size=4)
    prims = P.skeleton_primitives(res, which='track')
    assert prims.shape[0] > 0
    moved = [dict(r, sm=r['track']['points'], sm_inside=r['track']['inside']) for r in res]
    assert_array_equal(prims, P.skeleton_primitives(moved, which='sm'))      # the same capsules as the same joints under another name
    for a, b in zip(P.render_images(eng, frames, res, which='track', batch_size=4), P.render_images(eng, frames, moved, which='sm', batch_size=4)):
        assert_array_equal(a, b)
    with pytest.raises(ValueError, match='predict_sequence'):
        P.skeleton_primitives(world[2], which='track')


def test_cli_sequence_render(world, tmp_path):
    eng, frames, _ = world
    d = tmp_path / 'clip'
    d.mkdir()
    for i, im in enumerate(frames):
        np.save(str(d / ('frame%02d.npy' % i)), im)
    out, pics = str(tmp_path / 'track.json'), str(tmp_path / 'pics')
    res = run_cli(['--synthetic', '--debug', '--use_sm', '--gpus', '0', '--batch_size', '4', '--predict', str(d), '--predictions', out, '--sequence', 'viterbi',
                   '--seq_sigma', '2.0', '--seq_rho', '0.1', '--render', pics], str(tmp_path))
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    line = json.loads(res.stdout.strip().splitlines()[-1])
    assert line['sequence'] == 'viterbi' and line['render_ms'] > 0 and line['n_images'] == 6
    doc = json.load(open(out))
    want = P.predict_sequence(eng, frames, mode='viterbi', sigma=2.0, rho=0.1, batch_size=4)
    assert [os.path.basename(e['path']) for e in doc['images']] == ['frame%02d.npy' % i for i in range(6)]
    for e, w in zip(doc['images'], want):
        assert e['track']['mode'] == 'viterbi'
        assert_array_equal(np.array(e['track']['points']), w['track']['points'])
        assert_array_equal(np.array(e['track']['breaks']), w['track']['breaks'])
        assert_array_equal(np.array(e['sm']), w['sm'])
    assert sorted(os.listdir(pics)) == ['%05d_frame%02d.png' % (i, i) for i in range(6)]
