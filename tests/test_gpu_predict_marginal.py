"""The smoothed marginals in --predict (predict.predict_sequence(mode='marginal'), predict.seq_fit, main.py --sequence marginal and
--seq_fit) on the six synthetic 96x128 frames the sequence tests use, and a rendered clip (dataset.render_clip) against the renderer's
restatement."""
import json
import os

import numpy as np
import pytest
import torch
from numpy.testing import assert_array_equal

import synth_people_ref as SP
from cli_util import run_cli
import joint_cnn_mrf_amd  # noqa: F401
from joint_cnn_mrf_amd import dataset, synth
from joint_cnn_mrf_amd import main as M
from joint_cnn_mrf_amd import predict as P
from joint_cnn_mrf_amd.evaluation import fit_to_source

pytestmark = pytest.mark.gpu
KEYS = {'size', 'joint_names', 'geom', 'pd', 'pd_inside', 'sm', 'sm_inside', 'torso_cell'}
TRACK = {'mode', 'points', 'inside', 'conf', 'norm', 'reset', 'cut'}
HERE = os.path.dirname(os.path.abspath(__file__))


def _frames():
    """Six frames of one clip: a bright square drifting over a noisy background (those of test_gpu_predict_sequence.py)."""
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


def test_marginal_track_is_seq_smooth_on_the_kept_maps(world):
    eng, frames, plain = world
    got = P.predict_sequence(eng, frames, mode='marginal', sigma=2.0, rho=0.1, batch_size=4)
    hm = torch.stack([r['maps']['sm'] for r in plain]).contiguous()
    seq = eng.seq_smooth(hm, 2.0, 0.1)
    torch.cuda.synchronize()
    cells = seq['coords'].cpu().numpy().transpose(0, 2, 1).astype(np.float64)
    pts, inside = fit_to_source(cells * P.STRIDE, np.array([r['geom'] for r in plain], np.int64))
    for t, (g, a) in enumerate(zip(got, plain)):
        assert set(g) == KEYS | {'track'} and set(g['track']) == TRACK and g['track']['mode'] == 'marginal'
        for k in KEYS:      # every earlier key keeps its value
            assert_array_equal(np.asarray(g[k]), np.asarray(a[k]))
        assert_array_equal(g['track']['points'], pts[t])
        assert_array_equal(g['track']['inside'], inside[t])
        for k in ('conf', 'norm', 'reset', 'cut'):
            assert_array_equal(g['track'][k], seq[k][t].cpu().numpy())
        assert g['track']['points'].shape == (9, 2) and g['track']['conf'].shape == (9,)
        assert ((g['track']['conf'] > 0) & (g['track']['conf'] <= 1)).all()
    json.dumps(P.predictions_document(['f%d' % i for i in range(6)], got))      # the document takes the track
    # the track is drawn like the other two
    prims = P.skeleton_primitives(got, which='track')
    moved = [dict(r, sm=r['track']['points'], sm_inside=r['track']['inside']) for r in got]
    assert prims.shape[0] > 0
    assert_array_equal(prims, P.skeleton_primitives(moved, which='sm'))
    for a, b in zip(P.render_images(eng, frames, got, which='track', batch_size=4), P.render_images(eng, frames, moved, which='sm', batch_size=4)):
        assert_array_equal(a, b)


def test_fit_iters_runs_the_mode_with_the_fitted_values(world):
    eng, frames, plain = world
    got = P.predict_sequence(eng, frames, mode='viterbi', sigma=2.0, rho=0.1, batch_size=4, fit_iters=2)
    hm = torch.stack([r['maps']['sm'] for r in plain]).contiguous()
    fit = P.seq_fit(eng, hm, 2.0, 0.1, iters=2)
    assert set(got[0]) == KEYS | {'track', 'seq_fit'} and all('seq_fit' not in g for g in got[1:])
    assert_array_equal(got[0]['seq_fit']['sigma'], fit['sigma'])
    assert got[0]['seq_fit']['rho'] == fit['rho'] and fit['loglik'].shape == (3,) and fit['sigma'].shape == (9,)
    want = eng.seq_viterbi(hm, fit['sigma'], fit['rho'])
    torch.cuda.synchronize()
    for t, g in enumerate(got):
        assert_array_equal(g['track']['maxes'], want['maxes'][t].cpu().numpy())
    json.dumps(P.predictions_document(['f%d' % i for i in range(6)], got))


def test_refused_requests(world):
    eng, frames, _ = world
    with pytest.raises(ValueError, match='filter and Viterbi only'):
        P.predict_sequence_people(eng, frames, 2, mode='marginal')
    with pytest.raises(ValueError, match='fit_iters'):
        P.predict_sequence(eng, frames, mode='marginal', fit_iters=101)
    with pytest.raises(ValueError, match='iters'):
        P.seq_fit(eng, torch.zeros(2, 4, 4, 1, device='cuda:0'), iters=0)

    def refusal(argv):
        with pytest.raises(SystemExit) as e:
            M.main(argv)
        return str(e.value)

    base = ['--synthetic', '--debug', '--use_sm', '--gpus', '0', '--predict', HERE, '--predictions', os.path.join(HERE, 'never_written.json')]
    assert refusal(base + ['--seq_fit', '3']) == M.SEQ_FIT_NEEDS_SEQUENCE
    assert refusal(base + ['--sequence', 'marginal', '--seq_fit', '0']) == '--seq_fit 0: 1 <= ITERS <= 100'
    assert refusal(base + ['--sequence', 'filter', '--seq_fit', '101']) == '--seq_fit 101: 1 <= ITERS <= 100'
    assert refusal(base + ['--sequence', 'viterbi', '--seq_fit', '3', '--seq_people', '2']) == M.SEQ_FIT_NO_PEOPLE
    assert refusal(base + ['--sequence', 'marginal', '--seq_people', '2']) == M.SEQ_MARGINAL_NO_PEOPLE
    assert refusal(['--synthetic', '--sequence', 'marginal']) == M.SEQUENCE_NEEDS_PREDICT      # the earlier tables come first


def test_cli_marginal_with_fit(world, tmp_path):
    eng, frames, _ = world
    d = tmp_path / 'clip'
    d.mkdir()
    for i, im in enumerate(frames):
        np.save(str(d / ('frame%02d.npy' % i)), im)
    out, pics = str(tmp_path / 'track.json'), str(tmp_path / 'pics')
    res = run_cli(['--synthetic', '--debug', '--use_sm', '--gpus', '0', '--batch_size', '4', '--predict', str(d), '--predictions', out, '--sequence', 'marginal',
                   '--seq_sigma', '2.0', '--seq_rho', '0.1', '--seq_fit', '2', '--render', pics], str(tmp_path))
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    line = json.loads(res.stdout.strip().splitlines()[-1])
    want = P.predict_sequence(eng, frames, mode='marginal', sigma=2.0, rho=0.1, batch_size=4, fit_iters=2)
    fit = want[0]['seq_fit']
    assert line['sequence'] == 'marginal' and line['n_images'] == 6 and line['render_ms'] > 0
    assert set(line['seq_fit']) == {'sigma', 'rho', 'loglik', 'clamped'}
    assert line['seq_fit']['sigma'] == fit['sigma'].tolist() and line['seq_fit']['rho'] == fit['rho'] and len(line['seq_fit']['loglik']) == 3
    doc = json.load(open(out))
    for e, w in zip(doc['images'], want):
        assert e['track']['mode'] == 'marginal'
        assert_array_equal(np.array(e['track']['points']), w['track']['points'])
        assert_array_equal(np.array(e['track']['cut']), w['track']['cut'])
        assert_array_equal(np.array(e['track']['conf'], np.float32), w['track']['conf'])
    assert sorted(os.listdir(pics)) == ['%05d_frame%02d.png' % (i, i) for i in range(6)]


def test_rendered_clip_is_the_restatements(world):
    """A 48x72 three-frame clip with a cut, drawn by one Engine.synth_people call, against tests/synth_people_ref.py on its records."""
    eng = world[0]
    poses = np.load(os.path.join(HERE, 'golden', 'flic_train_xy.npy'))
    x, records, prims, xy = dataset.render_clip(eng, np.random.RandomState(3), poses[10], poses[500], 3, poses[20], H=48, W=72, cuts=(2,))
    torch.cuda.synchronize()
    assert x.shape == (3, 48, 72, 3) and x.dtype == torch.uint8 and xy.shape == (3, 2, 9)
    assert_array_equal(x.cpu().numpy(), SP.render_batch(records, prims, 48, 72))
    assert (x[0] != x[1]).any() and (x[1] != x[2]).any()
    want = synth.people_clip(np.random.RandomState(3), poses[10], poses[500], 3, poses[20], H=48, W=72, cuts=(2,))
    assert_array_equal(records, want[0])
    assert_array_equal(xy, want[2])
