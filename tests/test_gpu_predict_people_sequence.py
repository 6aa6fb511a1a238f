"""Clips with several people (predict.predict_sequence_people, predict.PeopleTracker, main.py --seq_people) on five synthetic
96x128 byte frames with the narrow parameters and generated priors of --synthetic --debug, people = 2: 'tracks' against the composition of
Engine calls done by hand, 'track' against track 0, the online tracker against the one-call filter, every earlier key against predict_images,
the pictures' skeleton count, and the command line."""
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
NUM = {'filter': ('coords', 'norm', 'reset'), 'viterbi': ('path', 'maxes', 'breaks')}
M, T = 2, 5
ARGS = dict(sigma=2.0, torso_sigma=1.0, rho=0.1, exclude=3)


def _frames():
    """Five frames of one clip: two bright squares drifting over a noisy background, towards each other."""
    rs = np.random.RandomState(78)
    frames = []
    for t in range(T):
        im = rs.randint(0, 96, (96, 128, 3)).astype(np.uint8)
        im[10 + 2 * t:30 + 2 * t, 10 + 8 * t:30 + 8 * t] = 230
        im[60 - 2 * t:84 - 2 * t, 90 - 8 * t:118 - 8 * t] = 200
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
def test_tracks_are_the_engine_calls_composed_by_hand(world, mode):
    eng, frames, plain = world
    got = P.predict_sequence_people(eng, frames, M, mode=mode, batch_size=4, **ARGS)
    cells_key, value, flag = NUM[mode]
    # step 1: the torso maps, spatial_softmax of the energy of the frames' part-detector maps
    pd = torch.stack([r['maps']['pd'] for r in plain]).contiguous()
    with torch.cuda.stream(eng._stream):
        energy = eng.torso_infer(pd, want_energy=True)['energy']
        torso_prob = eng.spatial_softmax(energy.view(T, 60, 90, 1)).view(T, 60, 90)
        # step 2: the torso tracks
        torso = eng.seq_tracks(torso_prob, M, ARGS['torso_sigma'], ARGS['rho'], exclude=ARGS['exclude'], mode=mode)
        # step 3: per (frame, track) the spatial model at the track's cell
        maps = []
        for m in range(M):
            blob = eng.torso_infer(None, cells=torso[cells_key][m].contiguous())['torso']
            prob, _ = eng.softmax_argmax(eng.spatial_model(torch.cat([pd, blob], dim=3)), want_prob=True)
            maps.append(prob)
        # step 4: the persons as the sequences of the existing calls
        seq = (eng.seq_filter if mode == 'filter' else eng.seq_viterbi)(torch.stack(maps).contiguous(), ARGS['sigma'], ARGS['rho'])
    torch.cuda.synchronize()
    geom = np.array([r['geom'] for r in plain], np.int64)
    tv, tf = torso['value'].cpu().numpy(), torso[flag].cpu().numpy()
    present = (tv > 0.0) & (tf != 2)
    for t, (g, a) in enumerate(zip(got, plain)):
        assert set(g) == KEYS | {'track', 'tracks'}
        for k in KEYS:      # every earlier key keeps its value
            assert_array_equal(np.asarray(g[k]), np.asarray(a[k]))
        tr = g['tracks']
        assert set(tr) == {'mode', 'count', 'torso', 'torso_value', 'present', 'points', 'inside', value, flag} and tr['mode'] == mode
        # step 5
        tpts, _ = fit_to_source(torso[cells_key][:, t].cpu().numpy().astype(np.float64)[None] * P.STRIDE, geom[t:t + 1])
        assert_array_equal(tr['torso'], tpts[0])
        assert_array_equal(tr['torso_value'], tv[:, t])
        assert_array_equal(tr['present'], present[:, t])
        assert tr['count'] == int(present.any(axis=1).sum())
        cells = seq[cells_key][:, t].cpu().numpy().transpose(0, 2, 1).astype(np.float64)      # [M,K,2]
        pts, inside = fit_to_source(cells[None] * P.STRIDE, geom[t:t + 1])
        assert_array_equal(tr['points'], pts[0])
        assert_array_equal(tr['inside'], inside[0])
        assert_array_equal(tr[value], seq[value][:, t].cpu().numpy())
        assert_array_equal(tr[flag], seq[flag][:, t].cpu().numpy())
        assert tr['points'].shape == (M, 9, 2) and tr['inside'].shape == (M, 9) and tr['torso'].shape == (M, 2)
        # 'track' is track 0 in the layout of predict_sequence
        assert set(g['track']) == {'mode', 'points', 'inside', value, flag}
        for k in ('points', 'inside', value, flag):
            assert_array_equal(g['track'][k], tr[k][0])
    # the two torso tracks are two places: the second keeps out of the first's neighbourhood wherever the first has support
    c = torso[cells_key].cpu().numpy()
    assert (np.abs(c[0] - c[1]).max(axis=1)[tv[0] > 0] > ARGS['exclude']).all()
    json.dumps(P.predictions_document(['f%d' % i for i in range(T)], got))


def test_tracker_frame_by_frame_is_one_filter_call(world):
    eng, frames, _ = world
    whole = P.predict_sequence_people(eng, frames, M, mode='filter', batch_size=1, **ARGS)
    tracker = P.PeopleTracker(eng, M, batch_size=1, **ARGS)
    pushed = [tracker.push([f])[0] for f in frames]
    for a, b in zip(pushed, whole):
        assert set(a) == set(b)
        for k in ('torso', 'torso_value', 'present', 'points', 'inside', 'norm', 'reset'):
            assert_array_equal(a['tracks'][k], b['tracks'][k])
        for k in ('points', 'inside', 'norm', 'reset'):
            assert_array_equal(a['track'][k], b['track'][k])
    with pytest.raises(ValueError, match='one size'):
        tracker.push([np.zeros((64, 64, 3), np.uint8)])
    tracker.reset()
    again = tracker.push(frames[:1])
    assert_array_equal(again[0]['tracks']['points'], whole[0]['tracks']['points'])


def test_torso_prob_is_kept_only_on_request(world):
    eng, frames, plain = world
    assert all(set(r['maps']) == {'pd', 'sm'} for r in plain)
    kept = P.predict_images(eng, frames, use_sm=True, batch_size=4, keep_maps=True, torso_prob=True)
    for a, b in zip(kept, plain):
        assert set(a) == set(b) and set(a['maps']) == {'pd', 'sm', 'torso_prob'} and tuple(a['maps']['torso_prob'].shape) == (60, 90)
        for k in KEYS:
            assert_array_equal(np.asarray(a[k]), np.asarray(b[k]))
        for k in ('pd', 'sm'):
            assert torch.equal(a['maps'][k], b['maps'][k])
    with pytest.raises(ValueError, match='torso_prob'):
        P.predict_images(eng, frames, use_sm=True, torso_prob=True)
    x, _ = eng.fit_images(frames[:1], out_hw=P.FRAME)
    assert 'torso_prob' not in eng.forward(x, 'infer') and 'torso_prob' in eng.forward(x, 'infer', want_torso_prob=True)


def test_refused_requests(world):
    eng, frames, _ = world
    with pytest.raises(ValueError, match='people'):
        P.predict_sequence(eng, frames, people=2)      # the one-person call stays what it was
    with pytest.raises(ValueError, match='zoom'):
        P.predict_sequence_people(eng, frames, M, zoom=True)
    with pytest.raises(ValueError, match='1..4'):
        P.predict_sequence_people(eng, frames, 5)
    with pytest.raises(ValueError, match='mode'):
        P.predict_sequence_people(eng, frames, M, mode='smooth')


def test_one_skeleton_per_present_track(world):
    eng, frames, _ = world
    res = P.predict_sequence_people(eng, frames, M, mode='viterbi', batch_size=4, **ARGS)
    full = [i for i, r in enumerate(res) if r['tracks']['present'].all()]
    assert full and res[full[0]]['tracks']['count'] == M
    i = full[0]
    r = res[i]
    per_track = [P.skeleton_primitives([dict(r, sm=r['tracks']['points'][m], sm_inside=r['tracks']['inside'][m])], which='sm') for m in range(M)]
    prims = P.skeleton_primitives([r], which='track')
    assert prims.shape[0] == sum(p.shape[0] for p in per_track) > 0
    assert_array_equal(prims, np.concatenate(per_track))
    pictures = P.render_images(eng, frames, res, which='track', batch_size=4)
    assert len(pictures) == T and pictures[i].shape == frames[i].shape


def test_cli_seq_people(world, tmp_path):
    eng, frames, _ = world
    d = tmp_path / 'clip'
    d.mkdir()
    for i, im in enumerate(frames):
        np.save(str(d / ('frame%02d.npy' % i)), im)
    out = str(tmp_path / 'tracks.json')
    res = run_cli(['--synthetic', '--debug', '--use_sm', '--gpus', '0', '--batch_size', '4', '--predict', str(d), '--predictions', out, '--sequence', 'viterbi',
                   '--seq_sigma', '2.0', '--seq_rho', '0.1', '--seq_people', '2', '--seq_torso_sigma', '1.0', '--seq_exclude', '3'], str(tmp_path))
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    line = json.loads(res.stdout.strip().splitlines()[-1])
    assert line['sequence'] == 'viterbi' and line['seq_people'] == 2 and line['n_images'] == T and line['seq_torso_ms'] > 0 and line['seq_people_sm_ms'] > 0
    doc = json.load(open(out))
    want = P.predict_sequence_people(eng, frames, M, mode='viterbi', batch_size=4, **ARGS)
    assert [os.path.basename(e['path']) for e in doc['images']] == ['frame%02d.npy' % i for i in range(T)]
    for e, w in zip(doc['images'], want):
        assert e['tracks']['mode'] == 'viterbi' and e['tracks']['count'] == w['tracks']['count']
        for k in ('torso', 'points', 'breaks', 'present'):
            assert_array_equal(np.array(e['tracks'][k]), w['tracks'][k])
        assert_array_equal(np.array(e['track']['points']), w['tracks']['points'][0])
