"""Clip pose decoding in the prediction layer, on the GPU: predict.predict_sequence(mode='viterbi', pose=P) on a four-frame clip of
a rendered person (dataset.render_clip), an engine with the narrow synthetic parameters.  pose=0 must change nothing; pose=2 must leave 'track' and
every other key what it was and add 'track_pose', which must be the restatement (tests/seq_pose_ref.py) fed with the same tables; pose_weight=0 must
give every frame's own decode; and the command line."""
import json
import os

import numpy as np
import pytest
import torch
from numpy.testing import assert_array_equal

import seq_pose_ref as R
from cli_util import run_cli
import joint_cnn_mrf_amd  # noqa: F401
from joint_cnn_mrf_amd import dataset, synth
from joint_cnn_mrf_amd import predict as P

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
SIGMA, RHO, T, NP = 2.0, 0.1, 4, 2
ARGS = dict(mode='viterbi', sigma=SIGMA, rho=RHO, batch_size=4)
TRACK_POSE = {'peaks', 'index', 'points', 'inside', 'score', 'maxes', 'breaks', 'changed'}


@pytest.fixture(scope='module')
def world():
    """The engine, the clip, the plain track, the run with pose = 2 and the tables made by hand -- computed once, read by every test."""
    from joint_cnn_mrf_amd.engine import Engine
    p = synth.make_pd_params(debug=True)
    p.update(synth.make_sm_params(synth.synthetic_priors(), kind='init'))
    eng = Engine(device=0).load_params(p)
    poses = np.load(os.path.join(HERE, 'golden', 'flic_train_xy.npy'))
    x = dataset.render_clip(eng, np.random.RandomState(3), poses[10], poses[500], T, poses[20])[0]
    torch.cuda.synchronize()
    frames = [x[t] for t in range(T)]
    plain = P.predict_sequence(eng, frames, **ARGS)
    posed = P.predict_sequence(eng, frames, pose=NP, **ARGS)
    one = P.predict_images(eng, frames, use_sm=True, batch_size=4, peaks=NP, decode=True, keep_maps=True, keep_peaks=True)
    maps = [r['maps'] for r in one]
    hm10 = torch.cat([torch.stack([m['pd'] for m in maps]), torch.stack([m['torso'] for m in maps])], dim=3).contiguous()
    peaks = {f: torch.stack([m['pd_peaks'][f] for m in maps]).contiguous() for f in ('cells', 'count')}
    dec = eng.pose_decode(hm10, peaks, want_tables=True)
    torch.cuda.synchronize()
    host = {k: v.cpu().numpy() for k, v in dict(dec, **peaks).items()}
    yield eng, {'frames': frames, 'plain': plain, 'posed': posed, 'one': one, 'host': host}
    eng.close()


def _same(u, v):
    if isinstance(u, dict):
        assert isinstance(v, dict) and list(u) == list(v)
        for k in u:
            _same(u[k], v[k])
    else:
        i, j = np.asarray(u), np.asarray(v)
        assert i.dtype == j.dtype and i.shape == j.shape and i.tobytes() == j.tobytes()


def test_pose_0_changes_nothing(world):
    eng, w = world
    got = P.predict_sequence(eng, w['frames'], pose=0, **ARGS)
    for g, a in zip(got, w['plain']):
        _same(g, a)


def test_pose_2_adds_track_pose_and_keeps_the_rest(world):
    _, w = world
    for g, a, o in zip(w['posed'], w['plain'], w['one']):
        assert set(g) == set(a) | {'track_pose', 'pd_peaks', 'pd_peaks_inside', 'sm_peaks', 'sm_peaks_inside', 'pose', 'pose_inside'}
        assert set(g['track_pose']) == TRACK_POSE and g['track_pose']['peaks'] == NP
        for k in a:      # 'track' among them
            _same(g[k], a[k])
        for k in ('pd_peaks', 'pd_peaks_inside', 'sm_peaks', 'sm_peaks_inside', 'pose', 'pose_inside'):      # what peaks=2, decode=True gives
            _same(g[k], o[k])


def test_track_pose_is_the_restatement_on_the_same_tables(world):
    _, w = world
    h = w['host']
    tau = P.seq_pose_tau(h['cells'], h['count'], SIGMA, RHO)
    want = R.decode_clip(h['V'], h['M'], h['count'], h['cells'], tau)
    for t, g in enumerate(w['posed']):
        tp = g['track_pose']
        assert_array_equal(tp['index'], want['index'][t])
        assert tp['score'] == float(want['frame_score'][t]) and tp['maxes'] == float(want['maxes'][t]) and tp['breaks'] == int(want['breaks'][t])
        assert tp['changed'] == int((want['index'][t] != h['index'][t]).sum())
        pick = np.maximum(want['index'][t], 0).astype(np.int64)
        assert_array_equal(tp['points'], g['pd_peaks'][np.arange(9), pick, :2])
        assert_array_equal(tp['inside'], g['pd_peaks_inside'][np.arange(9), pick])
        # the chosen cell in fitted-frame pixels is the candidate's cell of the library's coords
        assert_array_equal(want['coords'][t].T, h['cells'][t, np.arange(9), pick])


def test_weight_0_is_every_frames_own_decode(world):
    eng, w = world
    got = P.predict_sequence(eng, w['frames'], pose=NP, pose_weight=0.0, **ARGS)
    for t, g in enumerate(got):
        assert_array_equal(g['track_pose']['index'], w['host']['index'][t])
        assert g['track_pose']['changed'] == 0
        assert_array_equal(g['track_pose']['points'], g['pose'][:, :2].astype(np.float64))


def test_refusals(world):
    eng, w = world
    for kw in (dict(pose=5), dict(pose=-1), dict(pose=2, camera=True), dict(pose=2, flow=1), dict(pose=2, flow_centre=True), dict(pose=2, fit_iters=2),
               dict(pose=2, use_sm=False), dict(pose=2, pose_weight=-1.0), dict(pose=True)):
        with pytest.raises(ValueError):
            P.predict_sequence(eng, w['frames'], **dict(ARGS, **kw))
    with pytest.raises(ValueError, match="mode='viterbi'"):
        P.predict_sequence(eng, w['frames'], **dict(ARGS, mode='filter', pose=2))


def test_cli_seq_pose_render(world, tmp_path):
    eng, w = world
    d = tmp_path / 'clip'
    d.mkdir()
    for i, im in enumerate(w['frames']):
        np.save(str(d / ('frame%02d.npy' % i)), im.cpu().numpy())
    out, pics = str(tmp_path / 'track.json'), str(tmp_path / 'pics')
    res = run_cli(['--synthetic', '--debug', '--use_sm', '--gpus', '0', '--batch_size', '4', '--predict', str(d), '--predictions', out, '--sequence', 'viterbi',
                   '--seq_sigma', '2.0', '--seq_rho', '0.1', '--seq_pose', '2', '--seq_pose_weight', '0.5', '--render', pics], str(tmp_path))
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    line = json.loads(res.stdout.strip().splitlines()[-1])
    assert line['seq_pose'] == 2 and line['seq_pose_weight'] == 0.5 and line['sequence'] == 'viterbi' and line['n_images'] == T and line['render_ms'] > 0
    doc = json.load(open(out))
    assert len(doc['images']) == T and len(os.listdir(pics)) == T
    for im in doc['images']:
        tp = im['track_pose']
        assert set(tp) == TRACK_POSE and tp['peaks'] == 2 and len(tp['index']) == 9 and len(tp['points']) == 9 and 'track' in im
        assert all(0 <= i < 2 for i in tp['index']) and 0 <= tp['changed'] <= 9
