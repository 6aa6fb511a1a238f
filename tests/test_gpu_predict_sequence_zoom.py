"""Zoomed clips of --predict (predict.predict_sequence_zoom, main.py --seq_zoom) on six synthetic 96x144 byte frames with the narrow
parameters and generated priors of --synthetic --debug: every key of predict_sequence keeps its value, 'track_zoom' is the composition it is
made of -- zoom_window_track, Engine.fit_windows, the forward, Engine.seq_viterbi(shift=), evaluation.window_to_source --, a clip with no valid
frame is reported unzoomed, and the command line with --render."""
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
from joint_cnn_mrf_amd.evaluation import fit_to_source, window_to_source

pytestmark = pytest.mark.gpu
T = 6
ARGS = dict(sigma=2.0, rho=0.1, batch_size=4)
TRACK_ZOOM = {'filter': {'mode', 'points', 'inside', 'window', 'shift', 'pitch', 'norm', 'reset'},
              'viterbi': {'mode', 'points', 'inside', 'window', 'shift', 'pitch', 'maxes', 'breaks'}}
ZOOM = {'zoomed', 'window', 'torso_len', 'pd', 'pd_inside', 'sm', 'sm_inside'}


def _frames():
    """Six frames of one clip: a bright square drifting over a noisy background."""
    rs = np.random.RandomState(78)
    frames = []
    for t in range(T):
        im = rs.randint(0, 96, (96, 144, 3)).astype(np.uint8)
        im[30 + 4 * t:50 + 4 * t, 20 + 12 * t:44 + 12 * t] = 230
        frames.append(im)
    return frames


@pytest.fixture(scope='module')
def world():
    from joint_cnn_mrf_amd.engine import Engine
    p = synth.make_pd_params(debug=True)
    p.update(synth.make_sm_params(synth.synthetic_priors(), kind='init'))
    eng = Engine(device=0).load_params(p)
    frames = _frames()
    plain = {mode: P.predict_sequence(eng, frames, mode=mode, keep_maps=True, torso_prob=True, **ARGS) for mode in ('filter', 'viterbi')}
    yield eng, frames, plain
    eng.close()


def _same(a, b):
    if isinstance(a, dict):
        assert set(a) == set(b)
        for k in a:
            _same(a[k], b[k])
    else:
        assert_array_equal(np.asarray(a), np.asarray(b))


@pytest.mark.parametrize('mode', ['filter', 'viterbi'])
def test_track_zoom_is_its_composition(world, mode):
    eng, frames, plain = world
    first = plain[mode]
    timing = {}
    got = P.predict_sequence_zoom(eng, frames, mode=mode, timing=timing, **ARGS)
    # pass 1 and the windows, restated
    torso_maps = torch.stack([r['maps']['torso_prob'] for r in first]).contiguous()
    torso = eng.seq_tracks(torso_maps, 1, P.SEQ_TORSO_SIGMA, ARGS['rho'], mode=mode)
    torch.cuda.synchronize()
    tc = torso['coords' if mode == 'filter' else 'path'].cpu().numpy().reshape(T, 2).astype(np.float64)
    geom1 = np.array([r['geom'] for r in first], np.int64)
    torso_px, _ = fit_to_source(tc * P.STRIDE, geom1)
    points, inside = np.stack([r['track']['points'] for r in first]), np.stack([r['track']['inside'] for r in first])
    wins, cells, shift, pitch, valid = P.zoom_window_track(points, inside, torso_px, geom1)
    assert pitch > 0 and valid.any(), 'the clip of this test must have a valid frame'
    assert timing['seq_zoom_pitch'] == pitch and timing['zoom_fit_ms'] > 0 and timing['zoom_forward_ms'] > 0 and timing['fit_ms'] > 0
    # pass 2, restated in the same batches of four
    parts, geoms = [], []
    for lo in range(0, T, ARGS['batch_size']):
        hi = min(T, lo + ARGS['batch_size'])
        local = wins[lo:hi].copy()
        local[:, 0] -= lo
        x2, g2 = eng.fit_windows([torch.from_numpy(f).to(eng.device) for f in frames[lo:hi]], local, out_hw=P.FRAME)
        blob = eng.torso_infer(None, cells=torch.from_numpy(cells[lo:hi].copy()).to(eng.device))['torso']
        part = eng.forward(x2, torso=blob, use_sm=True, want_prob=True)
        parts.append({k: part[k].clone() for k in ('sm_prob', 'sm_coords', 'pd_coords')})
        geoms.append(g2)
    r2 = {k: torch.cat([p[k] for p in parts]) for k in parts[0]}
    geom2 = np.concatenate(geoms)
    seq =(eng.seq_filter if mode == 'filter' else eng.seq_viterbi)(r2['sm_prob'].contiguous(), ARGS['sigma'], ARGS['rho'], shift=shift)
    torch.cuda.synchronize()
    sizes = np.array([r['size'] for r in first], np.int64)
    tpts, tin = window_to_source(P._coords_to_points(seq['coords' if mode == 'filter' else 'path']), geom2, wins, sizes)
    second = {key: window_to_source(P._coords_to_points(r2[key + '_coords']), geom2, wins, sizes) for key in ('pd', 'sm')}
    value, flag = ('norm', 'reset') if mode == 'filter' else ('maxes', 'breaks')
    for t, (g, a) in enumerate(zip(got, first)):
        assert set(g) == (set(a) - {'maps'}) | {'zoom', 'track_zoom'}
        for k in set(a) - {'maps'}:      # every key of predict_sequence keeps its value
            _same(g[k], a[k])
        tz = g['track_zoom']
        assert set(tz) == TRACK_ZOOM[mode] and tz['mode'] == mode and tz['pitch'] == pitch
        assert tz['window'] == tuple(int(v) for v in wins[t, 1:]) and tz['shift'] == (int(shift[t, 0]), int(shift[t, 1]))
        assert_array_equal(tz['points'], tpts[t])
        assert_array_equal(tz['inside'], tin[t])
        assert_array_equal(tz[value], seq[value][t].cpu().numpy())
        assert_array_equal(tz[flag], seq[flag][t].cpu().numpy())
        assert tz['points'].shape == (9, 2) and tz['inside'].shape == (9,)
        assert len(g['zoom']) == 1 and set(g['zoom'][0]) == ZOOM and g['zoom'][0]['zoomed'] is True and g['zoom'][0]['window'] == tz['window']
        for key in ('pd', 'sm'):
            assert_array_equal(g['zoom'][0][key], second[key][0][t])
            assert_array_equal(g['zoom'][0][key + '_inside'], second[key][1][t])
    json.dumps(P.predictions_document(['f%d' % i for i in range(T)], got))      # the document takes the new keys
    kept = P.predict_sequence_zoom(eng, frames, mode=mode, keep_maps=True, **ARGS)
    assert set(kept[0]['maps']) == {'pd', 'sm', 'torso_prob', 'sm_zoom'}
    assert_array_equal(kept[2]['maps']['sm_zoom'].cpu().numpy(), r2['sm_prob'][2].cpu().numpy())


def test_a_clip_with_no_valid_frame_is_not_zoomed(world, monkeypatch):
    """Torsos below two pass-1 cells in every frame (here: of length 0 by decree) are quantisation, zoom_window_track's skip rule."""
    eng, frames, plain = world
    monkeypatch.setattr(P, 'torso_length', lambda sm: np.zeros(np.asarray(sm).shape[:-2]))
    timing = {}
    got = P.predict_sequence_zoom(eng, frames, mode='viterbi', timing=timing, **ARGS)
    assert timing['seq_zoom_pitch'] == 0 and timing['zoom_fit_ms'] == 0.0 and timing['zoom_forward_ms'] == 0.0
    for g, a in zip(got, plain['viterbi']):
        assert set(g) == (set(a) - {'maps'}) | {'zoom'}
        for k in set(a) - {'maps'}:
            _same(g[k], a[k])
        e, = g['zoom']
        assert e['zoomed'] is False and set(e) == ZOOM
        for key in ('pd', 'sm', 'pd_inside', 'sm_inside'):
            assert_array_equal(e[key], a[key])
    assert P.render_images(eng, frames, got, batch_size=4)[0].shape == frames[0].shape      # the default falls back to 'sm'


def test_track_zoom_is_drawn(world):
    eng, frames, _ = world
    res = P.predict_sequence_zoom(eng, frames, mode='viterbi', **ARGS)
    moved = [dict({k: v for k, v in r.items() if k not in ('zoom', 'track_zoom')}, sm=r['track_zoom']['points'], sm_inside=r['track_zoom']['inside']) for r in res]
    want = P.render_images(eng, frames, moved, which='sm', batch_size=4)
    for which in ('track_zoom', None):      # drawn when it is there
        for a, b in zip(P.render_images(eng, frames, res, which=which, batch_size=4), want):
            assert_array_equal(a, b)


def test_cli_seq_zoom_render(world, tmp_path):
    eng, frames, _ = world
    d = tmp_path / 'clip'
    d.mkdir()
    for i, im in enumerate(frames):
        np.save(str(d / ('frame%02d.npy' % i)), im)
    out, pics = str(tmp_path / 'track.json'), str(tmp_path / 'pics')
    res = run_cli(['--synthetic', '--debug', '--use_sm', '--gpus', '0', '--batch_size', '4', '--predict', str(d), '--predictions', out, '--sequence', 'viterbi',
                   '--seq_sigma', '2.0', '--seq_rho', '0.1', '--seq_zoom', '--render', pics], str(tmp_path))
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    line = json.loads(res.stdout.strip().splitlines()[-1])
    want = P.predict_sequence_zoom(eng, frames, mode='viterbi', **ARGS)
    assert line['seq_zoom'] is True and line['sequence'] == 'viterbi' and line['n_images'] == T and line['render_ms'] > 0
    assert line['seq_zoom_pitch'] == want[0]['track_zoom']['pitch'] and line['zoom_fit_ms'] > 0 and line['zoom_forward_ms'] > 0 and 'zoom' not in line
    doc = json.load(open(out))
    for e, w in zip(doc['images'], want):
        assert e['track_zoom']['mode'] == 'viterbi' and tuple(e['track_zoom']['window']) == w['track_zoom']['window']
        assert_array_equal(np.array(e['track_zoom']['points']), w['track_zoom']['points'])
        assert_array_equal(np.array(e['track_zoom']['breaks']), w['track_zoom']['breaks'])
        assert_array_equal(np.array(e['track']['points']), w['track']['points'])
        assert_array_equal(np.array(e['zoom'][0]['sm']), w['zoom'][0]['sm'])
    assert sorted(os.listdir(pics)) == ['%05d_frame%02d.png' % (i, i) for i in range(T)]
