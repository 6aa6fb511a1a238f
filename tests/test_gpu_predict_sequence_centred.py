"""Flow-centred scans in the prediction layer, on the GPU: predict.predict_sequence(flow_centre=True) and
SequenceTracker(flow_centre=True) on a four-frame clip of a rendered person seen by a camera that pans (dataset.render_clip_pan), an engine with
synthetic parameters.  The track must be, bit for bit, the composition by hand -- Engine.frame_flow of the kept frames against the frame before,
motion.flow_cell_shifts, Engine.seq_filter(centre=) on the kept maps (the pooled ones with flow = N) --; flow_centre=False must change nothing; any
split of the clip into pushes must give the one call."""
import os

import numpy as np
import pytest
import torch
from numpy.testing import assert_array_equal

import joint_cnn_mrf_amd  # noqa: F401
from joint_cnn_mrf_amd import dataset, synth
from joint_cnn_mrf_amd import predict as P
from joint_cnn_mrf_amd.evaluation import fit_to_source

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
PAN = np.array([[0, 0], [4, -6], [-3, 8], [12, -12]])
MARGIN = (16, 24)
SIGMA, RHO, SEARCH, T = 2.0, 0.1, 8, 4
KEYS = {'filter': ('coords', 'norm', 'reset'), 'viterbi': ('path', 'maxes', 'breaks')}


def _count_flow_calls(monkeypatch, eng):
    """The engine's frame_flow with its calls counted -> the list that grows by one per call."""
    calls, real = [], eng.frame_flow

    def frame_flow(*a, **kw):
        calls.append(1)
        return real(*a, **kw)
    monkeypatch.setattr(eng, 'frame_flow', frame_flow)
    return calls


@pytest.fixture(scope='module')
def world():
    """The engine, the clip, pass 1 with the maps and the frames kept, the table made by hand -- computed once, read by every test."""
    from joint_cnn_mrf_amd.engine import Engine
    p = synth.make_pd_params(debug=True)
    p.update(synth.make_sm_params(synth.synthetic_priors(), kind='init'))
    eng = Engine(device=0).load_params(p)
    poses = np.load(os.path.join(HERE, 'golden', 'flic_train_xy.npy'))
    x = dataset.render_clip_pan(eng, np.random.RandomState(3), poses[10], poses[500], T, PAN, MARGIN, poses[20])[0]
    torch.cuda.synchronize()
    frames = [x[t] for t in range(T)]
    plain = P.predict_images(eng, frames, use_sm=True, batch_size=4, keep_maps=True, keep_frames=True)
    hm = torch.stack([r['maps']['sm'] for r in plain]).contiguous()
    geom = np.array([r['geom'] for r in plain], np.int64)
    flow = eng.frame_flow(x, geom[0, :4], np.array([[-1], [0], [1], [2]], np.int32), search=SEARCH)['flow'][:, 0]
    centre = P.flow_cell_shifts(flow)
    torch.cuda.synchronize()
    yield eng, {'x': x, 'frames': frames, 'plain': plain, 'hm': hm, 'geom': geom, 'flow': flow, 'centre': centre}
    eng.close()


def _points(cells, geom):
    return fit_to_source(cells.cpu().numpy().transpose(0, 2, 1).astype(np.float64) * P.STRIDE, geom)


def _same(u, v):
    if isinstance(u, dict):
        assert isinstance(v, dict) and list(u) == list(v)
        for k in u:
            _same(u[k], v[k])
    elif isinstance(u, (list, tuple)) and u and isinstance(u[0], dict):
        assert len(u) == len(v)
        for i, j in zip(u, v):
            _same(i, j)
    elif isinstance(u, torch.Tensor):
        assert u.dtype == v.dtype and torch.equal(u.view(torch.uint8), v.view(torch.uint8))
    else:
        i, j = np.asarray(u), np.asarray(v)
        assert i.dtype == j.dtype and i.shape == j.shape and i.tobytes() == j.tobytes()


def _check(got, plain, seq, mode, geom, centre, extra=()):
    pts, inside = _points(seq[KEYS[mode][0]], geom)
    moved = (centre != 0).any(dim=3).sum(dim=(1, 2)).cpu().numpy()
    for t, (g, a) in enumerate(zip(got, plain)):
        assert set(g) == (set(a) - {'maps'}) | {'track', 'flow_centre'} | set(extra) and g['track']['mode'] == mode
        for k in set(a) - {'maps'}:      # every earlier key keeps its value
            assert_array_equal(np.asarray(g[k]), np.asarray(a[k]))
        assert_array_equal(g['track']['points'], pts[t])
        assert_array_equal(g['track']['inside'], inside[t])
        for k in KEYS[mode][1:]:
            assert_array_equal(g['track'][k], seq[k][t].cpu().numpy())
        assert g['flow_centre'] == {'search': SEARCH, 'moved': int(moved[t])}


def test_the_clip_moves_and_the_table_is_the_rounded_flow(world):
    eng, c = world
    f, ce = c['flow'].cpu().numpy(), c['centre'].cpu().numpy()
    assert f.shape == (T, 60, 90, 2) and ce.shape == f.shape and ce.dtype == np.int32 and not f[0].any() and f[1:].any()
    assert_array_equal(ce, np.floor((f.astype(np.int64) + 4) / 8.0).astype(np.int32))
    assert ce[1:].any() and len(np.unique(ce[1:].reshape(-1, 2), axis=0)) > 1      # a pan of 12 pixels is more than a cell; the table is not uniform


@pytest.mark.parametrize('mode', ['filter', 'viterbi'])
def test_track_is_the_composition_by_hand(world, mode, monkeypatch):
    eng, c = world
    calls = _count_flow_calls(monkeypatch, eng)
    got = P.predict_sequence(eng, c['frames'], mode=mode, sigma=SIGMA, rho=RHO, batch_size=4, flow_centre=True, flow_search=SEARCH)
    assert len(calls) == 1
    monkeypatch.undo()
    seq = (eng.seq_filter if mode == 'filter' else eng.seq_viterbi)(c['hm'], SIGMA, RHO, centre=c['centre'])
    torch.cuda.synchronize()
    _check(got, c['plain'], seq, mode, c['geom'], c['centre'])
    still = (eng.seq_filter if mode == 'filter' else eng.seq_viterbi)(c['hm'], SIGMA, RHO)
    assert not torch.equal(seq['norm' if mode == 'filter' else 'maxes'], still['norm' if mode == 'filter' else 'maxes'])      # the table does something


def test_with_flow_pooling_there_is_one_matching_call(world, monkeypatch):
    eng, c = world
    calls = _count_flow_calls(monkeypatch, eng)
    got = P.predict_sequence(eng, c['frames'], mode='filter', sigma=SIGMA, rho=RHO, batch_size=4, flow=1, flow_centre=True, flow_search=SEARCH)
    assert len(calls) == 1
    monkeypatch.undo()
    flow = eng.frame_flow(c['x'], c['geom'][0, :4], P.flow_refs(T, 1), search=SEARCH)['flow']
    assert torch.equal(flow[:, 0], c['flow'])      # slot 0 of the pooling's layout IS the frame before
    pooled = eng.hm_flow_pool(c['hm'], flow, P.flow_weights(1))
    seq = eng.seq_filter(pooled, SIGMA, RHO, centre=c['centre'])
    torch.cuda.synchronize()
    _check(got, c['plain'], seq, 'filter', c['geom'], c['centre'], extra=('flow',))


@pytest.mark.parametrize('mode', ['filter', 'viterbi'])
def test_flow_centre_off_changes_nothing(world, mode):
    eng, c = world
    a = P.predict_sequence(eng, c['frames'], mode=mode, sigma=SIGMA, rho=RHO, batch_size=4, keep_maps=True)
    b = P.predict_sequence(eng, c['frames'], mode=mode, sigma=SIGMA, rho=RHO, batch_size=4, keep_maps=True, flow_centre=False, flow_search=3)
    for ra, rb in zip(a, b):
        _same(ra, rb)


@pytest.mark.parametrize('split', [(1, 3), (2, 2)])
def test_any_split_of_the_tracker_is_the_one_call(world, split):
    eng, c = world
    whole = P.predict_sequence(eng, c['frames'], mode='filter', sigma=SIGMA, rho=RHO, batch_size=4, flow_centre=True, flow_search=SEARCH)
    tracker = P.SequenceTracker(eng, sigma=SIGMA, rho=RHO, batch_size=4, flow_centre=True, flow_search=SEARCH)
    pushed, lo = [], 0
    for n in split:
        pushed += tracker.push(c['frames'][lo:lo + n])
        lo += n
    assert len(pushed) == T
    for ra, rb in zip(pushed, whole):
        _same(ra, rb)
    assert tracker.last_frame is not None and torch.equal(tracker.last_frame, c['x'][-1])
    tracker.reset()
    assert tracker.last_frame is None and tracker.state is None
    again = tracker.push(c['frames'][:1])      # a new clip: no frame before, no belief
    _same(again[0], whole[0])
