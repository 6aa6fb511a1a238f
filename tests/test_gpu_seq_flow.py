"""Local motion in the prediction layer, on the GPU: predict.predict_sequence(flow=N) on a five-frame clip of a rendered person who
moves (dataset.render_clip), an engine with synthetic parameters.  The track must be the same mode of Engine.seq_* run on Engine.hm_flow_pool of the
kept maps and Engine.frame_flow of the kept frames, bit for bit; 'flow' must be the arg-max of the pooled maps; flow = 0 must change nothing."""
import os

import numpy as np
import pytest
import torch
from numpy.testing import assert_array_equal

import frame_flow_ref as FF
import joint_cnn_mrf_amd  # noqa: F401
from joint_cnn_mrf_amd import dataset, synth
from joint_cnn_mrf_amd import predict as P
from joint_cnn_mrf_amd.evaluation import fit_to_source

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
SIGMA, RHO, T = 2.0, 0.1, 5
KEYS = {'filter': ('coords', 'norm', 'reset'), 'viterbi': ('path', 'maxes', 'breaks'), 'marginal': ('coords', 'conf', 'norm', 'reset', 'cut')}


@pytest.fixture(scope='module')
def world():
    """The engine, the clip, pass 1 with the maps and the frames kept, and per N the flow and the pooled maps of the engine's own entries on them
    -- computed once, read by every test."""
    from joint_cnn_mrf_amd.engine import Engine
    p = synth.make_pd_params(debug=True)
    p.update(synth.make_sm_params(synth.synthetic_priors(), kind='init'))
    eng = Engine(device=0).load_params(p)
    poses = np.load(os.path.join(HERE, 'golden', 'flic_train_xy.npy'))
    x = dataset.render_clip(eng, np.random.RandomState(3), poses[10], poses[500], T, poses[20])[0]
    torch.cuda.synchronize()
    frames = [x[t] for t in range(T)]
    plain = P.predict_images(eng, frames, use_sm=True, batch_size=4, keep_maps=True, keep_frames=True)
    hm = torch.stack([r['maps']['sm'] for r in plain]).contiguous()
    geom = np.array([r['geom'] for r in plain], np.int64)
    pooled = {}
    for N, search in ((1, 8), (2, 5)):
        flow = eng.frame_flow(x, geom[0, :4], P.flow_refs(T, N), search=search)
        pooled[N] = (search, flow, eng.hm_flow_pool(hm, flow['flow'], P.flow_weights(N)))
    torch.cuda.synchronize()
    yield eng, {'x': x, 'frames': frames, 'plain': plain, 'hm': hm, 'geom': geom, 'pooled': pooled}
    eng.close()


def _points(cells, geom):
    return fit_to_source(cells.cpu().numpy().transpose(0, 2, 1).astype(np.float64) * P.STRIDE, geom)


def test_the_clip_moves_and_the_engine_entries_agree_with_the_restatement(world):
    eng, c = world
    assert c['x'].shape == (T, 480, 720, 3) and tuple(c['geom'][0]) == (0, 0, 480, 720, 480, 720)
    search, flow, pooled = c['pooled'][1]
    f = flow['flow'].cpu().numpy()
    assert f.shape == (T, 2, 60, 90, 2) and f[1:, 0].any() and f[:-1, 1].any()      # the person moves; the background rests
    assert not f[0, 0].any() and not f[-1, 1].any() and (f == 0).all(axis=-1).mean() > 0.5
    want = FF.frame_flow(c['x'][:2].cpu().numpy(), (0, 0, 480, 720), search, np.array([[1], [0]], np.int32))      # one pair of the clip, restated
    assert_array_equal(f[0, 1], want[0][0, 0])
    assert_array_equal(f[1, 0], want[0][1, 0])
    hm = c['hm'][:2].cpu().numpy()
    two = np.zeros((2, 2, 60, 90, 2), np.int32)
    two[0, 1], two[1, 0] = want[0][0, 0], want[0][1, 0]
    got = eng.hm_flow_pool(c['hm'][:2].contiguous(), torch.as_tensor(two, device='cuda:0'), (1.0, 1.0))
    torch.cuda.synchronize()
    assert_array_equal(got.cpu().numpy().view(np.uint32), FF.hm_flow_pool(hm, two, (1.0, 1.0)).view(np.uint32))


@pytest.mark.parametrize('mode,N,fit', [('filter', 1, 0), ('viterbi', 2, 0), ('marginal', 1, 0), ('filter', 2, 2)])
def test_track_is_the_scan_on_the_pooled_maps(world, mode, N, fit):
    eng, c = world
    search, flow, pooled = c['pooled'][N]
    got = P.predict_sequence(eng, c['frames'], mode=mode, sigma=SIGMA, rho=RHO, batch_size=4, flow=N, flow_search=search, fit_iters=fit)
    sigma, rho = SIGMA, RHO
    if fit:
        est = P.seq_fit(eng, pooled, SIGMA, RHO, iters=fit)
        sigma, rho = est['sigma'], est['rho']
        assert_array_equal(got[0]['seq_fit']['sigma'], sigma)
    seq = {'filter': eng.seq_filter, 'viterbi': eng.seq_viterbi, 'marginal': eng.seq_smooth}[mode](pooled, sigma, rho)
    torch.cuda.synchronize()
    pts, inside = _points(seq[KEYS[mode][0]], c['geom'])
    fpts, finside = _points(eng.argmax_coords(pooled), c['geom'])
    for t, (g, a) in enumerate(zip(got, c['plain'])):
        assert set(g) == (set(a) - {'maps'}) | {'track', 'flow'} | ({'seq_fit'} if fit and t == 0 else set()) and g['track']['mode'] == mode
        for k in set(a) - {'maps'}:      # every earlier key keeps its value
            assert_array_equal(np.asarray(g[k]), np.asarray(a[k]))
        assert_array_equal(g['track']['points'], pts[t])
        assert_array_equal(g['track']['inside'], inside[t])
        for k in KEYS[mode][1:]:
            assert_array_equal(g['track'][k], seq[k][t].cpu().numpy())
        assert set(g['flow']) == {'n', 'search', 'points', 'inside'} and g['flow']['n'] == N and g['flow']['search'] == search
        assert_array_equal(g['flow']['points'], fpts[t])
        assert_array_equal(g['flow']['inside'], finside[t])


def test_kept_maps_and_weights(world):
    eng, c = world
    search, flow, pooled = c['pooled'][1]
    kept = P.predict_sequence(eng, c['frames'], mode='filter', sigma=SIGMA, rho=RHO, batch_size=4, flow=1, keep_maps=True)
    for t, r in enumerate(kept):
        assert_array_equal(r['maps']['pooled'].cpu().numpy().view(np.uint32), pooled[t].cpu().numpy().view(np.uint32))
        assert_array_equal(r['maps']['frame'].cpu().numpy(), c['x'][t].cpu().numpy())
        assert_array_equal(r['maps']['sm'].cpu().numpy(), c['hm'][t].cpu().numpy())
    assert not torch.equal(pooled, c['hm'])
    own = P.predict_sequence(eng, c['frames'], mode='filter', sigma=SIGMA, rho=RHO, batch_size=4, flow=1, flow_weights=(1.0, 0.0), keep_maps=True)
    plain = P.predict_sequence(eng, c['frames'], mode='filter', sigma=SIGMA, rho=RHO, batch_size=4)
    for a, b in zip(own, plain):      # w = [1, 0]: the pooled maps are the maps
        assert_array_equal(a['maps']['pooled'].cpu().numpy().view(np.uint32), a['maps']['sm'].cpu().numpy().view(np.uint32))
        for k in b['track']:
            assert_array_equal(np.asarray(a['track'][k]), np.asarray(b['track'][k]))


@pytest.mark.parametrize('mode', ['filter', 'viterbi', 'marginal'])
def test_flow_zero_changes_nothing(world, mode):
    eng, c = world
    a = P.predict_sequence(eng, c['frames'], mode=mode, sigma=SIGMA, rho=RHO, batch_size=4, keep_maps=True)
    b = P.predict_sequence(eng, c['frames'], mode=mode, sigma=SIGMA, rho=RHO, batch_size=4, keep_maps=True, flow=0, flow_search=3)

    def same(u, v):
        if isinstance(u, dict):
            assert isinstance(v, dict) and list(u) == list(v)
            for k in u:
                same(u[k], v[k])
        elif isinstance(u, (list, tuple)) and u and isinstance(u[0], dict):
            assert len(u) == len(v)
            for i, j in zip(u, v):
                same(i, j)
        elif isinstance(u, torch.Tensor):
            assert u.dtype == v.dtype and torch.equal(u.view(torch.uint8), v.view(torch.uint8))
        else:
            i, j = np.asarray(u), np.asarray(v)
            assert i.dtype == j.dtype and i.shape == j.shape and i.tobytes() == j.tobytes()
    for ra, rb in zip(a, b):
        same(ra, rb)


def test_flow_with_camera_carries_both(world):
    eng, c = world
    search, flow, pooled = c['pooled'][1]
    got = P.predict_sequence(eng, c['frames'], mode='viterbi', sigma=SIGMA, rho=RHO, batch_size=4, flow=1, camera=True)
    cam = P.predict_sequence(eng, c['frames'], mode='viterbi', sigma=SIGMA, rho=RHO, batch_size=4, camera=True)
    shift = np.array([r['camera']['shift'] for r in cam], np.int32)
    seq = eng.seq_viterbi(pooled, SIGMA, RHO, shift=shift)
    torch.cuda.synchronize()
    pts, _ = _points(seq['path'], c['geom'])
    for t, (g, k) in enumerate(zip(got, cam)):
        assert set(g) == set(k) | {'flow'} and g['camera'] == k['camera']
        assert_array_equal(g['track']['points'], pts[t])


def test_refused_combinations_raise(world):
    eng, c = world
    frames = c['frames'][:2]
    for kw in ({'mode': 'lag', 'lag': 2, 'flow': 1}, {'flow': 5}, {'flow': 1, 'flow_search': 0}, {'flow': 1, 'flow_search': 17}, {'flow': 2, 'flow_weights': (1.0, 1.0)}):
        with pytest.raises(ValueError, match='flow'):
            P.predict_sequence(eng, frames, batch_size=4, **kw)
    with pytest.raises(ValueError, match='flow'):
        P.predict_sequence_zoom(eng, frames, flow=1)
    with pytest.raises(ValueError, match='flow'):
        P.predict_sequence_people(eng, frames, 2, flow=1)
