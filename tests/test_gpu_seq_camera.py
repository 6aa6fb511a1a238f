"""Camera pans in the prediction layer, on the GPU: predict.predict_sequence(camera=True) and SequenceTracker(camera=True) on
six-frame clips of rendered people seen by a panning camera (dataset.render_clip_pan), an engine with synthetic parameters.  The track must be
the moving scan on the kept maps with the shifts of the RESTATED displacement (tests/frame_shift_ref.py), bit for bit; the reported displacement
must be the clip's true one; a camera that stands still must change nothing."""
import os

import numpy as np
import pytest
import torch
from numpy.testing import assert_array_equal

import frame_shift_ref as FR
import joint_cnn_mrf_amd  # noqa: F401
from joint_cnn_mrf_amd import dataset, synth
from joint_cnn_mrf_amd import predict as P
from joint_cnn_mrf_amd.evaluation import fit_to_source

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
PAN = np.array([[0, 0], [4, -6], [-3, 8], [12, -12], [-5, 5], [-9, 17]])
MARGIN = (16, 24)
SIGMA, RHO = 2.0, 0.1
KEYS = {'filter': ('norm', 'reset'), 'viterbi': ('maxes', 'breaks')}


@pytest.fixture(scope='module')
def world():
    """The engine, the panned clip and the still clip of the same scene, their true displacements, pass 1 of both with the maps kept, and the
    restated displacement of the panned clip -- computed once, read by every test."""
    from joint_cnn_mrf_amd.engine import Engine
    p = synth.make_pd_params(debug=True)
    p.update(synth.make_sm_params(synth.synthetic_priors(), kind='init'))
    eng = Engine(device=0).load_params(p)
    poses = np.load(os.path.join(HERE, 'golden', 'flic_train_xy.npy'))
    clips = {}
    for name, pan in (('pan', PAN), ('still', PAN * 0)):
        x, xy, inside, disp = dataset.render_clip_pan(eng, np.random.RandomState(3), poses[10], poses[500], len(PAN), pan, MARGIN, poses[20])
        torch.cuda.synchronize()
        frames = [x[t] for t in range(x.shape[0])]
        clips[name] = {'x': x, 'frames': frames, 'xy': xy, 'inside': inside, 'disp': disp,
                       'plain': P.predict_images(eng, frames, use_sm=True, batch_size=4, keep_maps=True)}
    clips['pan']['ref'] = FR.frame_shift(clips['pan']['x'].cpu().numpy(), (0, 0, 480, 720), 8)
    yield eng, clips
    eng.close()


def test_panned_clip_geometry(world):
    _, clips = world
    c, s = clips['pan'], clips['still']
    assert c['x'].shape == (6, 480, 720, 3) and c['x'].dtype == torch.uint8 and c['xy'].shape == (6, 2, 9) and c['inside'].shape == (6, 9)
    assert_array_equal(c['disp'][1:], PAN[1:])
    assert not c['disp'][0].any() and not s['disp'].any()
    o = dataset.pan_origins(PAN, MARGIN, 6)
    assert_array_equal(c['xy'][:, 0] + o[:, 1, None], s['xy'][:, 0] + MARGIN[1])      # one scene: the joints agree on the canvas
    assert_array_equal(c['xy'][:, 1] + o[:, 0, None], s['xy'][:, 1] + MARGIN[0])
    x, y = c['x'].cpu().numpy(), s['x'].cpu().numpy()
    assert_array_equal(x[0], y[0])                                                    # pan_0 = 0: the same crop
    assert_array_equal(x[1, :400, 100:], y[1, 4:404, 94:714])                         # frame 1 is the still frame 1 moved by (4, -6)
    with pytest.raises(ValueError, match='leaves the canvas'):
        dataset.render_clip_pan(None, np.random.RandomState(3), None, None, 2, np.array([[17, 0], [0, 0]]), MARGIN)


def test_camera_disp_is_the_true_displacement(world):
    eng, clips = world
    for name in ('pan', 'still'):
        c = clips[name]
        got = P.predict_sequence(eng, c['frames'], mode='filter', sigma=SIGMA, rho=RHO, batch_size=4, camera=True)
        assert_array_equal(np.array([r['camera']['disp'] for r in got]), c['disp'])
    assert_array_equal(clips['pan']['ref'][0], clips['pan']['disp'])
    r = eng.frame_shift(clips['pan']['x'], (0, 0, 480, 720))
    torch.cuda.synchronize()
    assert_array_equal(r['disp'].cpu().numpy(), clips['pan']['ref'][0])
    assert_array_equal(r['sad'].cpu().numpy(), clips['pan']['ref'][1])


@pytest.mark.parametrize('mode', ['filter', 'viterbi'])
def test_track_is_the_moving_scan_on_the_kept_maps(world, mode):
    eng, clips = world
    c = clips['pan']
    got = P.predict_sequence(eng, c['frames'], mode=mode, sigma=SIGMA, rho=RHO, batch_size=4, camera=True)
    hm = torch.stack([r['maps']['sm'] for r in c['plain']]).contiguous()
    shift, _ = P.camera_shifts(c['ref'][0])
    assert shift.any()
    seq = (eng.seq_filter if mode == 'filter' else eng.seq_viterbi)(hm, SIGMA, RHO, shift=shift)
    torch.cuda.synchronize()
    cells = seq['coords' if mode == 'filter' else 'path'].cpu().numpy().transpose(0, 2, 1).astype(np.float64)
    pts, inside = fit_to_source(cells * P.STRIDE, np.array([r['geom'] for r in c['plain']], np.int64))
    for t, (g, a) in enumerate(zip(got, c['plain'])):
        assert set(g) == (set(a) - {'maps'}) | {'track', 'camera'} and g['track']['mode'] == mode
        for k in set(a) - {'maps'}:      # every earlier key keeps its value
            assert_array_equal(np.asarray(g[k]), np.asarray(a[k]))
        assert_array_equal(g['track']['points'], pts[t])
        assert_array_equal(g['track']['inside'], inside[t])
        for k in KEYS[mode]:
            assert_array_equal(g['track'][k], seq[k][t].cpu().numpy())
        assert g['camera'] == {'disp': tuple(int(v) for v in c['ref'][0][t]), 'shift': tuple(int(v) for v in shift[t]), 'sad': tuple(int(v) for v in c['ref'][1][t])}
    kept = P.predict_sequence(eng, c['frames'][:2], mode=mode, sigma=SIGMA, rho=RHO, batch_size=4, camera=True, keep_maps=True)
    assert_array_equal(kept[1]['maps']['frame'].cpu().numpy(), c['x'][1].cpu().numpy())
    assert 'frame' not in c['plain'][0]['maps']


@pytest.mark.parametrize('mode', ['filter', 'viterbi'])
def test_still_camera_changes_nothing(world, mode):
    eng, clips = world
    c = clips['still']
    a = P.predict_sequence(eng, c['frames'], mode=mode, sigma=SIGMA, rho=RHO, batch_size=4)
    b = P.predict_sequence(eng, c['frames'], mode=mode, sigma=SIGMA, rho=RHO, batch_size=4, camera=True)
    for ra, rb in zip(a, b):
        assert set(rb) == set(ra) | {'camera'} and rb['camera']['shift'] == (0, 0)
        assert set(ra['track']) == set(rb['track'])
        for k in ra['track']:
            assert_array_equal(np.asarray(ra['track'][k]), np.asarray(rb['track'][k]))


def test_tracker_split_equals_one_call(world):
    eng, clips = world
    c = clips['pan']
    whole = P.predict_sequence(eng, c['frames'], mode='filter', sigma=SIGMA, rho=RHO, batch_size=4, camera=True)
    tr = P.SequenceTracker(eng, sigma=SIGMA, rho=RHO, batch_size=4, camera=True)
    for _ in range(2):      # and again after reset(): nothing of the first clip is left
        parts = tr.push(c['frames'][:1]) + tr.push(c['frames'][1:3]) + tr.push(c['frames'][3:])
        assert tr.last_frame is not None
        for g, w in zip(parts, whole):
            assert g['camera'] == w['camera']
            for k in w['track']:
                assert_array_equal(np.asarray(g['track'][k]), np.asarray(w['track'][k]))
        tr.reset()
        assert tr.last_frame is None and tr.carry == (0, 0) and tr.state is None


def test_refused_combinations_raise(world):
    eng, clips = world
    frames = clips['pan']['frames'][:2]
    for kw in ({'mode': 'marginal'}, {'mode': 'lag', 'lag': 2}, {'mode': 'filter', 'fit_iters': 2}, {'mode': 'viterbi', 'camera_search': 17}):
        with pytest.raises(ValueError):
            P.predict_sequence(eng, frames, camera=True, batch_size=4, **kw)
    with pytest.raises(ValueError, match='camera'):
        P.predict_sequence_zoom(eng, frames, camera=True)
    with pytest.raises(ValueError, match='camera'):
        P.predict_sequence_people(eng, frames, 2, camera=True)
    with pytest.raises(ValueError, match='keep_maps'):
        P.predict_images(eng, frames, keep_frames=True)
