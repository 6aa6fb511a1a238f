"""The torso map from the part detector on the GPU (csrc/torso_infer.hip): jcm_torso_infer against the float64 restatement
tests/torso_ref.py (pinned by tests/test_torso_cpu.py), the blob bit for bit against data.target_heat_maps, then Engine.torso_sm,
forward(torso='infer'), forward(people=M), the towers and the command line, each against the composition of the calls that existed before.

One route exists, "torso_algo" = 1 (direct); the frequency-domain route of the issue is not shipped, so there is no route-agreement test."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch
from numpy.testing import assert_array_equal

import torso_ref as T
from cli_util import run_cli
import joint_cnn_mrf_amd  # noqa: F401
from joint_cnn_mrf_amd import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K, H, W = T.K, T.H, T.W
ROUTES = {'direct': 1}


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), device='cuda:0')


def _bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and bool((_bits(a) == _bits(b)).all())


def _pd_params(debug=True):
    return synth.make_pd_params(debug=debug, bn='trained', conv6_gain=8.0)


# name -> (probabilities, spatial-model parameters, may an image be undecided?)
def _inputs():
    trained = T.trained_params()
    scene_prob, scene_params, _, _ = T.scene()
    sharp_prob, sharp_params, _, _ = T.sharp_scene()
    out = {'noise%d' % B: (T.noise_prob(B, seed), 'trained', True) for B, seed in T.NOISE_SEEDS.items()}
    out.update(corners=(T.corner_prob(), 'corner', False), underflow=(T.underflow_prob(3, 7), 'trained', True), scene=(scene_prob, 'scene', False),
               sharp=(sharp_prob, 'sharp', False))
    return out, {'trained': trained, 'corner': T.corner_params(), 'scene': scene_params, 'sharp': sharp_params, 'flat': T.flat_params()}


@pytest.fixture(scope='module')
def world():
    """fp32 handles at --debug width, one per set of spatial-model parameters; the inputs; and the float64 reference of every input, computed
    once."""
    from joint_cnn_mrf_amd.engine import Engine
    inputs, params = _inputs()
    engines = {k: Engine(device=0).load_params(dict(_pd_params(), **p)) for k, p in params.items()}
    ref = {}
    for name, (prob, kind, _) in inputs.items():
        C = T.corr64(prob, params[kind])
        ref[name] = (T.energy64(C),) + T.argmax_cells(T.energy64(C))
    yield engines, inputs, params, ref
    for e in engines.values():
        e.close()


def _run(eng, prob, **kw):
    r = eng.torso_infer(_dev(prob), **kw)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in r.items()}


@pytest.mark.parametrize('route', sorted(ROUTES))
def test_energy(world, route):
    """max |E_gpu - E_f64| over noise probabilities (B = 1, 3, 33), corner peaks, underflowed maps, the planted scenes; trained-like, sharp and
    Gaussian parameters.  Measured on the MI355X, direct route: see torso_ref.ENERGY_MEASURED; the bound is 4 x that.  The cell equals the
    restatement's wherever the float64 top-2 gap exceeds twice the bound; at most 10 % of the noise images may fall under it, none of the others.
    The cell is also the first-occurrence arg-max of the energy the device returns (the tie rule on the device's own numbers), and the blob is
    data.target_heat_maps at the returned cell, bit for bit."""
    engines, inputs, _, ref = world
    worst = 0.0
    for name, (prob, kind, may_skip) in sorted(inputs.items()):
        eng = engines[kind]
        eng.set_option('torso_algo', ROUTES[route])
        got = _run(eng, prob, want_energy=True)
        E64, cell64, gap = ref[name]
        err = float(np.abs(got['energy'].astype(np.float64) - E64).max())
        worst = max(worst, err)
        print('torso energy %-10s %-7s max |E_gpu - E_f64| = %.3e   (E in [%.1f, %.1f], min gap %.3e)' % (name, route, err, E64.min(), E64.max(), gap.min()))
        assert err <= T.ENERGY_BOUND[route], (name, err)
        decided = gap > 2 * T.ENERGY_BOUND[route]
        assert (~decided).mean() <= (0.10 if may_skip else 0.0), (name, gap)
        assert_array_equal(got['cell'][decided], cell64[decided], err_msg=name)
        flat = got['energy'].reshape(len(prob), -1).argmax(axis=1)
        assert_array_equal(got['cell'], np.stack([flat // W, flat % W], axis=1), err_msg=name)
        assert_array_equal(got['torso'].view(np.uint32), T.blobs(got['cell']).view(np.uint32), err_msg=name)
        lean = _run(eng, prob)
        assert sorted(lean) == ['cell', 'torso'] and np.array_equal(lean['cell'], got['cell']) and np.array_equal(lean['torso'], got['torso'])
    print('torso energy worst %-7s %.3e (bound %.3e)' % (route, worst, T.ENERGY_BOUND[route]))


def test_ties_and_corners(world):
    """A constant prior makes C_j(t) the same operations on the same numbers for every t: an exact tie over the whole map goes to (0,0).  Two
    equal planted skeletons are equal to rounding only (torso_ref.tie_scene): the cell is one of the two.  The corner inputs put the arg-max,
    and so the cut blob, into each corner."""
    engines, inputs, _, _ = world
    got = _run(engines['flat'], T.noise_prob(3, 9), want_energy=True)
    assert (got['energy'] == got['energy'][:, :1, :1]).all()
    assert_array_equal(got['cell'], np.zeros((3, 2), np.int32))
    prob, _, ta, tb = T.tie_scene()
    cell = tuple(_run(engines['scene'], prob)['cell'][0])
    assert cell in (ta, tb)
    got = _run(engines['corner'], T.corner_prob())
    assert got['cell'].tolist() == [[0, 0], [0, W - 1], [H - 1, 0], [H - 1, W - 1]]
    assert [float(t.sum()) for t in got['torso']] == [9 / 16] * 4


def test_cells_in_writes_blobs(world):
    """cells_in: the blob at the given cells, bit for bit; border cells are cut, out-of-range cells clamped first; 33 cells cross any packing."""
    eng = world[0]['flat']
    rs = np.random.RandomState(3)
    cells = np.concatenate([np.array([(0, 0), (59, 89), (0, 89), (59, 0), (30, 0), (0, 45), (-1, -1), (60, 90), (-2 ** 31, 2 ** 31 - 1), (17, 1000)]),
                            np.stack([rs.randint(0, H, 23), rs.randint(0, W, 23)], axis=1)]).astype(np.int32)
    r = eng.torso_infer(None, cells=_dev(cells))
    torch.cuda.synchronize()
    assert_array_equal(r['torso'].cpu().numpy().view(np.uint32), T.blobs(cells).view(np.uint32))
    assert_array_equal(r['cell'].cpu().numpy(), np.stack([np.clip(cells[:, 0], 0, H - 1), np.clip(cells[:, 1], 0, W - 1)], axis=1))


def test_argument_contract(world):
    """Wrong geometry, B = 0 and a null prob are JCM_ERR_ARG and leave sentinel-filled outputs untouched; null energy or torso is accepted; a
    handle without spatial model or before finalize is JCM_ERR_STATE; the option has one value."""
    from joint_cnn_mrf_amd.engine import Engine
    eng = world[0]['trained']
    lib, p = eng._lib, Engine._p
    prob = _dev(T.noise_prob(2, 4))

    def call(h, B=2, HH=H, WW=W, KK=K, prob_t=prob, cells=None, energy=True, cell=True, torso=True):
        out = {'energy': torch.full((2, H, W), -7.0, device='cuda:0'), 'cell': torch.full((2, 2), -7, dtype=torch.int32, device='cuda:0'),
               'torso': torch.full((2, H, W, 1), -7.0, device='cuda:0')}
        st = lib.jcm_torso_infer(h, p(prob_t), B, HH, WW, KK, p(cells), p(out['energy'] if energy else None), p(out['cell'] if cell else None),
                                 p(out['torso'] if torso else None))
        torch.cuda.synchronize()
        return st, {k: bool((v == -7).all()) for k, v in out.items()}
    untouched = {'energy': True, 'cell': True, 'torso': True}
    for kw in (dict(HH=61), dict(WW=91), dict(KK=10), dict(KK=8), dict(HH=120, WW=180), dict(B=0), dict(B=-1), dict(prob_t=None), dict(cell=False),
               dict(cells=_dev(np.zeros((2, 2), np.int32)), torso=False)):
        assert call(eng._h, **kw) == (1, untouched), kw
        assert 'torso_infer' in joint_cnn_mrf_amd._lib.last_error()
    assert call(eng._h, energy=False) == (0, {'energy': True, 'cell': False, 'torso': False})
    assert call(eng._h, torso=False) == (0, {'energy': False, 'cell': False, 'torso': True})
    assert call(eng._h, cells=_dev(np.zeros((2, 2), np.int32))) == (0, {'energy': True, 'cell': True, 'torso': False})
    bare = Engine(device=0).load_params(_pd_params())
    fresh = Engine(device=0)
    try:
        assert call(bare._h) == (2, untouched) and call(fresh._h) == (2, untouched)
    finally:
        bare.close()
        fresh.close()
    v = ctypes.c_int64(-1)
    assert lib.jcm_get_option(eng._h, b'torso_algo', ctypes.byref(v)) == 0 and v.value == 1
    assert lib.jcm_set_option(eng._h, b'torso_algo', 1) == 0
    for bad in (0, 2, 3):
        assert lib.jcm_set_option(eng._h, b'torso_algo', bad) == 1 and 'torso_algo' in joint_cnn_mrf_amd._lib.last_error()
    assert eng.get_option('torso_algo') == 1


def test_scene_at_the_map_level(world):
    """torso_sm on the planted scene: the inferred torso is person A's, so sm_coords equal those of the spatial model given the planted blob,
    and the result is the composition torso_infer -> spatial_model -> softmax_argmax, bit for bit."""
    engines, inputs, _, _ = world
    import pose_ref
    eng = engines['scene']
    prob = _dev(inputs['scene'][0])
    r = eng.torso_sm(prob)
    planted = _dev(T.blobs([pose_ref.TORSO_A]))
    sm_prob, sm_coords = eng.softmax_argmax(eng.spatial_model(torch.cat([prob, planted], dim=3)))
    torch.cuda.synchronize()
    assert r['torso_cell'].tolist() == [list(pose_ref.TORSO_A)] and _same_bits(r['torso'], planted)
    assert _same_bits(r['sm_coords'], sm_coords) and _same_bits(r['sm_prob'], sm_prob)


def test_people(world):
    """people=2 on the sharp two-person scene: count 2, the cells A's and B's, slot k the spatial model given slot k's blob, bit for bit; one
    person: count 1 and slot 1 all -1 / 0; people=1 is the plain call."""
    engines, _, _, _ = world
    eng = engines['sharp']
    prob2, _, ta, tb = T.sharp_scene(True)
    prob1 = T.sharp_scene(False)[0]
    prob = _dev(np.concatenate([prob2, prob1, prob2]))
    r = eng.torso_sm(prob, people=2)
    plain = eng.torso_sm(prob)
    one = eng.torso_sm(prob, people=1)
    torch.cuda.synchronize()
    pe = r['people']
    assert pe['count'].tolist() == [2, 1, 2]
    assert pe['torso_cell'].tolist() == [[list(ta), list(tb)], [list(ta), [-1, -1]], [list(ta), list(tb)]]
    assert tuple(pe['sm_coords'].shape) == (3, 2, 2, K) and tuple(pe['sm_prob'].shape) == (3, 2, H, W, K) and tuple(pe['torso_score'].shape) == (3, 2)
    assert bool((pe['sm_coords'][1, 1] == -1).all()) and bool((pe['sm_prob'][1, 1] == 0).all()) and float(pe['torso_score'][1, 1]) == 0.0
    assert bool((pe['torso_score'][:, 0] > pe['torso_score'][:, 1]).all())
    for k, cell in enumerate((ta, tb)):
        blob = _dev(np.repeat(T.blobs([cell]), 3, axis=0))
        sm_prob, sm_coords = eng.softmax_argmax(eng.spatial_model(torch.cat([prob, blob], dim=3)))
        torch.cuda.synchronize()
        for b in ((0, 1, 2) if k == 0 else (0, 2)):
            assert _same_bits(pe['sm_coords'][b, k], sm_coords[b]) and _same_bits(pe['sm_prob'][b, k], sm_prob[b]), (k, b)
    for name in ('sm_coords', 'sm_prob', 'torso_cell', 'torso'):
        assert _same_bits(r[name], plain[name]) and _same_bits(one[name], plain[name]), name
    assert 'people' not in one and sorted(one) == sorted(plain)
    lean = eng.torso_sm(prob, people=2, want_prob=False)
    torch.cuda.synchronize()
    assert 'sm_prob' not in lean and 'sm_prob' not in lean['people'] and _same_bits(lean['people']['sm_coords'], pe['sm_coords'])
    with pytest.raises(ValueError, match='people'):
        eng.torso_sm(prob, people=5)


def _check_forward(e, x, t_given):
    """forward(torso='infer') on images: pd_* are the bits of forward(use_sm=False), sm_* those of forward(x, torso=r['torso'])."""
    r = e.forward(x, 'infer', use_sm=True)
    pd = e.forward(x, None, use_sm=False)
    given = e.forward(x, r['torso'], use_sm=True)
    torch.cuda.synchronize()
    assert sorted(r) == ['pd_coords', 'pd_prob', 'sm_coords', 'sm_prob', 'torso', 'torso_cell']
    for name in ('pd_coords', 'pd_prob'):
        assert _same_bits(r[name], pd[name]) and _same_bits(r[name], given[name]), name
    for name in ('sm_coords', 'sm_prob'):
        assert _same_bits(r[name], given[name]), name
    want = e.torso_infer(r['pd_prob'])
    torch.cuda.synchronize()
    assert _same_bits(r['torso'], want['torso']) and _same_bits(r['torso_cell'], want['cell'])
    assert_array_equal(r['torso'].cpu().numpy().view(np.uint32), T.blobs(r['torso_cell'].cpu().numpy()).view(np.uint32))
    return r


def test_forward_infer_fp32(world):
    """fp32 handle at --debug width, float and byte images; peaks, decode, people, the lean call, the refusals and an unchanged default."""
    e = world[0]['trained']
    k8 = np.random.RandomState(5).randint(0, 256, (2, 480, 720, 3)).astype(np.uint8)
    x = _dev(k8.astype(np.float32) / np.float32(255))
    r = _check_forward(e, x, None)
    r8 = _check_forward(e, _dev(k8), None)
    for name in r:
        assert _same_bits(r[name], r8[name]), name
    full = e.forward(x, 'infer', peaks=3, decode=True)
    lean = e.forward(x, 'infer', peaks=3, decode=True, want_prob=False)
    torch.cuda.synchronize()
    assert sorted(full) == sorted(list(r) + ['pd_peaks', 'sm_peaks', 'pose'])
    assert sorted(lean) == ['pd_coords', 'pd_peaks', 'pose', 'sm_coords', 'sm_peaks', 'torso', 'torso_cell']
    for name in r:
        assert _same_bits(full[name], r[name]), name
    pose = e.pose_decode(torch.cat([r['pd_prob'], r['torso']], dim=3), full['pd_peaks'])
    torch.cuda.synchronize()
    for f in pose:
        assert _same_bits(full['pose'][f], pose[f]) and _same_bits(lean['pose'][f], pose[f]), f
    for f in full['sm_peaks']:
        assert _same_bits(lean['sm_peaks'][f], full['sm_peaks'][f]), f
    two = e.forward(x, 'infer', people=2, peaks=2, decode=True)
    torch.cuda.synchronize()
    assert tuple(two['people']['sm_coords'].shape) == (2, 2, 2, K) and tuple(two['pose']['index'].shape) == (2, 2, K)
    assert bool((two['people']['count'] >= 1).all()) and _same_bits(two['people']['sm_coords'][:, 0].contiguous(), two['sm_coords'])
    t = _dev(synth.make_torso(2, seed=3))
    for kw in (dict(flip_test=True), dict(use_sm=False), dict(people=0), dict(people=5)):
        with pytest.raises(ValueError):
            e.forward(x, 'infer', **kw)
    with pytest.raises(ValueError):
        e.forward(x, 'guess')
    with pytest.raises(ValueError):
        e.forward(x, t, people=2)
    with pytest.raises(ValueError, match='torso'):
        e.forward(x, None, use_sm=True)
    from joint_cnn_mrf_amd import multiscale as MS
    with pytest.raises(ValueError, match='multi-scale'):
        MS.get_predictions(e, k8.astype(np.float32), synth.make_targets(2, seed=42), torso='infer')


def test_forward_infer_bf16():
    """A bf16 handle.  At the model's full width: jcm_finalize refuses the --debug widths on a bf16 handle (conv2 has Cin = 16 there, the bf16
    kernels need Cin % 32 == 0), as tests/test_gpu_options.py notes.  One image."""
    from joint_cnn_mrf_amd.engine import Engine
    e = Engine(device=0, precision='bf16').load_params(dict(_pd_params(debug=False), **T.trained_params()))
    try:
        _check_forward(e, _dev(np.random.RandomState(6).randint(0, 256, (1, 480, 720, 3)).astype(np.uint8)), None)
    finally:
        e.close()


def test_towers_infer(world):
    """Two in-process towers on the one device, one image each, against one engine on both images."""
    from joint_cnn_mrf_amd.dist import Towers
    e = world[0]['trained']
    xf = np.random.RandomState(8).random_sample((2, 480, 720, 3)).astype(np.float32)
    tw = Towers(dict(_pd_params(), **T.trained_params()), [0, 0])
    try:
        got = tw.forward(xf, 'infer', use_sm=True, want_prob=True, people=2)
        want = e.forward(_dev(xf), 'infer', use_sm=True, people=2)
        torch.cuda.synchronize()
        assert sorted(got) == sorted(want)
        for name in want:
            if name == 'people':
                for f in want[name]:
                    assert _same_bits(got[name][f], want[name][f]), f
            else:
                assert _same_bits(got[name], want[name]), name
    finally:
        tw.close()


# ------------------------------------------------------------------ the command line
def test_cli_infer_torso(tmp_path):
    import scipy.io
    mat = str(tmp_path / 'P.mat')
    r = run_cli(['--synthetic', '--debug', '--use_sm', '--infer_torso', '--people', '2', '--gpus', '0', '--batch_size', '2', '--synthetic_size', '4',
              '--predictions', mat], str(tmp_path))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line['infer_torso'] is True and line['n_images'] == 4 and line['people'] == 2
    assert isinstance(line['torso_cell_dist'], float) and 0 <= line['torso_cell_dist'] <= float(np.hypot(H, W))
    m = scipy.io.loadmat(mat)
    assert m['flic_torso_cell'].shape == (4, 2) and m['flic_pred_sm'].shape == (2, K, 4)
    assert (m['flic_torso_cell'] >= 0).all() and (m['flic_torso_cell'][:, 0] < H).all() and (m['flic_torso_cell'][:, 1] < W).all()
    assert m['flic_people_sm'].shape == (4, 2, 2, K) and m['flic_people_count'].reshape(-1).shape == (4,)
    assert_array_equal(m['flic_people_sm'][:, 0].transpose(1, 2, 0), m['flic_pred_sm'])


def test_cli_refusals(tmp_path):
    for extra, word in ((['--train', '--infer_torso', '--use_sm'], '--infer_torso'), (['--infer_torso', '--use_sm', '--multiscale'], '--multiscale'),
                        (['--use_sm', '--people', '2'], '--infer_torso')):
        r = run_cli(['--debug', '--synthetic', '--gpus', '0'] + extra, str(tmp_path))
        assert r.returncode != 0 and word in r.stderr, extra
