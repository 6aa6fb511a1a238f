"""Detection-rate curves on the GPU: jcm_det_curve (csrc/det_curve.hip) against the numpy restatement of evaluation.py:15-36
(tests/det_curve_ref.py, pinned by tests/test_det_curve_cpu.py) BIT FOR BIT -- every step is one correctly rounded float32 operation on
exactly representable integers, so any difference is a kernel fault, not a tolerance question -- then the accumulator, eval_error /
eval_curves on a --debug engine, the error paths and the command line."""
import json
import os

import numpy as np
import pytest
import torch

import det_curve_ref as R
from cli_util import run_cli
import joint_cnn_mrf_amd  # noqa: F401
from joint_cnn_mrf_amd import evaluation, synth
from joint_cnn_mrf_amd import main as M

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RADII = np.arange(1, 21)


@pytest.fixture(scope='module')
def eng():
    """A bare fp32 handle: the curve kernel needs no parameters."""
    from joint_cnn_mrf_amd.engine import Engine
    e = Engine(device=0)
    yield e
    e.close()


@pytest.fixture(scope='module')
def tower():
    """fp32 handle at --debug width with parameters, and 5 images with their targets."""
    from joint_cnn_mrf_amd.engine import Engine
    p = synth.make_pd_params(debug=True, bn='trained', conv6_gain=8.0)
    p.update(synth.make_sm_params(synth.synthetic_priors(), kind='trained'))
    e = Engine(device=0).load_params(p)
    yield e, synth.make_images(5, seed=41), synth.make_targets(5, seed=42)
    e.close()


def _dev(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), device='cuda:0', dtype=dtype)


def _run(eng, pred, y, radii, **kw):
    r = eng.det_curve(_dev(pred, torch.int32), _dev(y, torch.float32), radii, want_dist=True, want_true=True, **kw)
    torch.cuda.synchronize()
    return r['true_coords'].cpu().numpy(), r['norm_dist'].cpu().numpy(), r['hits'].cpu().numpy()


def _check(eng, pred, y, radii):
    true, nd, hits = _run(eng, pred, y, radii)
    w_true, w_nd, w_counts = R.det_curve(pred, y, radii)
    assert true.dtype == np.int32 and np.array_equal(true, w_true)
    assert R.same_floats(nd, w_nd), (nd, w_nd)
    assert hits.dtype == np.int32 and np.array_equal(hits, w_counts)
    return true, nd, hits


def _case(seed, B, H, W, K, C):
    rs = np.random.RandomState(seed)
    y = R.blob_targets(rs, B, H, W, C, noisy=(1, 4, C - 1))
    return R.displaced(rs, R.argmax_coords(y, K), H, W), y


# (B, HH, WW, K, C): 7*11*10 = 770 and 13*17*10 = 2210 floats per image are no multiples of 4: the scalar sweep.  6*37*10 = 2220 is one, with
# 222 % 4 = 2 pixels behind the last quad, at the model's channel count; 9x5x8 and 6x7x16 leave 1 and 2 pixels behind it.  60x90 is the model's
# map: more quads than threads.  K = C, K = 8 and K = 16 are the limits.
CASES = [(1, 7, 11, 9, 10), (3, 60, 90, 9, 10), (5, 13, 17, 9, 10), (2, 9, 5, 8, 8), (4, 60, 90, 9, 9), (2, 6, 7, 16, 16), (2, 6, 37, 9, 10)]


@pytest.mark.parametrize('shape', CASES, ids=lambda s: 'x'.join(map(str, s)))
def test_bit_equal_to_the_restatement(eng, shape):
    B, H, W, K, C = shape
    pred, y = _case(sum(shape), *shape)
    true, nd, hits = _check(eng, pred, y, RADII)
    assert 0 < hits.sum() < B * K * 20                        # the case exercises both outcomes
    want = eng.argmax_coords(_dev(y[..., :K]))                 # the library's own arg-max, bit for bit
    assert np.array_equal(true, want.cpu().numpy())


def test_one_radius_and_thirty_two_fractional_radii(eng):
    pred, y = _case(3, 5, 13, 17, 9, 10)
    _check(eng, pred, y, [7.5])
    _t, _nd, hits = _check(eng, pred, y, np.linspace(0.25, 31.25, 32))
    assert hits.shape == (9, 32) and (np.diff(hits, axis=1) >= 0).all()


def test_unaligned_targets_take_the_scalar_sweep(eng):
    """A view that starts 4 bytes into an allocation: 16-byte loads are not possible, the result is the same."""
    pred, y = _case(4, 2, 6, 8, 9, 10)
    flat = torch.zeros(y.size + 1, device='cuda:0')
    flat[1:] = _dev(y).reshape(-1)
    yv = flat[1:].view(2, 6, 8, 10)
    assert yv.data_ptr() % 16 == 4 and yv.is_contiguous()
    r = eng.det_curve(_dev(pred, torch.int32), yv, RADII, want_dist=True, want_true=True)
    w_true, w_nd, w_counts = R.det_curve(pred, y, RADII)
    assert np.array_equal(r['true_coords'].cpu().numpy(), w_true) and R.same_floats(r['norm_dist'].cpu().numpy(), w_nd)
    assert np.array_equal(r['hits'].cpu().numpy(), w_counts)


def _maps(cells, H=12, W=14, C=10):
    y = np.zeros((1, H, W, C), np.float32)
    for k, (r, c) in enumerate(cells):
        y[0, r, c, k] = 1
    return y


CELLS = [(0, 0), (3, 3), (4, 4), (5, 5), (6, 6), (7, 7), (8, 8), (6, 8), (9, 9)]


def test_edge_maps(eng):
    # two equal maxima: the lower flat index wins; all-zero, all-NaN and all -inf channels give (0,0); a NaN elsewhere never wins
    y = _maps(CELLS)
    y[0, 2, 13, 1] = 1
    y[0, 11, 0, 2] = 1
    y[0, :, :, 3] = 0
    y[0, :, :, 4] = np.nan
    y[0, :, :, 5] = -np.inf
    y[0, 0, 1, 6] = np.nan
    y[0, :, :, 8] = -np.inf                                   # NaN, NaN, then -inf only: the first -inf (-inf ties the start value, NaN never does)
    y[0, 0, :2, 8] = np.nan
    pred = np.array(CELLS, np.int32).T[None].copy()
    true, _nd, _h = _check(eng, pred, y, RADII)
    assert true[0, :, 8].tolist() == [0, 2]
    assert true[0, :, 1].tolist() == [2, 13] and true[0, :, 2].tolist() == [4, 4] and true[0, :, 6].tolist() == [8, 8]
    assert true[0, :, 3].tolist() == [0, 0] and true[0, :, 4].tolist() == [0, 0] and true[0, :, 5].tolist() == [0, 0]
    assert np.array_equal(true, eng.argmax_coords(_dev(y[..., :9])).cpu().numpy())
    # maxima in the last pixel of the map and in the last channel (K = C = 9: channel 8 is the last float of every pixel)
    last = list(CELLS)
    last[8] = (11, 13)
    last[3] = (11, 13)
    y = _maps(last, C=9)
    true, _nd, _h = _check(eng, np.array(CELLS, np.int32).T[None].copy(), y, RADII)
    assert true[0, :, 8].tolist() == [11, 13] and true[0, :, 3].tolist() == [11, 13]


def test_zero_torso_and_exact_equality(eng):
    # joints 0 and 7 on one cell: NaN where pred == true, inf elsewhere, no hit at any radius
    same = list(CELLS)
    same[0] = same[7] = (5, 5)
    pred = np.array(same, np.int32).T[None].copy()
    pred[0, 0, 2] += 2
    _t, nd, hits = _check(eng, pred, _maps(same), RADII)
    assert np.isnan(nd[0, 0]) and np.isposinf(nd[0, 2]) and hits.sum() == 0
    # torso exactly 10, one cell off: nd == 10.0, a hit at radius 10 and a miss at radius 9
    pred = np.array(CELLS, np.int32).T[None].copy()
    pred[0, 1, 2] += 1
    _t, nd, hits = _check(eng, pred, _maps(CELLS), RADII)
    assert nd[0, 2] == np.float32(10.0) and hits[2].tolist() == [0] * 9 + [1] * 11


def test_accumulation_and_the_accumulator(eng):
    pred, y = _case(11, 7, 13, 17, 9, 10)
    want = R.det_curve(pred, y, RADII)[2]
    one = eng.det_curve(_dev(pred, torch.int32), _dev(y), RADII)                     # hits=None starts from zero
    assert sorted(one) == ['hits'] and np.array_equal(one['hits'].cpu().numpy(), want)
    hits = torch.zeros(9, 20, dtype=torch.int32, device='cuda:0')
    for lo, hi in ((0, 3), (3, 7)):
        r = eng.det_curve(_dev(pred[lo:hi], torch.int32), _dev(y[lo:hi]), RADII, hits=hits)
        assert r['hits'] is hits
    assert np.array_equal(hits.cpu().numpy(), want)
    a = evaluation.DetCurve(eng)
    for lo, hi in ((0, 1), (1, 5), (5, 7)):
        a.update(_dev(pred[lo:hi], torch.int32), _dev(y[lo:hi]))
    assert a.n_images == 7 and np.array_equal(a.counts(), want) and np.array_equal(a.rates(), 100 * want / 7)
    b, c = evaluation.DetCurve(eng), evaluation.DetCurve(eng)
    b.update(_dev(pred[:2], torch.int32), _dev(y[:2]))
    c.update(_dev(pred[2:], torch.int32), _dev(y[2:]))
    b.merge(c)
    assert b.n_images == 7 and np.array_equal(b.counts(), want)
    assert a.as_dict(M.joint_names)['lwri'] == (100 * want[2] / 7).tolist() and a.rate(2, 10) == 100 * want[2, 9] / 7


def test_agrees_with_det_rate_from_coords(eng):
    """The number the repository already had: joint 2, radius 10, as a float32 mean -- the only difference is that rounding."""
    rs = np.random.RandomState(13)
    y = R.blob_targets(rs, 6, 60, 90, 10, noisy=(1, 4, 9))
    pred = R.displaced(rs, R.argmax_coords(y, 9), 60, 90, -2, 2)      # small offsets: 4 of the 6 left wrists lie within radius 10
    true, _nd, hits = _run(eng, pred, y, RADII)
    assert hits[2, 9] == 4
    old = float(evaluation.det_rate_from_coords(_dev(pred, torch.int32), _dev(true), 10, [2]))
    assert abs(old - 100 * hits[2, 9] / 6) <= 1e-4


def test_eval_error_feeds_curves_and_returns_the_same_numbers(tower):
    e, X, Y = tower
    plain = evaluation.eval_error(X, Y, e, 2, use_sm=True, joints=[2], det_radius=10)
    pd, sm = evaluation.DetCurve(e), evaluation.DetCurve(e)
    fed = evaluation.eval_error(X, Y, e, 2, use_sm=True, joints=[2], det_radius=10, curves=(pd, sm))
    assert np.array_equal(np.array(plain, np.float64).view(np.uint64), np.array(fed, np.float64).view(np.uint64))
    assert pd.n_images == 4 and sm.n_images == 4              # whole batches: the fifth image is dropped (get_next_batch)
    rs = [e.eval_forward(_dev(X[lo:lo + 2]), _dev(Y[lo:lo + 2]), use_sm=True, want_prob=False) for lo in (0, 2)]      # the same batches
    for curve, key in ((pd, 'pd_coords'), (sm, 'sm_coords')):
        coords = np.concatenate([r[key].cpu().numpy() for r in rs])
        assert np.array_equal(curve.counts(), R.det_curve(coords, Y[:4], RADII)[2])


def test_eval_curves_counts_every_image(tower):
    e, X, Y = tower
    pd, sm = evaluation.eval_curves(X, Y, e, 2, use_sm=True)
    assert pd.n_images == 5 and sm.n_images == 5              # batches of 2, 2 and 1
    c_pd, c_sm = [], []
    for lo in (0, 2, 4):                                      # engine.forward's coordinates of the same batches
        r = e.forward(_dev(X[lo:lo + 2]), _dev(Y[lo:lo + 2, :, :, 9:]), use_sm=True, want_prob=False)
        c_pd.append(r['pd_coords'].cpu().numpy())
        c_sm.append(r['sm_coords'].cpu().numpy())
    assert np.array_equal(pd.counts(), R.det_curve(np.concatenate(c_pd), Y, RADII)[2])
    assert np.array_equal(sm.counts(), R.det_curve(np.concatenate(c_sm), Y, RADII)[2])
    pd0, sm0 = evaluation.eval_curves(X[:3], Y[:3], e, 2, use_sm=False, radii=[5, 10])
    assert pd0.n_images == 3 and np.array_equal(pd0.counts(), sm0.counts()) and pd0.counts().shape == (9, 2)


def test_error_paths_launch_nothing(eng):
    hits = torch.full((9, 20), 7, dtype=torch.int32, device='cuda:0')

    def refused(pred, y, radii, match, h=None):
        with pytest.raises(RuntimeError, match=match):
            eng.det_curve(pred, y, radii, hits=h)
    y10 = torch.zeros(2, 6, 7, 10, device='cuda:0')
    refused(torch.zeros(2, 2, 7, dtype=torch.int32, device='cuda:0'), y10, RADII, r'jcm_det_curve failed.*K = 7',
            torch.full((7, 20), 7, dtype=torch.int32, device='cuda:0'))
    refused(torch.zeros(2, 2, 9, dtype=torch.int32, device='cuda:0'), torch.zeros(2, 6, 7, 8, device='cuda:0'), RADII, r'jcm_det_curve failed.*C = 8', hits)
    refused(torch.zeros(2, 2, 9, dtype=torch.int32, device='cuda:0'), torch.zeros(2, 6, 7, 17, device='cuda:0'), RADII, r'jcm_det_curve failed.*C = 17', hits)
    refused(torch.zeros(2, 2, 17, dtype=torch.int32, device='cuda:0'), torch.zeros(2, 6, 7, 17, device='cuda:0'), RADII, r'jcm_det_curve failed.*K = 17')
    refused(torch.zeros(2, 2, 9, dtype=torch.int32, device='cuda:0'), y10, [], r'jcm_det_curve failed.*R = 0')
    refused(torch.zeros(2, 2, 9, dtype=torch.int32, device='cuda:0'), y10, np.arange(33), r'jcm_det_curve failed.*R = 33')
    with pytest.raises(ValueError, match='y is on cpu'):      # a host tensor never reaches the library
        eng.det_curve(torch.zeros(2, 2, 9, dtype=torch.int32, device='cuda:0'), torch.zeros(2, 6, 7, 10), RADII, hits=hits)
    with pytest.raises(TypeError):
        eng.det_curve(torch.zeros(2, 2, 9, dtype=torch.int64, device='cuda:0'), y10, RADII, hits=hits)
    with pytest.raises(ValueError):
        eng.det_curve(torch.zeros(3, 2, 9, dtype=torch.int32, device='cuda:0'), y10, RADII, hits=hits)
    torch.cuda.synchronize()
    assert int((hits != 7).sum()) == 0


def _run_ok(args, cwd):
    r = run_cli(args, cwd)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return r.stdout


@pytest.mark.parametrize('multiscale', [False, True], ids=['single', 'multiscale'])
def test_cli_writes_the_curves_of_its_predictions(tmp_path, multiscale):
    """The JSON of --det_curve is the restatement applied to the coordinates the same run wrote to --predictions and to the synthetic
    targets the run generated; stdout carries the reference's test_dr line (main.py:424: left wrist, radius 10) before the JSON line."""
    import scipy.io
    P, Mat = str(tmp_path / 'curves' / 'det.json'), str(tmp_path / 'pred.mat')
    n = 2 if multiscale else 5                                # 5 images in batches of 2: 4 are evaluated (whole batches)
    args = ['--synthetic', '--debug', '--use_sm', '--synthetic_size', str(n), '--batch_size', '2', '--det_curve', P, '--predictions', Mat]
    out = _run_ok(args + (['--multiscale'] if multiscale else []), str(tmp_path))
    doc = json.load(open(P))
    m = scipy.io.loadmat(Mat)
    N = 2 if multiscale else 4
    assert m['flic_pred_pd'].shape == (2, 9, N)
    y = M._synthetic_dataset(2, n)[3]                         # the call the command line makes (batch size 2)
    names = list(M.joint_names[:9])
    assert sorted(doc) == ['joint_names', 'multiscale', 'n_images', 'pd', 'radii', 'sm', 'use_sm']
    assert doc['radii'] == [float(r) for r in range(1, 21)] and doc['joint_names'] == names and doc['n_images'] == N
    assert doc['multiscale'] is multiscale and doc['use_sm'] is True
    for key, mat in (('pd', 'flic_pred_pd'), ('sm', 'flic_pred_sm')):
        counts = R.det_curve(m[mat].transpose(2, 0, 1), y[:N], RADII)[2]
        assert sorted(doc[key]) == sorted(names)
        for k, name in enumerate(names):
            assert doc[key][name] == (100.0 * counts[k] / N).tolist(), (key, name)
    lines = out.strip().splitlines()
    dr = [l for l in lines if l.startswith('test_dr: ')]
    assert len(dr) == 1 and lines.index(dr[0]) < len(lines) - 1 and json.loads(lines[-1])['n_images'] == N
    assert [float(v) for v in dr[0].split()[1:]] == [doc['pd']['lwri'][9], doc['sm']['lwri'][9]]
