"""The detection-rate sweep over person scale (evaluation.eval_curves_affine, --eval_scale / --scale_curve) on a --debug engine:
against a loop written out here from Engine.augment_affine, Engine.forward and the numpy restatement of the curves (tests/det_curve_ref.py), against
eval_curves at scale 1, the images it leaves out, and the command line -- whose other outputs are those of the run without the flags."""
import json

import numpy as np
import pytest
import torch

import det_curve_ref as R
from cli_util import run_cli
import joint_cnn_mrf_amd  # noqa: F401
from joint_cnn_mrf_amd import augmentation, data, evaluation, synth
from joint_cnn_mrf_amd import main as M

pytestmark = pytest.mark.gpu
RADII = np.arange(1, 21)
H, W = 480, 720


def _dev(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), device='cuda:0', dtype=dtype)


@pytest.fixture(scope='module')
def tower():
    """fp32 handle at --debug width with parameters; 8 images whose joints lie in the middle third of the frame (so that scale 1.5 keeps them inside),
    except joint 3 of image 0, planted in the top left corner."""
    from joint_cnn_mrf_amd.engine import Engine
    p = synth.make_pd_params(debug=True, bn='trained', conv6_gain=8.0)
    p.update(synth.make_sm_params(synth.synthetic_priors(), kind='trained'))
    e = Engine(device=0).load_params(p)
    rs = np.random.RandomState(77)
    cells = np.stack([rs.randint(22, 38, (8, 10)), rs.randint(33, 57, (8, 10))], axis=2).astype(np.int32)
    cells[0, 3] = [2, 2]
    yield e, synth.make_images(8, seed=41), cells, data.target_heat_maps(cells, H // 8, W // 8).astype(np.float32)
    e.close()


def inside(cells, g):
    """Written out: the ten points (8 col + 3.5, 8 row + 3.5) under the forward map of geom row g, all inside [0, W] x [0, H]?"""
    keep = []
    for c in cells:
        ok = True
        for r, q in c:
            px, py = 8.0 * q + 3.5, 8.0 * r + 3.5
            qx, qy = (g[6] * px + g[7] * py) + g[8], (g[9] * px + g[10] * py) + g[11]
            ok = ok and 0.0 <= qx <= W and 0.0 <= qy <= H
        keep.append(ok)
    return np.array(keep)


def test_equals_the_loop_written_out(tower):
    e, X, cells, _ = tower
    scales, angle, pad, B = [0.5, 1.5], 0.1, 0.5, 3
    got = evaluation.eval_curves_affine(X, cells, e, B, scales, angle=angle, pad=pad, use_sm=True)
    assert list(got) == scales
    for s in scales:
        c_pd, c_sm, ys = [], [], []
        for lo in (0, 3, 6):                                      # batches of 3, 3 and 2
            n = len(X[lo:lo + B])
            draw = augmentation.fixed_affine(n, H, W, s, angle=angle, pad=pad)
            assert draw.width.tolist() == [max(1.0, 1.0 / s)] * n
            xa, ya = e.augment_affine(_dev(X[lo:lo + B]), _dev(cells[lo:lo + B]), draw.colour, draw.geom, pad, width=draw.width)
            r = e.forward(xa, ya[..., 9:].contiguous(), use_sm=True, want_prob=False)
            keep = inside(cells[lo:lo + B], draw.geom[0])
            c_pd.append(r['pd_coords'].cpu().numpy()[keep])
            c_sm.append(r['sm_coords'].cpu().numpy()[keep])
            ys.append(ya.cpu().numpy()[keep])
        pd, sm = got[s]
        ys = np.concatenate(ys)
        assert pd.n_images == sm.n_images == len(ys) == (7 if s == 1.5 else 8)
        assert np.array_equal(pd.counts(), R.det_curve(np.concatenate(c_pd), ys, RADII)[2])
        assert np.array_equal(sm.counts(), R.det_curve(np.concatenate(c_sm), ys, RADII)[2])


def test_scale_one_gives_the_counts_of_eval_curves(tower):
    e, X, cells, Y = tower
    assert np.array_equal(e.joint_cells(_dev(Y)).cpu().numpy(), cells)
    pd1, sm1 = evaluation.eval_curves_affine(X, e.joint_cells(_dev(Y)), e, 3, [1.0], use_sm=True)[1.0]
    pd0, sm0 = evaluation.eval_curves(X, Y, e, 3, use_sm=True)
    assert pd1.n_images == pd0.n_images == 8 and sm1.n_images == 8
    assert np.array_equal(pd1.counts(), pd0.counts()) and np.array_equal(sm1.counts(), sm0.counts())
    pd2, sm2 = evaluation.eval_curves_affine(X[:3], cells[:3], e, 2, [1.0], use_sm=False, radii=[5, 10], antialias=False)[1.0]
    assert pd2.n_images == 3 and np.array_equal(pd2.counts(), sm2.counts()) and pd2.counts().shape == (9, 2)


def test_counted_falls_where_a_joint_leaves_the_frame(tower):
    e, X, cells, _ = tower
    got = evaluation.eval_curves_affine(X, cells, e, 4, [1.0, 1.5], use_sm=True)
    assert [got[s][0].n_images for s in (1.0, 1.5)] == [8, 7]      # the planted joint of image 0: (19.5, 19.5) -> (-150.5, -90.5) at scale 1.5
    moved = cells.copy()
    moved[:, 9] = [0, 0]                                             # every torso point out of the frame: nothing is counted, and nothing fails
    none = evaluation.eval_curves_affine(X[:2], moved[:2], e, 2, [1.5], use_sm=True)[1.5]
    assert none[0].n_images == 0 and none[1].n_images == 0


def _run_ok(args, cwd):
    r = run_cli(args, cwd)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return r.stdout


def test_cli_writes_the_curves_and_leaves_the_other_outputs_as_they_are(tmp_path):
    import scipy.io
    a, b = tmp_path / 'with', tmp_path / 'without'
    a.mkdir()
    b.mkdir()
    base = ['--synthetic', '--debug', '--use_sm', '--synthetic_size', '5', '--batch_size', '2', '--det_curve', 'det.json', '--predictions', 'pred.mat']
    out_a = _run_ok(base + ['--eval_scale', '1.0', '0.5', '--scale_curve', 'curves/scale.json'], str(a)).strip().splitlines()
    out_b = _run_ok(base, str(b)).strip().splitlines()
    # the other outputs
    ma, mb = scipy.io.loadmat(str(a / 'pred.mat')), scipy.io.loadmat(str(b / 'pred.mat'))
    for k in ('flic_pred_pd', 'flic_pred_sm'):
        assert np.array_equal(ma[k], mb[k])
    assert json.load(open(a / 'det.json')) == json.load(open(b / 'det.json'))
    assert out_a[:-1] == out_b[:-1]                                  # the test_dr line
    la, lb = json.loads(out_a[-1]), json.loads(out_b[-1])
    assert la.pop('eval_scale') == [1.0, 0.5] and 'eval_scale' not in lb
    for k in ('seconds', 'images_per_sec'):
        la.pop(k), lb.pop(k)
    assert la == lb
    # the file
    doc = json.load(open(a / 'curves' / 'scale.json'))
    names = list(M.joint_names[:9])
    assert sorted(doc) == ['antialias', 'counted', 'joint_names', 'n_images', 'pd', 'radii', 'scales', 'sm', 'use_sm']
    assert doc['scales'] == [1.0, 0.5] and doc['antialias'] is True and doc['radii'] == [float(r) for r in range(1, 21)] and doc['n_images'] == 5
    y = M._synthetic_dataset(2, 5)[3]                                # the call the command line makes (batch size 2): all 5 images are swept
    cells = R.argmax_coords(y, 10).transpose(0, 2, 1)
    want = [int(augmentation.affine_joints_inside(cells, augmentation.fixed_affine(5, H, W, s).geom, H, W).sum()) for s in (1.0, 0.5)]
    assert doc['counted'] == want == [5, 5]
    for key in ('pd', 'sm'):
        assert sorted(doc[key]) == ['0.5', '1.0']
        for s in ('1.0', '0.5'):
            assert sorted(doc[key][s]) == sorted(names)
            for name in names:
                rates = doc[key][s][name]
                assert len(rates) == 20 and all(r in (0.0, 20.0, 40.0, 60.0, 80.0, 100.0) for r in rates) and rates == sorted(rates)
