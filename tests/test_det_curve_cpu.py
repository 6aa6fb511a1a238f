"""Detection-rate curves without a GPU: hand-computed known answers of the numpy restatement (tests/det_curve_ref.py) that the GPU tests
hold jcm_det_curve to, the host-side bookkeeping of evaluation.DetCurve, and the --det_curve flag."""
import numpy as np
import pytest

import det_curve_ref as R
import joint_cnn_mrf_amd  # noqa: F401
from joint_cnn_mrf_amd import evaluation
from joint_cnn_mrf_amd import main as M

RADII = np.arange(1, 21)


def _maps(cells, H=12, W=14, C=9):
    """One image whose channel k has a single 1 at cells[k]."""
    y = np.zeros((1, H, W, C), np.float32)
    for k, (r, c) in enumerate(cells):
        y[0, r, c, k] = 1
    return y


def test_exact_equality_is_a_hit():
    """Joint 0 at (0,0), joint 7 at (6,8): torso = sqrt(36 + 64) = 10 exactly.  A prediction one cell off: 1 * 100 / 10 = 10.0 exactly --
    a hit at radius 10 (<=), a miss at radius 9."""
    cells = [(0, 0), (3, 3), (4, 4), (5, 5), (6, 6), (7, 7), (8, 8), (6, 8), (9, 9)]
    y = _maps(cells)
    pred = np.array(cells, np.int32).T[None].copy()           # [1,2,9]
    pred[0, 1, 2] += 1                                       # joint 2 one column off
    pred[0, 0, 4] -= 3                                       # joint 4 three rows off: 30.0
    pred[0, :, 5] += [3, 4]                                  # joint 5: 5 cells -> 50.0
    true, nd, counts = R.det_curve(pred, y, RADII)
    assert np.array_equal(true[0].T, np.array(cells))
    assert nd.dtype == np.float32 and nd[0, 2] == np.float32(10.0) and nd[0, 4] == np.float32(30.0) and nd[0, 5] == np.float32(50.0)
    assert nd[0, 0] == 0 and nd[0, 8] == 0
    assert counts[2, 9] == 1 and counts[2, 8] == 0            # radius 10 / radius 9
    assert counts[2].tolist() == [0] * 9 + [1] * 11
    assert counts[4].sum() == 0 and counts[5].sum() == 0
    assert counts[0].tolist() == [1] * 20


def test_zero_torso_is_never_a_hit():
    """Joints 0 and 7 on one cell: pred == true gives 0 * 100 / 0 = NaN, pred != true gives inf; neither is <= any radius."""
    cells = [(5, 5), (3, 3), (4, 4), (5, 5), (6, 6), (7, 7), (8, 8), (5, 5), (9, 9)]
    y = _maps(cells)
    pred = np.array(cells, np.int32).T[None].copy()
    pred[0, 0, 2] += 2
    true, nd, counts = R.det_curve(pred, y, [1, 10, 3e38])
    assert np.isnan(nd[0, 0]) and np.isnan(nd[0, 1]) and np.isinf(nd[0, 2]) and nd[0, 2] > 0
    assert counts.sum() == 0                                  # no finite radius reaches inf, nothing compares with NaN
    true, nd, counts = R.det_curve(pred, y, RADII)
    assert counts.sum() == 0


def test_tie_goes_to_the_lower_flat_index_and_empty_maps_to_the_origin():
    y = _maps([(0, 0), (3, 3), (4, 4), (5, 5), (6, 6), (7, 7), (8, 8), (6, 8), (9, 9)])
    y[0, 2, 13, 1] = 1                                        # flat 2 * 14 + 13 = 41 < 3 * 14 + 3 = 45
    y[0, 11, 0, 2] = 1                                        # flat 154 > 4 * 14 + 4
    y[0, :, :, 3] = 0                                         # all zero
    y[0, :, :, 4] = np.nan                                    # all NaN
    y[0, :, :, 5] = -np.inf
    y[0, 0, 1, 6] = np.nan                                    # a NaN in front of the maximum does not win
    y[0, :, :, 8] = -np.inf                                   # NaN, NaN, then -inf only: the first -inf, as in the kernels (-inf ties the start, NaN never)
    y[0, 0, :2, 8] = np.nan
    true = R.argmax_coords(y, 9)
    assert true[0, :, 8].tolist() == [0, 2]
    assert true[0, :, 1].tolist() == [2, 13] and true[0, :, 2].tolist() == [4, 4]
    assert true[0, :, 3].tolist() == [0, 0] and true[0, :, 4].tolist() == [0, 0] and true[0, :, 5].tolist() == [0, 0]
    assert true[0, :, 6].tolist() == [8, 8]


def test_counts_never_decrease_over_ascending_radii():
    rs = np.random.RandomState(5)
    y = R.blob_targets(rs, 40, 13, 17, 10, noisy=(1, 4))
    true = R.argmax_coords(y, 9)
    pred = R.displaced(rs, true, 13, 17)
    _t, nd, counts = R.det_curve(pred, y, RADII)
    assert counts.shape == (9, 20) and (np.diff(counts, axis=1) >= 0).all()
    assert 0 < counts.sum() < 40 * 9 * 20 and counts.max() <= 40
    # the single number the repository already had: joint 2, radius 10
    want = np.mean(nd[:, 2] <= np.float32(10))
    assert counts[2, 9] / 40 == want


class _StubEngine:
    """Stands in for Engine.det_curve on the host: the restatement on numpy arrays, accumulating like the kernel does."""
    n_joints = 9

    def det_curve(self, pred, y, radii, hits=None, want_dist=False, want_true=False):
        class _Arr:                                           # the two tensor methods DetCurve.counts() uses
            def __init__(self, a):
                self.a = a

            def cpu(self):
                return self

            def numpy(self):
                return self.a
        counts = R.det_curve(pred, y, radii)[2].astype(np.int32)
        return {'hits': _Arr(counts if hits is None else hits.a + counts)}


def _set(seed, B):
    rs = np.random.RandomState(seed)
    y = R.blob_targets(rs, B, 13, 17, 10)
    return R.displaced(rs, R.argmax_coords(y, 9), 13, 17), y


def test_det_curve_accumulates_merges_and_reports():
    pred, y = _set(7, 11)
    want = R.det_curve(pred, y, RADII)[2]
    a = evaluation.DetCurve(_StubEngine())
    for lo, hi in ((0, 3), (3, 4), (4, 11)):
        a.update(pred[lo:hi], y[lo:hi])
    assert a.n_images == 11 and np.array_equal(a.counts(), want)
    assert np.array_equal(a.rates(), 100 * want / 11)
    b, c = evaluation.DetCurve(_StubEngine()), evaluation.DetCurve(None, n_joints=9)      # c: counts merged in only, no engine
    b.update(pred[:5], y[:5])
    c.merge(evaluation.DetCurve(_StubEngine()).update(pred[5:], y[5:]))
    b.merge(c)
    assert b.n_images == 11 and np.array_equal(b.counts(), want)
    assert a.rate(2, 10) == 100 * want[2, 9] / 11
    with pytest.raises(KeyError):
        a.rate(2, 10.5)
    d = a.as_dict(M.joint_names)
    assert d['radii'] == [float(r) for r in range(1, 21)] and d['n_images'] == 11
    assert sorted(d) == sorted(['radii', 'n_images'] + list(M.joint_names[:9]))
    assert d['lwri'] == (100 * want[2] / 11).tolist()
    with pytest.raises(ValueError):
        a.merge(evaluation.DetCurve(None, radii=[1, 2], n_joints=9))
    with pytest.raises(ValueError):
        evaluation.DetCurve(None, n_joints=9).rates()          # no image seen


def test_parser_knows_det_curve_and_training_refuses_it(tmp_path):
    a = M.build_parser().parse_args(['--use_sm', '--det_curve', 'curves.json'])
    assert a.det_curve == 'curves.json' and M.build_parser().parse_args([]).det_curve is None
    hps = M.hps
    try:
        with pytest.raises(SystemExit) as ei:
            M.main(['--train', '--synthetic', '--debug', '--det_curve', str(tmp_path / 'c.json')])
    finally:
        M.hps = hps                                           # main() stores its arguments in the module global
    assert '--det_curve' in str(ei.value) and '--train' in str(ei.value)
    assert not (tmp_path / 'c.json').exists()


def test_evaluated_indices_follow_the_towers():
    """Which test image a prediction column belongs to: whole batches only, and per batch the towers' slices (batch_size // n_towers each)."""
    from joint_cnn_mrf_amd.dist import shard_bounds
    assert M.evaluated_indices(5, 2, 1).tolist() == [0, 1, 2, 3]
    assert M.evaluated_indices(30, 14, 4).tolist() == list(range(0, 12)) + list(range(14, 26))      # column 12 is image 14
    assert M.evaluated_indices(30, 14, 2).tolist() == list(range(28))
    assert M.evaluated_indices(7, 3, 2).tolist() == [0, 1, 3, 4]
    assert M.evaluated_indices(3, 4, 1).tolist() == [] and M.evaluated_indices(5, 2, 1, multiscale=True).tolist() == [0, 1, 2, 3, 4]
    for n, B, T in ((30, 14, 4), (17, 5, 3), (8, 4, 2)):         # the same walk as main(): batches, then Towers.slices
        want = [b0 + i for b0 in range(0, (n // B) * B, B) for t in range(T) for i in range(*shard_bounds(B, T, t))]
        assert M.evaluated_indices(n, B, T).tolist() == want


def test_curves_of_predictions_use_the_index():
    """Column i of the predictions is judged against y[index[i]]: with a dropped remainder the targets are not the first N."""
    rs = np.random.RandomState(9)
    y = R.blob_targets(rs, 7, 13, 17, 10)
    index = M.evaluated_indices(7, 3, 2)                        # images 0, 1, 3, 4
    pred = R.displaced(rs, R.argmax_coords(y[index], 9), 13, 17, -1, 1)
    cols = pred.transpose(1, 2, 0)                              # [2,K,N]
    pd, sm = M.det_curves_of_predictions(_NumpyEngine(), cols, cols, y, index=index)
    want = R.det_curve(pred, y[index], RADII)[2]
    assert pd.n_images == 4 and np.array_equal(pd.counts(), want) and np.array_equal(sm.counts(), want)
    assert not np.array_equal(R.det_curve(pred, y[:4], RADII)[2], want)      # the pairing the index prevents
    with pytest.raises(ValueError):
        M.det_curves_of_predictions(_NumpyEngine(), cols, cols, y, index=index[:3])


class _NumpyEngine(_StubEngine):
    """_StubEngine behind det_curves_of_predictions, which hands it host torch tensors."""
    device = 'cpu'

    def det_curve(self, pred, y, radii, hits=None, want_dist=False, want_true=False):
        return super().det_curve(pred.numpy(), y.numpy(), radii, hits=hits)
