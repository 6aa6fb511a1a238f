"""CPU side of the per-layer activation summaries (--tb_activations): the numpy restatement the GPU tests compare the kernel
with (tests/act_summary_ref.py), the grouping of a batch into tower slices, the tag names and their order, and the command-line refusals."""
import inspect
import os
import re
import sys

import numpy as np
import pytest

import joint_cnn_mrf_amd  # noqa: F401
from joint_cnn_mrf_amd import main as M
from joint_cnn_mrf_amd import summary as S

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import act_summary_ref as A  # noqa: E402
import tb_ref as R  # noqa: E402


def test_restatement_buckets_follow_upper_bound():
    lim = A.limits()
    assert lim.size == A.N_BUCKETS == S.bucket_limits().size and np.array_equal(lim, R.default_limits())
    mid = lim.size // 2                                   # the 0.0 limit
    e = np.float32(lim[mid + 40])
    z = np.array([0.0, -0.0, 1e-12, -1e-12, e, np.nextafter(e, np.float32(0)), np.nan, np.inf, -np.inf, 2.5, -3.0], np.float32).reshape(1, -1)
    (st,) = A.stats(z, 1)
    assert (st['num'], st['n_pos'], st['n_nonfinite'], st['size']) == (8, 4, 3, 11)
    assert st['min'] == -3.0 and st['max'] == 2.5
    b = st['buckets']
    # +-0.0: upper_bound of 0.0 is the bucket behind the 0.0 limit; float32(1e-12) = 9.99999996e-13 lies inside the +-1e-12 limits
    assert b.sum() == 8 and b[mid + 1] == 3 and b[mid] == 1 and b[mid - 1] == 0
    for v in z.reshape(-1)[np.isfinite(z.reshape(-1))]:
        k = int(np.searchsorted(lim, np.float64(v), 'right'))
        assert b[k] >= 1 and (k == 0 or lim[k - 1] <= np.float64(v)) and np.float64(v) < lim[k]
    mn, mx, num, s, ss, counts = R.histogram(z.reshape(-1)[np.isfinite(z.reshape(-1))].astype(np.float64), lim)
    assert np.array_equal(counts, b) and (mn, mx, num) == (st['min'], st['max'], 8.0)
    assert abs(s - st['sum']) <= st['sum_bound'] and abs(ss - st['sum_squares']) <= st['sum_squares_bound']
    (empty,) = A.stats(np.full((1, 4), np.nan, np.float32), 1)
    assert empty['num'] == 0 and empty['min'] == sys.float_info.max and empty['max'] == -sys.float_info.max and empty['buckets'].sum() == 0


def test_grouping_leaves_the_remainder_out():
    assert A.groups(5, 2) == [(0, 2), (2, 4)] and A.groups(4, 2) == [(0, 2), (2, 4)] and A.groups(3, 1) == [(0, 3)]
    assert S.tower_slices(5, 2) == (2, 4) and S.tower_slices(14, 4) == (3, 12) and S.tower_slices(3, 1) == (3, 3)
    for bad in ((1, 2), (3, 0)):
        with pytest.raises(ValueError):
            A.groups(*bad)
        with pytest.raises(ValueError):
            S.tower_slices(*bad)
    z = np.arange(5 * 6, dtype=np.float32).reshape(5, 6) - 7
    st = A.stats(z, 2)
    assert [s['size'] for s in st] == [12, 12] and st[0]['min'] == -7 and st[1]['max'] == 16      # image 4 (23 .. 29 - 7) belongs to no group
    pics = A.pictures(z.reshape(5, 1, 2, 3), 2, 1, 2)
    assert pics.shape == (2, 2, 1, 2) and np.array_equal(pics[1, 0], z.reshape(5, 1, 2, 3)[2, :, :, 1])


def test_activation_is_two_rounded_operations_and_keeps_nan():
    rng = np.random.RandomState(1)
    z = rng.standard_normal((2, 3, 4, 5)).astype(np.float32)
    z[0, 0, 0, 0] = np.nan
    z[0, 0, 1, 1] = np.inf
    z[0, 0, 2, 2] = -np.inf
    sc, sh = A.fold64(rng.uniform(0.5, 2, 5), rng.standard_normal(5), rng.standard_normal(5), rng.uniform(0.1, 2, 5))
    a = A.activation(z, sc, sh)
    assert a.dtype == np.float32 and np.isnan(a[0, 0, 0, 0]) and a[0, 0, 1, 1] == np.inf and a[0, 0, 2, 2] == sh[2]
    neg = z <= 0
    assert np.array_equal(a[neg], np.broadcast_to(sh, z.shape)[neg])
    pos = np.isfinite(z) & (z > 0)
    want = (z.astype(np.float64) * sc.astype(np.float64)).astype(np.float32).astype(np.float64) + sh.astype(np.float64)
    assert np.array_equal(a[pos], want.astype(np.float32)[pos])


def test_scopes_follow_the_models_call_order():
    """The scopes are the conv_layer calls of model (main.py:44-72) in order -- read off model_layerwise, which mirrors it line for line."""
    called = re.findall(r"conv_layer\([^)]*'(conv\w+)'", inspect.getsource(M.model_layerwise))
    assert list(S.ACTIV_SCOPES) == called == A.SCOPES and len(called) == 14
    assert S.ACTIV_CHANNEL == 7 and S.N_ACTIV_TO_SHOW == 3


def test_tag_names_and_order():
    for n_towers, per in ((1, 14), (2, 2), (4, 1)):
        tags = S.activ_tags(n_towers, per)
        assert tags == A.tags(n_towers, per) and len(tags) == len(set(tags)) == n_towers * 14 * (6 + min(3, per))
    t = S.activ_tags(2, 2)
    assert t[:8] == ['tower_0/pre_activ_conv1_fullres/' + k for k in ('max', 'mean', 'min', 'std', 'n_pos', 'histogram')] + \
        ['tower_0/f_activ_conv1_fullres/image/0', 'tower_0/f_activ_conv1_fullres/image/1']
    assert t[-1] == 'tower_1/f_activ_conv6/image/1' and 'tower_0/f_activ_conv6/image/2' not in t
    # var_summary under a tower scope: the six tags, n_pos = the fraction of the slice's elements
    st, cn = np.array([-1.0, 3.0, 4.0, 14.0]), np.zeros(3 + A.N_BUCKETS, np.int64)
    cn[:3] = (4, 3, 0)
    cn[3 + A.N_BUCKETS // 2 + 5] = 4
    vals = [R.parse_value(v) for v in S.var_summary(st, cn, 4, 'conv5', baisc_name='tower_1/pre_activ_')]
    assert [v['tag'] for v in vals] == ['tower_1/pre_activ_conv5/' + k for k in ('max', 'mean', 'min', 'std', 'n_pos', 'histogram')]
    assert vals[0]['simple_value'] == 3.0 and vals[1]['simple_value'] == 1.0 and vals[4]['simple_value'] == 0.75 and vals[5]['histo']['num'] == 4


def test_flag_is_off_by_default_and_refused_without_its_needs():
    a = M.build_parser().parse_args(['--tb_dir', 'x'])
    assert a.tb_activations is False
    sig = inspect.signature(S.merged_summary)
    assert sig.parameters['activations'].default is False and sig.parameters['n_towers'].default == 1
    assert list(sig.parameters)[:10] == ['eng', 'layout', 'x', 'y', 'use_sm', 'n_joints', 'grads', 'params_flat', 'clip_norm', 'images']
    with pytest.raises(SystemExit, match='--tb_dir'):
        M.main(['--tb_activations', '--debug', '--synthetic'])
    with pytest.raises(SystemExit, match='fp32'):
        M.main(['--tb_activations', '--tb_dir', 'x', '--precision', 'bf16', '--debug', '--synthetic'])
