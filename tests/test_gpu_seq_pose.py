"""The clip decode on the GPU: jcm_seq_pose_viterbi (csrc/seq_pose.hip) bit for bit against the numpy restatement tests/seq_pose_ref.py (pinned by
tests/test_seq_pose_cpu.py), the argument contract, and jcm_pose_decode's bits after its scoring function moved to csrc/pose_score.h."""
import ctypes

import numpy as np
import pytest
import torch
from numpy.testing import assert_array_equal

import pose_ref
import seq_pose_ref as R
import joint_cnn_mrf_amd  # noqa: F401
from joint_cnn_mrf_amd import synth

pytestmark = pytest.mark.gpu
OUT = ('index', 'coords', 'frame_score', 'maxes', 'breaks')
CASES = [(2, 5, 2), (1, 4, 3), (1, 3, 4), (3, 1, 2)]      # (S, T, P); the last is T = 1


@pytest.fixture(scope='module')
def eng():
    from joint_cnn_mrf_amd.engine import Engine
    e = Engine(device=0).load_params(synth.make_pd_params(debug=True, bn='trained', conv6_gain=8.0))      # the entry itself reads no parameter
    yield e
    e.close()


def _dev(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), device='cuda:0', dtype=dtype)


def _bits(a):
    return a.view({4: np.int32, 8: np.int64}[a.dtype.itemsize])


def _run(eng, case):
    V, M, count, cells, tau = case
    got = eng.seq_pose_viterbi(_dev(V), _dev(M), _dev(count), _dev(cells), _dev(tau))
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in got.items()}


def _check(eng, case):
    got, want = _run(eng, case), R.decode(*case)
    for k in OUT:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, k
        assert_array_equal(_bits(got[k]), _bits(want[k]), err_msg=k)
    return got


@pytest.mark.parametrize('integers', [False, True])
@pytest.mark.parametrize('S,T,P', CASES)
def test_bit_equal_to_the_restatement(eng, S, T, P, integers):
    """Random floats, and a few small integers so that exact ties occur in every pass; counts mixed in 0..P with both kinds of break; -inf entries in
    tau; NaN in every slot of V, M and tau at or beyond count, which proves they are never read."""
    case = R.random_case(S, T, P, 100 * P + 10 * T + S + (50 if integers else 0), integers=integers)
    assert np.isnan(case[0]).any() and np.isnan(case[4]).any() and (T == 1 or np.isinf(case[4]).any())      # T = 1: tau is never read at all
    got = _check(eng, case)
    if T >= 3:
        assert (got['breaks'] == 2).any()
    if (S, T, P) == (2, 5, 2):
        assert (got['breaks'] == 1).any()
    assert not np.isnan(got['maxes']).any() and not np.isnan(got['frame_score']).any()


def test_full_counts_and_a_single_tensor_axis(eng):
    """Every count P (no break), tables without the S axis."""
    case = R.random_case(1, 4, 4, 7, counts='full', nan_fill=False)
    got = _check(eng, case)
    assert (got['breaks'] == 0).all() and (got['index'] >= 0).all()
    one = eng.seq_pose_viterbi(*[_dev(a[0]) for a in case])
    torch.cuda.synchronize()
    for k in OUT:
        assert_array_equal(_bits(one[k].cpu().numpy()), _bits(got[k][0]), err_msg=k)


def test_argument_contract(eng):
    p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)
    S, T, P = 1, 2, 2
    V, M, count, cells, tau = (_dev(a) for a in R.random_case(S, T, P, 3, counts='full', nan_fill=False))
    mark = -77

    def call(S_=S, T_=T, P_=P, drop=None, handle=None):
        ins = [V, M, count, cells, tau]
        outs = [torch.full((S, T, 9), mark, dtype=torch.int32, device='cuda:0'), torch.full((S, T, 2, 9), mark, dtype=torch.int32, device='cuda:0'),
                torch.full((S, T), float(mark), device='cuda:0'), torch.full((S, T), float(mark), dtype=torch.float64, device='cuda:0'),
                torch.full((S, T), mark, dtype=torch.int32, device='cuda:0')]
        args = [None if drop == i else t for i, t in enumerate(ins + outs)]
        torch.cuda.synchronize()
        rc = eng._lib.jcm_seq_pose_viterbi(eng._h if handle is None else handle, *[p(t) for t in args[:5]], S_, T_, P_, *[p(t) for t in args[5:]])
        torch.cuda.synchronize()
        return rc, all(bool((o == mark).all()) for o in outs)
    for kw in (dict(P_=0), dict(P_=5), dict(S_=0), dict(T_=0), dict(S_=-1), dict(S_=1 << 16, T_=1 << 15), dict(drop=0), dict(drop=1), dict(drop=2),
               dict(drop=3), dict(drop=4), dict(drop=5)):
        assert call(**kw) == (1, True), kw      # JCM_ERR_ARG, nothing touched
    for drop in (None, 6, 7, 8, 9):      # the optional outputs
        rc, untouched = call(drop=drop)
        assert rc == 0 and not untouched, drop
    with pytest.raises(ValueError, match='seq_pose_viterbi expects'):
        eng.seq_pose_viterbi(V, M, count, cells, tau[:, :1].contiguous())
    with pytest.raises(ValueError, match='seq_pose_viterbi expects'):
        five = [_dev(a) for a in R.random_case(1, 2, 5, 3, counts='full', nan_fill=False)]
        eng.seq_pose_viterbi(*five)
    with pytest.raises(ValueError, match='must be'):
        eng.seq_pose_viterbi(V, M, count.to(torch.int64), cells, tau)


def test_pose_decode_keeps_its_bits():
    """jcm_pose_decode on the inputs of tests/test_gpu_pose.py's generators, bit for bit against pose_ref.search32 on the GPU's own tables -- what that
    file holds the kernels to, here as the check that sharing the scoring function changed nothing: noise with full and with mixed counts, P = 1..4."""
    from joint_cnn_mrf_amd.engine import Engine
    params = dict(synth.make_pd_params(debug=True, bn='trained', conv6_gain=8.0), **synth.make_sm_params(synth.synthetic_priors(), kind='trained'))
    e = Engine(device=0).load_params(params)
    try:
        for P in (1, 2, 3, 4):
            hm10 = pose_ref.noise_hm10(3, 40 + P)
            cells, count = pose_ref.random_cells(3, P, 53)
            if P == 4:
                count = np.array([[4, 1, 3, 2, 4, 1, 2, 3, 4], [2, 2, 0, 4, 4, 4, 1, 1, 3], [1, 4, 4, 4, 2, 3, 4, 4, 1]], np.int32)
                cells[np.arange(P)[None, None, :] >= count[:, :, None]] = -1
            got = e.pose_decode(_dev(hm10), {'cells': _dev(cells, torch.int32), 'count': _dev(count, torch.int32)}, want_tables=True)
            torch.cuda.synchronize()
            got = {k: v.cpu().numpy() for k, v in got.items()}
            want = pose_ref.search32(got['V'], got['M'], count, cells)
            for k in ('index', 'coords', 'score', 'score0'):
                assert_array_equal(_bits(got[k]), _bits(want[k]), err_msg='%s P=%d' % (k, P))
    finally:
        e.close()
