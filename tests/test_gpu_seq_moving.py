"""Frame sequences whose lattice moves, on the GPU: jcm_seq_filter_moving and jcm_seq_viterbi_moving (csrc/sequence.hip, the scans
of csrc/seq_scan.h with the shift policy) against the numpy float64 restatement (tests/seq_moving_ref.py, pinned by tests/test_seq_moving_cpu.py)
on the inputs that file builds.  Viterbi is products, quotients and maxima only: path, maxes and breaks are compared bit for bit.  The filter's
coords and reset are compared exactly; its norm, state and belief bit for bit against the restatement that sums Z in the kernel's order;
filtered is the fp32 rounding of that belief."""
import ctypes
import functools

import numpy as np
import pytest
import torch
from numpy.testing import assert_array_equal

import seq_moving_ref as MR
import seq_ref as R
import joint_cnn_mrf_amd  # noqa: F401
from joint_cnn_mrf_amd import predict as P

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def eng():
    """A bare fp32 handle: the sequence kernels need no parameters."""
    from joint_cnn_mrf_amd.engine import Engine
    e = Engine(device=0)
    yield e
    e.close()


@functools.lru_cache(maxsize=None)
def _case(name):
    """The shared inputs of a case and the restatement's results, computed once and never written to."""
    hm, taps, Rr, sigma, rho, shift, _ = MR.case_inputs(name, P.seq_taps)
    return hm, taps, Rr, sigma, rho, shift, {'filter': MR.seq_filter(hm, taps, rho, shift), 'viterbi': MR.seq_viterbi(hm, taps, rho, shift)}


def _dev(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), device='cuda:0', dtype=dtype)


def _host(r):
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in r.items()}


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64 if a.dtype == np.float64 else np.int32)


@pytest.mark.parametrize('name', sorted(MR.CASES))
def test_viterbi_bits(eng, name):
    hm, taps, Rr, sigma, rho, shift, ref = _case(name)
    got = _host(eng.seq_viterbi(_dev(hm), sigma, rho, radius=Rr, shift=shift))
    want = ref['viterbi']
    assert_array_equal(got['path'], want['path'])
    assert_array_equal(got['breaks'], want['breaks'])
    assert_array_equal(_bits(got['maxes']), _bits(want['maxes']))


@pytest.mark.parametrize('name', sorted(MR.CASES))
def test_filter_bits(eng, name):
    hm, taps, Rr, sigma, rho, shift, ref = _case(name)
    got = _host(eng.seq_filter(_dev(hm), sigma, rho, radius=Rr, shift=_dev(shift, torch.int32)))      # the shift on the device this time
    want = ref['filter']
    assert_array_equal(got['coords'], want['coords'])
    assert_array_equal(got['reset'], want['reset'])
    assert_array_equal(_bits(got['norm']), _bits(want['norm']))
    assert_array_equal(_bits(got['state']), _bits(want['state']))
    assert_array_equal(_bits(got['filtered']), _bits(want['belief'].astype(np.float32)))


def test_filter_belief_bits_frame_by_frame(eng):
    """The float64 belief of EVERY frame, not only the last: a clip fed one frame per call hands each a_t out as 'state'."""
    hm, taps, Rr, sigma, rho, shift, ref = _case('odd')
    S, T, HH, WW, K = hm.shape
    t_hm, state = _dev(hm), None
    for t in range(T):
        r = eng.seq_filter(t_hm[:, t:t + 1].contiguous(), sigma, rho, radius=Rr, shift=shift[:, t:t + 1], state=state)
        state = r['state']
        torch.cuda.synchronize()
        assert_array_equal(_bits(state.cpu().numpy()), _bits(ref['filter']['belief'][:, t].transpose(0, 3, 1, 2)))


@pytest.mark.parametrize('name', ('odd', 'vector', 'clipped'))
def test_zero_shift_is_the_plain_entry(eng, name):
    hm, taps, Rr, sigma, rho, _ = R.case_inputs(name, P.seq_taps)
    S, T = hm.shape[:2]
    t_hm, zero = _dev(hm), np.zeros((S, T, 2), np.int32)
    for plain, moving in ((eng.seq_filter(t_hm, sigma, rho, radius=Rr), eng.seq_filter(t_hm, sigma, rho, radius=Rr, shift=zero)),
                          (eng.seq_viterbi(t_hm, sigma, rho, radius=Rr), eng.seq_viterbi(t_hm, sigma, rho, radius=Rr, shift=zero))):
        plain, moving = _host(plain), _host(moving)
        assert sorted(plain) == sorted(moving)
        for k in plain:
            assert_array_equal(_bits(moving[k]), _bits(plain[k]))


def test_split_call_carries_the_state_across_a_shift(eng):
    """T = 6 in one call equals 3 + 3 with the state carried, bit for bit; the second call's shift[0] is non-zero and applies to the state."""
    hm, taps, Rr, sigma, rho, shift, _ = _case('split')
    assert shift[0, 3].any()
    t = _dev(hm)
    whole = _host(eng.seq_filter(t, sigma, rho, radius=Rr, shift=shift))
    first = eng.seq_filter(t[:, :3].contiguous(), sigma, rho, radius=Rr, shift=shift[:, :3])
    second = _host(eng.seq_filter(t[:, 3:].contiguous(), sigma, rho, radius=Rr, shift=shift[:, 3:], state=first['state']))
    first = _host(first)
    for k in ('filtered', 'coords', 'norm', 'reset'):
        assert_array_equal(_bits(np.concatenate([first[k], second[k]], axis=1)), _bits(whole[k]))
    assert_array_equal(_bits(second['state']), _bits(whole['state']))


def test_a_4d_call_takes_a_2d_shift(eng):
    hm, taps, Rr, sigma, rho, shift, ref = _case('odd')
    got = _host(eng.seq_viterbi(_dev(hm[1]), sigma, rho, radius=Rr, shift=shift[1]))
    assert_array_equal(got['path'], ref['viterbi']['path'][1])
    with pytest.raises(ValueError, match='shift must be'):
        eng.seq_viterbi(_dev(hm), sigma, rho, radius=Rr, shift=shift[:, :2])
    with pytest.raises(ValueError, match='int32'):
        eng.seq_filter(_dev(hm), sigma, rho, radius=Rr, shift=shift.astype(np.float64))


def test_null_shift_is_refused_and_touches_nothing(eng):
    S, T, HH, WW, K, Rr = 1, 2, 5, 7, 2, 1
    hm = torch.rand(S, T, HH, WW, K, device='cuda:0')
    shift = torch.zeros(S, T, 2, dtype=torch.int32, device='cuda:0')
    tp = P.seq_taps(1.0, Rr, K).ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    outs = {'filtered': torch.full((S, T, HH, WW, K), 7.0, device='cuda:0'), 'coords': torch.full((S, T, 2, K), 7, dtype=torch.int32, device='cuda:0'),
            'norm': torch.full((S, T, K), 7.0, dtype=torch.float64, device='cuda:0'), 'reset': torch.full((S, T, K), 7, dtype=torch.int32, device='cuda:0'),
            'state': torch.full((S, K, HH, WW), 7.0, dtype=torch.float64, device='cuda:0'), 'path': torch.full((S, T, 2, K), 7, dtype=torch.int32, device='cuda:0'),
            'maxes': torch.full((S, T, K), 7.0, dtype=torch.float64, device='cuda:0'), 'breaks': torch.full((S, T, K), 7, dtype=torch.int32, device='cuda:0')}
    torch.cuda.synchronize()
    p, lib, h = eng._p, eng._lib, eng._h
    for sh, k, rho, coords in ((None, K, 0.05, outs['coords']), (shift, 17, 0.05, outs['coords']), (shift, K, 1.5, outs['coords']), (shift, K, 0.05, None)):
        rc = lib.jcm_seq_filter_moving(h, p(hm), S, T, HH, WW, k, tp, Rr, rho, p(sh), p(None), p(outs['filtered']), p(coords), p(outs['norm']),
                                       p(outs['reset']), p(outs['state']))
        assert rc == 1
        rc = lib.jcm_seq_viterbi_moving(h, p(hm), S, T, HH, WW, k, tp, Rr, rho, p(sh), p(None if coords is None else outs['path']), p(outs['maxes']),
                                        p(outs['breaks']))
        assert rc == 1
    torch.cuda.synchronize()
    for name, t in outs.items():
        assert int((t != 7).sum()) == 0, name
    from joint_cnn_mrf_amd import _lib
    lib.jcm_seq_filter_moving(h, p(hm), S, T, HH, WW, K, tp, Rr, 0.05, p(None), p(None), p(None), p(outs['coords']), p(None), p(None), p(None))
    assert 'seq_filter_moving' in _lib.last_error() and 'shift is required' in _lib.last_error()
