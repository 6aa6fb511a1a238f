"""Flow-centred scans on the GPU: jcm_seq_filter_centred and jcm_seq_viterbi_centred (csrc/seq_centred.hip) against the numpy float64
restatement (tests/seq_centred_ref.py, pinned by tests/test_seq_centred_cpu.py) on the inputs that file builds.  Viterbi is products, quotients
and maxima only: path, maxes and breaks are compared bit for bit.  The filter's coords and reset are compared exactly; its norm, state and belief
bit for bit against the restatement that sums Z in the kernel's order; filtered is the fp32 rounding of that belief.  A uniform table must give
the bits of Engine.seq_*(shift=), a zero table those of the plain calls."""
import ctypes
import functools

import numpy as np
import pytest
import torch
from numpy.testing import assert_array_equal

import seq_centred_ref as CR
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
    hm, taps, Rr, sigma, rho, centre, _ = CR.case_inputs(name, P.seq_taps)
    return hm, taps, Rr, sigma, rho, centre, {'filter': CR.seq_filter(hm, taps, rho, centre), 'viterbi': CR.seq_viterbi(hm, taps, rho, centre)}


def _dev(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), device='cuda:0', dtype=dtype)


def _host(r):
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in r.items()}


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64 if a.dtype == np.float64 else np.int32)


@pytest.mark.parametrize('name', sorted(CR.CASES))
def test_viterbi_bits(eng, name):
    hm, taps, Rr, sigma, rho, centre, ref = _case(name)
    got = _host(eng.seq_viterbi(_dev(hm), sigma, rho, radius=Rr, centre=centre))      # the table from the host
    want = ref['viterbi']
    assert_array_equal(got['path'], want['path'])
    assert_array_equal(got['breaks'], want['breaks'])
    assert_array_equal(_bits(got['maxes']), _bits(want['maxes']))


@pytest.mark.parametrize('name', sorted(CR.CASES))
def test_filter_bits(eng, name):
    hm, taps, Rr, sigma, rho, centre, ref = _case(name)
    got = _host(eng.seq_filter(_dev(hm), sigma, rho, radius=Rr, centre=_dev(centre, torch.int32)))      # the table on the device this time
    want = ref['filter']
    assert_array_equal(got['coords'], want['coords'])
    assert_array_equal(got['reset'], want['reset'])
    assert_array_equal(_bits(got['norm']), _bits(want['norm']))
    assert_array_equal(_bits(got['state']), _bits(want['state']))
    assert_array_equal(_bits(got['filtered']), _bits(want['belief'].astype(np.float32)))


def test_lost_resets_and_breaks(eng):
    hm, taps, Rr, sigma, rho, centre, ref = _case('lost')
    assert (ref['filter']['reset'][0, 2] == 1).all() and (ref['viterbi']['breaks'][0, 2] == 1).all()


def test_filter_belief_bits_frame_by_frame(eng):
    """The float64 belief of EVERY frame, not only the last: a clip fed one frame per call hands each a_t out as 'state'; every call's row 0 of the
    table applies to the state it is given."""
    hm, taps, Rr, sigma, rho, centre, ref = _case('odd')
    S, T, HH, WW, K = hm.shape
    t_hm, state = _dev(hm), None
    for t in range(T):
        r = eng.seq_filter(t_hm[:, t:t + 1].contiguous(), sigma, rho, radius=Rr, centre=centre[:, t:t + 1], state=state)
        state = r['state']
        torch.cuda.synchronize()
        assert_array_equal(_bits(state.cpu().numpy()), _bits(ref['filter']['belief'][:, t].transpose(0, 3, 1, 2)))


@pytest.mark.parametrize('name', sorted(MR.CASES))
def test_uniform_table_is_the_moving_entry(eng, name):
    hm, taps, Rr, sigma, rho, shift, _ = MR.case_inputs(name, P.seq_taps)
    t_hm, table = _dev(hm), CR.uniform_table(shift, hm.shape[2], hm.shape[3])
    for moving, centred in ((eng.seq_filter(t_hm, sigma, rho, radius=Rr, shift=shift), eng.seq_filter(t_hm, sigma, rho, radius=Rr, centre=table)),
                            (eng.seq_viterbi(t_hm, sigma, rho, radius=Rr, shift=shift), eng.seq_viterbi(t_hm, sigma, rho, radius=Rr, centre=table))):
        moving, centred = _host(moving), _host(centred)
        assert sorted(moving) == sorted(centred)
        for k in moving:
            assert_array_equal(_bits(centred[k]), _bits(moving[k]), err_msg=k)


@pytest.mark.parametrize('name', ('odd', 'vector', 'clipped'))
def test_zero_table_is_the_plain_entry(eng, name):
    hm, taps, Rr, sigma, rho, _ = R.case_inputs(name, P.seq_taps)
    t_hm, zero = _dev(hm), np.zeros(hm.shape[:4] + (2,), np.int32)
    for plain, centred in ((eng.seq_filter(t_hm, sigma, rho, radius=Rr), eng.seq_filter(t_hm, sigma, rho, radius=Rr, centre=zero)),
                           (eng.seq_viterbi(t_hm, sigma, rho, radius=Rr), eng.seq_viterbi(t_hm, sigma, rho, radius=Rr, centre=zero))):
        plain, centred = _host(plain), _host(centred)
        assert sorted(plain) == sorted(centred)
        for k in plain:
            assert_array_equal(_bits(centred[k]), _bits(plain[k]), err_msg=k)


def test_a_4d_call_takes_a_4d_table_and_wrong_ones_are_refused(eng):
    hm, taps, Rr, sigma, rho, centre, ref = _case('odd')
    got = _host(eng.seq_viterbi(_dev(hm[1]), sigma, rho, radius=Rr, centre=centre[1]))
    assert_array_equal(got['path'], ref['viterbi']['path'][1])
    with pytest.raises(ValueError, match='centre must be'):
        eng.seq_viterbi(_dev(hm), sigma, rho, radius=Rr, centre=centre[:, :2])
    with pytest.raises(ValueError, match='centre must be'):
        eng.seq_filter(_dev(hm), sigma, rho, radius=Rr, centre=centre[..., :1])
    with pytest.raises(ValueError, match='int32'):
        eng.seq_filter(_dev(hm), sigma, rho, radius=Rr, centre=centre.astype(np.float64))
    for call in (eng.seq_filter, eng.seq_viterbi):
        with pytest.raises(ValueError, match='centre and shift'):
            call(_dev(hm), sigma, rho, radius=Rr, centre=centre, shift=np.zeros(hm.shape[:2] + (2,), np.int32))


def test_null_centre_is_refused_and_touches_nothing(eng):
    S, T, HH, WW, K, Rr = 1, 2, 5, 7, 2, 1
    hm = torch.rand(S, T, HH, WW, K, device='cuda:0')
    centre = torch.zeros(S, T, HH, WW, 2, dtype=torch.int32, device='cuda:0')
    tp = P.seq_taps(1.0, Rr, K).ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    outs = {'filtered': torch.full((S, T, HH, WW, K), 7.0, device='cuda:0'), 'coords': torch.full((S, T, 2, K), 7, dtype=torch.int32, device='cuda:0'),
            'norm': torch.full((S, T, K), 7.0, dtype=torch.float64, device='cuda:0'), 'reset': torch.full((S, T, K), 7, dtype=torch.int32, device='cuda:0'),
            'state': torch.full((S, K, HH, WW), 7.0, dtype=torch.float64, device='cuda:0'), 'path': torch.full((S, T, 2, K), 7, dtype=torch.int32, device='cuda:0'),
            'maxes': torch.full((S, T, K), 7.0, dtype=torch.float64, device='cuda:0'), 'breaks': torch.full((S, T, K), 7, dtype=torch.int32, device='cuda:0')}
    torch.cuda.synchronize()
    p, lib, h = eng._p, eng._lib, eng._h
    for ce, k, rho, coords in ((None, K, 0.05, outs['coords']), (centre, 17, 0.05, outs['coords']), (centre, K, 1.5, outs['coords']), (centre, K, 0.05, None)):
        rc = lib.jcm_seq_filter_centred(h, p(hm), S, T, HH, WW, k, tp, Rr, rho, p(ce), p(None), p(outs['filtered']), p(coords), p(outs['norm']),
                                        p(outs['reset']), p(outs['state']))
        assert rc == 1
        rc = lib.jcm_seq_viterbi_centred(h, p(hm), S, T, HH, WW, k, tp, Rr, rho, p(ce), p(None if coords is None else outs['path']), p(outs['maxes']),
                                         p(outs['breaks']))
        assert rc == 1
    torch.cuda.synchronize()
    for name, t in outs.items():
        assert int((t != 7).sum()) == 0, name
    from joint_cnn_mrf_amd import _lib
    lib.jcm_seq_filter_centred(h, p(hm), S, T, HH, WW, K, tp, Rr, 0.05, p(None), p(None), p(None), p(outs['coords']), p(None), p(None), p(None))
    assert 'seq_filter_centred' in _lib.last_error() and 'centre is required' in _lib.last_error()
    lib.jcm_seq_viterbi_centred(h, p(hm), S, T, HH, WW, K, tp, Rr, 0.05, p(None), p(outs['path']), p(None), p(None))
    assert 'seq_viterbi_centred' in _lib.last_error() and 'centre is required' in _lib.last_error()


def test_the_calls_are_timed_under_their_names(eng):
    hm, taps, Rr, sigma, rho, centre, _ = _case('vector')
    eng.set_option('profile', 1)
    try:
        eng.seq_filter(_dev(hm), sigma, rho, radius=Rr, centre=centre)
        eng.seq_viterbi(_dev(hm), sigma, rho, radius=Rr, centre=centre)
        for scope in ('seq_filter_centred', 'seq_viterbi_centred'):      # one call files one pair of events under the entry's name
            ms, n = eng.profile_read(scope)
            assert n == 1 and ms >= 0.0, scope
            assert eng.profile_read(scope) == (0.0, 0), scope
    finally:
        eng.set_option('profile', 0)
