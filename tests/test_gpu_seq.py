"""Frame sequences on the GPU: jcm_seq_filter and jcm_seq_viterbi (csrc/sequence.hip) against the numpy float64 restatement
(tests/seq_ref.py, pinned by tests/test_seq_cpu.py) on the inputs that file builds.
Viterbi is products, quotients and maxima only: path, maxes and breaks are compared bit for bit.  The filter's coords and reset are compared
exactly; its float64 state and norm within the derived bound seq_ref.tolerance (first-order rounding of t + 1 steps of positive sums whose
order may differ) against a restatement that sums in ANOTHER order, and bit for bit against the one that mirrors the kernel's order; filtered
within one fp32 ulp of the float64 belief."""
import ctypes
import functools
import re

import numpy as np
import pytest
import torch
from numpy.testing import assert_array_equal

import seq_ref as R
import joint_cnn_mrf_amd  # noqa: F401
from joint_cnn_mrf_amd import _lib
from joint_cnn_mrf_amd import predict as P

pytestmark = pytest.mark.gpu
W3 = np.array([[0.25, 0.5, 0.25]])


@pytest.fixture(scope='module')
def eng():
    """A bare fp32 handle: the sequence kernels need no parameters."""
    from joint_cnn_mrf_amd.engine import Engine
    e = Engine(device=0)
    yield e
    e.close()


@functools.lru_cache(maxsize=None)
def _case(name):
    """The shared inputs of a case and the reference results, computed once and never written to."""
    hm, taps, Rr, sigma, rho, _ = R.case_inputs(name, P.seq_taps)
    ref = {'mirror': R.seq_filter(hm, taps, rho), 'other': R.seq_filter(hm, taps, rho, kernel_order=False), 'viterbi': R.seq_viterbi(hm, taps, rho)}
    return hm, taps, Rr, sigma, rho, ref


def _dev(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), device='cuda:0', dtype=dtype)


def _host(r):
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in r.items()}


def _maps(frames):
    return np.stack([np.asarray(f, np.float32) for f in frames])[None, :, :, :, None]


def _delta(HH, WW, y, x):
    a = np.zeros((HH, WW), np.float32)
    a[y, x] = 1.0
    return a


def _rel(got, want):
    """The largest |got - want| / |want| (0 where both are 0)."""
    d, w = np.abs(got - want), np.abs(want)
    return float(np.max(np.where(w > 0, d / np.where(w > 0, w, 1.0), np.where(d > 0, np.inf, 0.0))))


@pytest.mark.parametrize('name', sorted(R.CASES))
def test_viterbi_bits(eng, name):
    hm, taps, Rr, sigma, rho, ref = _case(name)
    got = _host(eng.seq_viterbi(_dev(hm), sigma, rho, radius=Rr))
    want = ref['viterbi']
    assert_array_equal(got['path'], want['path'])
    assert_array_equal(got['breaks'], want['breaks'])
    assert_array_equal(got['maxes'].view(np.int64), want['maxes'].view(np.int64))


@pytest.mark.parametrize('name', sorted(R.CASES))
def test_filter_against_the_restatement(eng, name):
    hm, taps, Rr, sigma, rho, ref = _case(name)
    S, T, HH, WW, K = hm.shape
    got = _host(eng.seq_filter(_dev(hm), sigma, rho, radius=Rr))
    for key in ('mirror', 'other'):
        assert_array_equal(got['coords'], ref[key]['coords'])
        assert_array_equal(got['reset'], ref[key]['reset'])
    other = ref['other']      # the order of Z differs from the kernel's: the derived bound
    for t in range(T):
        rel = _rel(got['norm'][:, t], other['norm'][:, t])
        print('%s frame %d: norm differs from the other-order restatement by %.3g relative (bound %.3g)' % (name, t, rel, R.tolerance(t, HH * WW, Rr)))
        assert rel <= R.tolerance(t, HH * WW, Rr)
    rel = _rel(got['state'], other['state'])
    print('%s: state differs by %.3g relative (bound %.3g)' % (name, rel, R.tolerance(T - 1, HH * WW, Rr)))
    assert rel <= R.tolerance(T - 1, HH * WW, Rr)
    belief32 = other['belief'].astype(np.float32)
    assert (np.abs(got['filtered'].astype(np.float64) - other['belief']) <= np.spacing(np.abs(belief32)).astype(np.float64)).all()
    mirror = ref['mirror']      # the kernel's order: the same bits
    assert_array_equal(got['norm'].view(np.int64), mirror['norm'].view(np.int64))
    assert_array_equal(got['state'].view(np.int64), mirror['state'].view(np.int64))
    assert_array_equal(got['filtered'].view(np.int32), mirror['filtered'].view(np.int32))


def test_sequence_1_alone(eng):
    """Sequences are independent: sequence 1 of the two-sequence case gives the bits it gives alone, as a 4-d call."""
    hm, taps, Rr, sigma, rho, _ = _case('odd')
    both_f, both_v = _host(eng.seq_filter(_dev(hm), sigma, rho, radius=Rr)), _host(eng.seq_viterbi(_dev(hm), sigma, rho, radius=Rr))
    one_f, one_v = _host(eng.seq_filter(_dev(hm[1]), sigma, rho, radius=Rr)), _host(eng.seq_viterbi(_dev(hm[1]), sigma, rho, radius=Rr))
    assert one_f['coords'].shape == (hm.shape[1], 2, hm.shape[4]) and one_f['state'].shape == (hm.shape[4],) + hm.shape[2:4]
    for k in one_f:
        assert_array_equal(one_f[k], both_f[k][1])
    for k in one_v:
        assert_array_equal(one_v[k], both_v[k][1])


def test_split_call_and_determinism(eng):
    """T = 6 in one call equals 3 + 3 with the state carried, bit for bit; and a second call gives the first call's bits."""
    hm, taps, Rr, sigma, rho, _ = _case('split')
    t = _dev(hm)
    whole = eng.seq_filter(t, sigma, rho, radius=Rr)
    first = eng.seq_filter(t[:, :3].contiguous(), sigma, rho, radius=Rr)
    second = eng.seq_filter(t[:, 3:].contiguous(), sigma, rho, radius=Rr, state=first['state'])
    again = eng.seq_filter(t, sigma, rho, radius=Rr)
    v1, v2 = eng.seq_viterbi(t, sigma, rho, radius=Rr), eng.seq_viterbi(t, sigma, rho, radius=Rr)
    whole, first, second, again, v1, v2 = (_host(r) for r in (whole, first, second, again, v1, v2))
    for k in ('filtered', 'coords', 'norm', 'reset'):
        assert_array_equal(np.concatenate([first[k], second[k]], axis=1), whole[k])
    assert_array_equal(second['state'].view(np.int64), whole['state'].view(np.int64))
    for k in whole:
        assert_array_equal(again[k], whole[k])
    for k in v1:
        assert_array_equal(v1[k], v2[k])


def _both(eng, hm, rho):
    t = _dev(hm)
    return _host(eng.seq_filter(t, 1.0, rho, radius=1)), _host(eng.seq_viterbi(t, 1.0, rho, radius=1))


def _same_as_ref(f, v, hm, rho):
    taps = P.seq_taps(1.0, 1, hm.shape[4])
    rf, rv = R.seq_filter(hm, taps, rho), R.seq_viterbi(hm, taps, rho)
    for k in ('coords', 'norm', 'reset', 'state'):
        assert_array_equal(f[k], rf[k])
    for k in rv:
        assert_array_equal(v[k], rv[k])


def test_zero_frame_mid_sequence(eng):
    hm = _maps([_delta(3, 9, 1, 2), np.zeros((3, 9)), _delta(3, 9, 1, 5)])
    f, v = _both(eng, hm, 0.05)
    assert_array_equal(f['reset'][0, :, 0], [0, 2, 0])
    assert_array_equal(v['breaks'][0, :, 0], [0, 2, 0])
    assert_array_equal(f['filtered'][0, 1, :, :, 0], np.full((3, 9), np.float32(1.0 / 27.0)))
    assert_array_equal(v['path'][0, :, :, 0], [[1, 2], [1, 5], [1, 5]])
    _same_as_ref(f, v, hm, 0.05)


def test_far_delta_breaks_without_rho_and_jumps_with_it(eng):
    hm = _maps([_delta(3, 9, 1, 0), _delta(3, 9, 1, 8)])
    f, v = _both(eng, hm, 0.0)
    assert_array_equal(f['reset'][0, :, 0], [0, 1])
    assert_array_equal(v['breaks'][0, :, 0], [0, 1])
    assert_array_equal(v['path'][0, :, :, 0], [[1, 0], [1, 8]])
    _same_as_ref(f, v, hm, 0.0)
    f, v = _both(eng, hm, 0.5)
    assert_array_equal(f['reset'][0, :, 0], [0, 0])
    assert_array_equal(v['breaks'][0, :, 0], [0, 0])
    assert_array_equal(v['path'][0, :, :, 0], [[1, 0], [1, 8]])      # the path arrives at the delta
    assert_array_equal(f['coords'][0, :, :, 0], [[1, 0], [1, 8]])
    assert_array_equal(v['maxes'][0, :, 0], [1.0, 0.5 / 27.0])
    _same_as_ref(f, v, hm, 0.5)


def test_equal_maxima_resolve_to_the_lower_index(eng):
    hm = _maps([[[0, 3, 0], [3, 0, 3]]])
    f, v = _both(eng, hm, 0.05)
    assert_array_equal(f['coords'][0, 0, :, 0], [0, 1])
    assert_array_equal(v['path'][0, 0, :, 0], [0, 1])
    # ... and a tie between two sources goes to the lowest offset (tests/test_seq_cpu.py has the reasoning)
    _, v = _both(eng, _maps([[[1, 0, 1, 0, 0]], [[0, 1, 0, 0, 0]]]), 0.0)
    assert_array_equal(v['path'][0, :, :, 0], [[0, 2], [0, 1]])


def test_refused_arguments_touch_nothing(eng):
    """Each JCM_ERR_ARG case and the 8193-cell map: a non-zero status and sentinel-filled outputs left as they were."""
    S, T, HH, WW, K, Rr = 1, 2, 5, 7, 2, 1
    hm = torch.rand(S, T, HH, WW, K, device='cuda:0')
    big = torch.rand(1, 1, 1, 8193, 1, device='cuda:0')
    taps = P.seq_taps(1.0, 16, 16)
    tp = taps.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    outs = {'filtered': torch.full((S, T, HH, WW, K), 7.0, device='cuda:0'), 'coords': torch.full((S, T, 2, K), 7, dtype=torch.int32, device='cuda:0'),
            'norm': torch.full((S, T, K), 7.0, dtype=torch.float64, device='cuda:0'), 'reset': torch.full((S, T, K), 7, dtype=torch.int32, device='cuda:0'),
            'state': torch.full((S, K, HH, WW), 7.0, dtype=torch.float64, device='cuda:0'), 'path': torch.full((S, T, 2, K), 7, dtype=torch.int32, device='cuda:0'),
            'maxes': torch.full((S, T, K), 7.0, dtype=torch.float64, device='cuda:0'), 'breaks': torch.full((S, T, K), 7, dtype=torch.int32, device='cuda:0'),
            'big': torch.full((1, 1, 1, 8193, 1), 7.0, device='cuda:0'), 'big_coords': torch.full((1, 1, 2, 1), 7, dtype=torch.int32, device='cuda:0')}
    torch.cuda.synchronize()
    p, lib, h = eng._p, eng._lib, eng._h
    ok = dict(hm=hm, S=S, T=T, HH=HH, WW=WW, K=K, taps=tp, R=Rr, rho=0.05, coords=outs['coords'], path=outs['path'])
    bad = [dict(S=0), dict(T=0), dict(HH=0), dict(WW=0), dict(K=0), dict(S=-1), dict(K=17), dict(R=-1), dict(R=17), dict(rho=-0.01), dict(rho=1.01),
           dict(rho=float('nan')), dict(hm=None), dict(taps=None), dict(coords=None, path=None),
           dict(hm=big, HH=1, WW=8193, K=1, T=1, coords=outs['big_coords'], path=outs['big_coords']), dict(HH=8193, WW=1), dict(HH=91, WW=91)]
    for change in bad:
        a = dict(ok, **change)
        rc = lib.jcm_seq_filter(h, p(a['hm']), a['S'], a['T'], a['HH'], a['WW'], a['K'], a['taps'], a['R'], a['rho'], p(None),
                                p(outs['big'] if a['hm'] is big else outs['filtered']), p(a['coords']), p(outs['norm']), p(outs['reset']), p(outs['state']))
        assert rc == 1, change
        rc = lib.jcm_seq_viterbi(h, p(a['hm']), a['S'], a['T'], a['HH'], a['WW'], a['K'], a['taps'], a['R'], a['rho'], p(a['path']), p(outs['maxes']),
                                 p(outs['breaks']))
        assert rc == 1, change
    torch.cuda.synchronize()
    for name, t in outs.items():
        assert int((t != 7).sum()) == 0, name
    with pytest.raises(RuntimeError, match=r'jcm_seq_filter failed.*HH \* WW <= 8192'):
        eng.seq_filter(big[0], 1.0, 0.05)
    with pytest.raises(RuntimeError, match=r'jcm_seq_viterbi failed.*rho outside'):
        eng.seq_viterbi(hm, 1.0, 1.5)
    # back-pointers no device can hold: JCM_ERR_STATE with the bytes in the message, before anything is read or launched
    rc = lib.jcm_seq_viterbi(h, p(hm), 1 << 13, 1 << 13, 64, 128, 8, tp, Rr, 0.05, p(outs['path']), p(outs['maxes']), p(outs['breaks']))
    found = re.search(r'need (\d+) bytes of workspace', _lib.last_error())
    assert rc == 2 and found and int(found.group(1)) >= (1 << 26) * 8 * 8192 * 2, _lib.last_error()
    torch.cuda.synchronize()
    for name in ('path', 'maxes', 'breaks'):
        assert int((outs[name] != 7).sum()) == 0, name
    # optional outputs may be NULL
    w3 = P.seq_taps(1.0, 1, K)
    want = R.seq_filter(hm.cpu().numpy(), w3, 0.05)
    coords = torch.empty(S, T, 2, K, dtype=torch.int32, device='cuda:0')
    rc = lib.jcm_seq_filter(h, p(hm), S, T, HH, WW, K, w3.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), 1, 0.05, p(None), p(None), p(coords), p(None), p(None),
                            p(None))
    assert rc == 0
    path = torch.empty(S, T, 2, K, dtype=torch.int32, device='cuda:0')
    assert lib.jcm_seq_viterbi(h, p(hm), S, T, HH, WW, K, w3.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), 1, 0.05, p(path), p(None), p(None)) == 0
    torch.cuda.synchronize()
    assert_array_equal(coords.cpu().numpy(), want['coords'])
    assert_array_equal(path.cpu().numpy(), R.seq_viterbi(hm.cpu().numpy(), w3, 0.05)['path'])
