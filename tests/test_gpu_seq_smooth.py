"""The smoother on the GPU: jcm_seq_smooth (csrc/seq_smooth.hip) against the numpy float64 restatement (tests/seq_smooth_ref.py,
pinned by tests/test_seq_smooth_cpu.py) on the inputs that file builds.  The restatement sums in the kernel's order, so every output is compared
bit for bit: the float64 ones as they are, smoothed and conf as the float32 rounding of the restatement's float64 values, coords exactly (the
seeds leave the reference's gamma a clear first maximum)."""
import ctypes
import re

import numpy as np
import pytest
import torch
from numpy.testing import assert_array_equal

import seq_ref as R
import seq_smooth_ref as SR
import joint_cnn_mrf_amd  # noqa: F401
from joint_cnn_mrf_amd import _lib
from joint_cnn_mrf_amd import predict as P

pytestmark = pytest.mark.gpu
F64 = ('norm', 'mass', 'trans')
F32 = ('smoothed', 'conf')
I32 = ('coords', 'reset', 'cut')


@pytest.fixture(scope='module')
def eng():
    """A bare fp32 handle: the sequence kernels need no parameters."""
    from joint_cnn_mrf_amd.engine import Engine
    e = Engine(device=0)
    yield e
    e.close()


def _dev(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), device='cuda:0', dtype=dtype)


def _host(r):
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in r.items()}


def _same_bits(got, want):
    for k in F64:
        assert_array_equal(got[k].view(np.int64), want[k].view(np.int64), err_msg=k)
    for k in F32:
        assert_array_equal(got[k].view(np.int32), want[k].view(np.int32), err_msg=k)
    for k in I32:
        assert_array_equal(got[k], want[k], err_msg=k)


@pytest.mark.parametrize('name', sorted(SR.CASES))
def test_bits_of_the_restatement(eng, name):
    hm, taps, Rr, sigma, rho, _, ref = SR.case(name)
    S, T, HH, WW, K = hm.shape
    assert (R.top2_gap(ref['gamma']) > 10.0 * R.tolerance(2 * T, HH * WW, Rr)).all()
    t = _dev(hm)
    got = _host(eng.seq_smooth(t, sigma, rho, radius=Rr))
    print('%s: mass within %.3g of 1, %d cuts, %d resets' % (name, np.abs(got['mass'] - 1.0).max(), got['cut'].sum(), got['reset'].sum()))
    _same_bits(got, ref)
    # the forward launch is the filter: norm and reset are its bits
    flt = _host(eng.seq_filter(t, sigma, rho, radius=Rr))
    assert_array_equal(got['norm'].view(np.int64), flt['norm'].view(np.int64))
    assert_array_equal(got['reset'], flt['reset'])


def test_two_sequences_are_two_calls(eng):
    hm, taps, Rr, sigma, rho, _, ref = SR.case('odd')
    assert hm.shape[0] == 2
    both = _host(eng.seq_smooth(_dev(hm), sigma, rho, radius=Rr))
    for s in range(2):
        one = _host(eng.seq_smooth(_dev(hm[s]), sigma, rho, radius=Rr))      # a 4-d call: no S axis in the outputs
        assert one['coords'].shape == (hm.shape[1], 2, hm.shape[4]) and one['trans'].shape == (hm.shape[1], hm.shape[4], 3)
        for k in both:
            assert_array_equal(one[k], both[k][s], err_msg=k)
    again = _host(eng.seq_smooth(_dev(hm), sigma, rho, radius=Rr))
    for k in both:
        assert_array_equal(again[k], both[k], err_msg=k)


def test_zero_frame_splits_the_chain(eng):
    rs = np.random.RandomState(3)
    hm = (rs.rand(1, 5, 3, 9, 1) + 0.05).astype(np.float32)
    hm[0, 2] = 0.0
    taps = P.seq_taps(1.0, 1, 1)
    got = _host(eng.seq_smooth(_dev(hm), 1.0, 0.05, radius=1))
    assert_array_equal(got['reset'][0, :, 0], [0, 0, 2, 0, 0])
    assert_array_equal(got['trans'][0, 2, 0], [0.0, 0.0, 0.0])
    _same_bits(got, SR.seq_smooth(hm, taps, 0.05))
    head = _host(eng.seq_smooth(_dev(hm[:, :2]), 1.0, 0.05, radius=1))      # beta = 1 behind the zero frame
    for k in ('smoothed', 'coords', 'conf', 'trans', 'mass'):
        assert_array_equal(got[k][:, :2], head[k], err_msg=k)


def test_refused_arguments_touch_nothing(eng):
    """Each JCM_ERR_ARG case and the map one cell above the limit: status 1 and sentinel-filled outputs left as they were."""
    S, T, HH, WW, K, Rr = 1, 2, 5, 7, 2, 1
    hm = torch.rand(S, T, HH, WW, K, device='cuda:0')
    big = torch.rand(1, 1, 1, SR.MAX_HW + 1, 1, device='cuda:0')
    taps = P.seq_taps(1.0, 16, 16)
    tp = taps.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    f = lambda shape, dtype=torch.float32: torch.full(shape, 7, dtype=dtype, device='cuda:0')
    outs = {'smoothed': f((S, T, HH, WW, K)), 'coords': f((S, T, 2, K), torch.int32), 'conf': f((S, T, K)), 'norm': f((S, T, K), torch.float64),
            'reset': f((S, T, K), torch.int32), 'mass': f((S, T, K), torch.float64), 'cut': f((S, T, K), torch.int32), 'trans': f((S, T, K, 3), torch.float64),
            'big': f((1, 1, 1, SR.MAX_HW + 1, 1))}
    torch.cuda.synchronize()
    p, lib, h = eng._p, eng._lib, eng._h
    ok = dict(hm=hm, S=S, T=T, HH=HH, WW=WW, K=K, taps=tp, R=Rr, rho=0.05, coords=outs['coords'])
    bad = [dict(S=0), dict(T=0), dict(HH=0), dict(WW=0), dict(K=0), dict(S=-1), dict(K=17), dict(R=-1), dict(R=17), dict(rho=-0.01), dict(rho=1.01),
           dict(rho=float('nan')), dict(hm=None), dict(taps=None), dict(coords=None), dict(hm=big, HH=1, WW=SR.MAX_HW + 1, K=1, T=1),
           dict(HH=SR.MAX_HW + 1, WW=1), dict(HH=79, WW=78), dict(HH=64, WW=128)]

    def call(a):
        return lib.jcm_seq_smooth(h, p(a['hm']), a['S'], a['T'], a['HH'], a['WW'], a['K'], a['taps'], a['R'], a['rho'],
                                  p(outs['big'] if a['hm'] is big else outs['smoothed']), p(a['coords']), p(outs['conf']), p(outs['norm']), p(outs['reset']),
                                  p(outs['mass']), p(outs['cut']), p(outs['trans']))

    for change in bad:
        assert call(dict(ok, **change)) == 1, change
    torch.cuda.synchronize()
    for name, t in outs.items():
        assert int((t != 7).sum()) == 0, name
    with pytest.raises(RuntimeError, match=r'jcm_seq_smooth failed.*HH \* WW <= 6144'):
        eng.seq_smooth(big[0], 1.0, 0.05)
    with pytest.raises(RuntimeError, match=r'jcm_seq_smooth failed.*rho outside'):
        eng.seq_smooth(hm, 1.0, 1.5)
    with pytest.raises(ValueError, match='radius'):
        eng.seq_smooth(hm, 1.0, 0.05, radius=17)
    # beliefs no device can hold: JCM_ERR_STATE with the bytes in the message, before anything is read or launched
    rc = call(dict(ok, S=1 << 13, T=1 << 13, HH=64, WW=96, K=8))
    found = re.search(r'need (\d+) bytes of workspace', _lib.last_error())
    assert rc == 2 and found and int(found.group(1)) >= (1 << 26) * 8 * 6144 * 8, _lib.last_error()
    torch.cuda.synchronize()
    for name, t in outs.items():
        assert int((t != 7).sum()) == 0, name
    # every output but coords may be NULL
    w3 = P.seq_taps(1.0, 1, K)
    coords = torch.empty(S, T, 2, K, dtype=torch.int32, device='cuda:0')
    rc = lib.jcm_seq_smooth(h, p(hm), S, T, HH, WW, K, w3.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), 1, 0.05, p(None), p(coords), p(None), p(None),
                            p(None), p(None), p(None), p(None))
    assert rc == 0, _lib.last_error()
    torch.cuda.synchronize()
    assert_array_equal(coords.cpu().numpy(), SR.seq_smooth(hm.cpu().numpy(), w3, 0.05)['coords'])


def test_fit_of_the_planted_clip(eng):
    """Engine.seq_fit runs the restatement's EM: the M-step is host float64 on sums of bit-equal device outputs."""
    hm, ref, _ = SR.planted_case()
    c = SR.PLANTED
    got = eng.seq_fit(_dev(hm), c['start'] * np.array(c['sigma']), c['rho'], iters=c['iters'], radius=c['radius'])
    print('sigma %s, rho %.6g, loglik %s' % (got['sigma'], got['rho'], got['loglik']))
    assert_array_equal(got['sigma'], ref['sigma'])
    assert got['rho'] == ref['rho']
    assert_array_equal(got['loglik'], ref['loglik'])
    assert_array_equal(got['clamped'], ref['clamped'])
    assert len(got['history']) == c['iters'] + 1
    fixed = eng.seq_fit(_dev(hm), 2.0, 0.07, iters=1, radius=c['radius'], fit_rho=False)
    assert fixed['rho'] == 0.07 and fixed['sigma'].shape == (2,)


def test_asymmetric_taps_through_the_c_abi(eng):
    """Taps that prefer motion towards larger rows and columns, which seq_taps never builds: a kernel whose backward pass indexed like the forward one
    would smooth the other way.  Odd sizes, two joints with different rows of taps (one of radius-2 shape), more than one cell per thread."""
    S, T, HH, WW, K, Rr = 1, 4, 37, 53, 2, 2
    hm = R.random_maps((S, T, HH, WW, K), 77)
    taps = np.array([[0.0, 0.05, 0.25, 0.70, 0.0], [0.02, 0.08, 0.15, 0.30, 0.45]])
    want = SR.seq_smooth(hm, taps, 0.05)
    mirrored = SR.seq_smooth(hm, np.ascontiguousarray(taps[:, ::-1]), 0.05)
    assert np.abs(want['gamma'] - mirrored['gamma']).max() > 1e-3 and (want['trans'] != mirrored['trans']).any()      # the case does tell the two apart
    assert (R.top2_gap(want['gamma']) > 10.0 * R.tolerance(2 * T, HH * WW, Rr)).all()
    f = lambda shape, dtype=torch.float32: torch.empty(shape, dtype=dtype, device='cuda:0')
    out = {'smoothed': f((S, T, HH, WW, K)), 'coords': f((S, T, 2, K), torch.int32), 'conf': f((S, T, K)), 'norm': f((S, T, K), torch.float64),
           'reset': f((S, T, K), torch.int32), 'mass': f((S, T, K), torch.float64), 'cut': f((S, T, K), torch.int32), 'trans': f((S, T, K, 3), torch.float64)}
    t = _dev(hm)
    p = eng._p
    rc = eng._lib.jcm_seq_smooth(eng._h, p(t), S, T, HH, WW, K, taps.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), Rr, 0.05, p(out['smoothed']), p(out['coords']),
                                 p(out['conf']), p(out['norm']), p(out['reset']), p(out['mass']), p(out['cut']), p(out['trans']))
    assert rc == 0, _lib.last_error()
    _same_bits(_host(out), want)
