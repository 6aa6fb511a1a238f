"""Several torso tracks on the GPU: jcm_seq_tracks_viterbi and jcm_seq_tracks_filter (csrc/seq_tracks.hip) against the numpy
restatement tests/seq_tracks_ref.py, which masks and calls tests/seq_ref.py at K = 1 in the kernel's summation order.  The exclusion is
comparisons of integers and the recurrence is seq_ref's, so EVERY output -- Viterbi's and the filter's, state_out and the float32 beliefs
included -- is compared bit for bit.  The shapes: the smallest map with several rows per thread stride (7x9), the tower's 60x90, and 64x128,
the 8192-cell limit; every listed T, S, M, D, R and rho occurs, and every map size meets T = 1, 2 and 37."""
import ctypes
import functools
import re

import numpy as np
import pytest
import torch
from numpy.testing import assert_array_equal

import seq_ref as R
import seq_tracks_ref as TR
import joint_cnn_mrf_amd  # noqa: F401
from joint_cnn_mrf_amd import _lib
from joint_cnn_mrf_amd import predict as P

pytestmark = pytest.mark.gpu
SIGMA = 1.5
# name: (HH, WW, T, S, M, D, R, rho)
CASES = {
    'tiny_one_frame': (7, 9, 1, 1, 1, 0, 0, 0.0),
    'tiny_two_frames': (7, 9, 2, 3, 2, 2, 5, 0.05),
    'tiny_long': (7, 9, 37, 1, 4, 0, 5, 0.05),
    'tiny_all_excluded': (7, 9, 37, 3, 4, 64, 0, 0.0),
    'real_one_frame': (60, 90, 1, 3, 4, 2, 5, 0.05),
    'real_two_frames': (60, 90, 2, 1, 2, 64, 5, 0.0),
    'real_long': (60, 90, 37, 3, 4, 2, 5, 0.05),
    'real_radius0': (60, 90, 37, 1, 2, 0, 0, 0.05),
    'limit_one_frame': (64, 128, 1, 1, 2, 2, 0, 0.0),
    'limit_two_frames': (64, 128, 2, 3, 4, 64, 5, 0.05),
    'limit_long': (64, 128, 37, 1, 4, 2, 5, 0.05),
    'limit_one_track': (64, 128, 37, 1, 1, 2, 5, 0.0),
}
INT_VIEW = {np.dtype(np.float32): np.int32, np.dtype(np.float64): np.int64}


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


def _same_bits(got, want, what):
    for k in got:
        g, w = got[k], want[k]
        assert g.shape == w.shape and g.dtype == w.dtype, (what, k, g.shape, w.shape, g.dtype, w.dtype)
        view = INT_VIEW.get(g.dtype)
        assert_array_equal(g.view(view) if view else g, w.view(view) if view else w, err_msg='%s: %s' % (what, k))


@functools.lru_cache(maxsize=None)
def _case(name):
    """The maps of a case and the restatement's results, computed once and never written to."""
    HH, WW, T, S, M, D, Rr, rho = CASES[name]
    hm = R.random_maps((S, T, HH, WW, 1), 4000 + sorted(CASES).index(name))[..., 0]
    taps = P.seq_taps(SIGMA, Rr, 1)
    return hm, {'viterbi': TR.seq_tracks_viterbi(hm, M, taps, rho, D), 'filter': TR.seq_tracks_filter(hm, M, taps, rho, D)}


def _plateaus():
    """Exact ties: two equal 3x3 plateaus and two equal single cells per frame, moving by one cell; dyadic values."""
    hm = np.zeros((2, 4, 9, 12), np.float32)
    for s in range(2):
        for t in range(4):
            hm[s, t, 1:4, 1 + t:4 + t] = 0.5
            hm[s, t, 5:8, 7 - t:10 - t] = 0.5
            hm[s, t, 0, 11] = hm[s, t, 8, 0] = 0.25 if s else 0.5
    return hm


@pytest.mark.parametrize('name', sorted(CASES))
def test_viterbi_bits(eng, name):
    HH, WW, T, S, M, D, Rr, rho = CASES[name]
    hm, want = _case(name)
    got = _host(eng.seq_tracks(_dev(hm), M, SIGMA, rho, radius=Rr, exclude=D, mode='viterbi'))
    assert sorted(got) == ['breaks', 'maxes', 'path', 'value']
    _same_bits(got, want['viterbi'], name)


@pytest.mark.parametrize('name', sorted(CASES))
def test_filter_bits(eng, name):
    HH, WW, T, S, M, D, Rr, rho = CASES[name]
    hm, want = _case(name)
    got = _host(eng.seq_tracks(_dev(hm), M, SIGMA, rho, radius=Rr, exclude=D, mode='filter', want_filtered=True))
    assert sorted(got) == ['coords', 'filtered', 'norm', 'reset', 'state', 'value']
    _same_bits(got, want['filter'], name)


@pytest.mark.parametrize('rho', [0.0, 0.05])
def test_ties_and_plateaus(eng, rho):
    hm = _plateaus()
    taps = P.seq_taps(1.0, 2, 1)
    for D in (0, 1):
        got = _host(eng.seq_tracks(_dev(hm), 3, 1.0, rho, radius=2, exclude=D, mode='viterbi'))
        _same_bits(got, TR.seq_tracks_viterbi(hm, 3, taps, rho, D), 'plateaus viterbi D=%d' % D)
        got = _host(eng.seq_tracks(_dev(hm), 3, 1.0, rho, radius=2, exclude=D, mode='filter', want_filtered=True))
        _same_bits(got, TR.seq_tracks_filter(hm, 3, taps, rho, D), 'plateaus filter D=%d' % D)
    # clip 1, whose single cells are lower than its plateaus: track 0 starts at the first cell of the first plateau
    assert_array_equal(got['coords'][1, 0, 0], [1, 1])


@pytest.mark.parametrize('name', ['tiny_long', 'real_long', 'limit_two_frames'])
def test_track_0_is_the_single_track(eng, name):
    HH, WW, T, S, M, D, Rr, rho = CASES[name]
    hm, _ = _case(name)
    t = _dev(hm)
    v, f = _host(eng.seq_tracks(t, M, SIGMA, rho, radius=Rr, exclude=D)), _host(eng.seq_tracks(t, M, SIGMA, rho, radius=Rr, exclude=D, mode='filter', want_filtered=True))
    v1, f1 = _host(eng.seq_viterbi(t.unsqueeze(-1), SIGMA, rho, radius=Rr)), _host(eng.seq_filter(t.unsqueeze(-1), SIGMA, rho, radius=Rr))
    _same_bits({k: v[k][:, 0] for k in v1}, {k: a[..., 0] for k, a in v1.items()}, name)
    _same_bits({k: f[k][:, 0] for k in ('coords', 'norm', 'reset', 'filtered')}, {k: f1[k][..., 0] for k in ('coords', 'norm', 'reset', 'filtered')}, name)
    _same_bits({'state': f['state'][:, 0]}, {'state': f1['state'].reshape(S, HH * WW)}, name)


def test_filter_split_at_every_frame(eng):
    """A T = 5 clip cut at each of its four frame boundaries, the states carried: the bits of one call.  A 3-d map gives tensors without S."""
    hm = R.random_maps((2, 5, 13, 17, 1), 4100)[..., 0]
    t = _dev(hm)
    whole = _host(eng.seq_tracks(t, 3, SIGMA, 0.05, exclude=2, mode='filter', want_filtered=True))
    for cut in range(1, 5):
        a = eng.seq_tracks(t[:, :cut].contiguous(), 3, SIGMA, 0.05, exclude=2, mode='filter', want_filtered=True)
        b = eng.seq_tracks(t[:, cut:].contiguous(), 3, SIGMA, 0.05, exclude=2, mode='filter', want_filtered=True, state=a['state'])
        a, b = _host(a), _host(b)
        joined = {k: np.concatenate([a[k], b[k]], axis=2) for k in ('coords', 'norm', 'reset', 'value', 'filtered')}
        joined['state'] = b['state']
        _same_bits(joined, whole, 'cut at %d' % cut)
    one = _host(eng.seq_tracks(t[1], 3, SIGMA, 0.05, exclude=2, mode='filter', want_filtered=True))
    assert one['coords'].shape == (3, 5, 2) and one['state'].shape == (3, 13 * 17)
    _same_bits(one, {k: v[1] for k, v in whole.items()}, 'clip 1 alone')


def test_refused_arguments_touch_nothing(eng):
    """Each JCM_ERR_ARG case, the 8193-cell map included: status 1 and sentinel-filled outputs left as they were."""
    S, T, HH, WW, M, Rr = 1, 2, 5, 7, 2, 1
    hm = torch.rand(S, T, HH, WW, device='cuda:0')
    big = torch.rand(1, 1, 1, 8193, device='cuda:0')
    tp = P.seq_taps(1.0, 16, 1).ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    i32 = dict(dtype=torch.int32, device='cuda:0')
    f64 = dict(dtype=torch.float64, device='cuda:0')
    outs = {'cells': torch.full((S, 4, T, 2), 7, **i32), 'num': torch.full((S, 4, T), 7.0, **f64), 'flag': torch.full((S, 4, T), 7, **i32),
            'value': torch.full((S, 4, T), 7.0, device='cuda:0'), 'state': torch.full((S, 4, HH * WW), 7.0, **f64),
            'filtered': torch.full((S, 4, T, HH, WW), 7.0, device='cuda:0'), 'big': torch.full((1, 4, 1, 8193), 7.0, device='cuda:0')}
    torch.cuda.synchronize()
    p, lib, h = eng._p, eng._lib, eng._h
    ok = dict(hm=hm, S=S, T=T, HH=HH, WW=WW, M=M, taps=tp, R=Rr, rho=0.05, D=2, cells=outs['cells'], value=outs['value'])
    bad = [dict(S=0), dict(T=0), dict(HH=0), dict(WW=0), dict(S=-1), dict(R=-1), dict(R=17), dict(rho=-0.01), dict(rho=1.01), dict(rho=float('nan')),
           dict(M=0), dict(M=5), dict(M=-1), dict(D=-1), dict(D=65), dict(hm=None), dict(taps=None), dict(cells=None), dict(value=None),
           dict(hm=big, HH=1, WW=8193, T=1), dict(HH=8193, WW=1), dict(HH=91, WW=91)]
    for change in bad:
        a = dict(ok, **change)
        rc = lib.jcm_seq_tracks_filter(h, p(a['hm']), a['S'], a['T'], a['HH'], a['WW'], a['M'], a['taps'], a['R'], a['rho'], a['D'], p(None),
                                       p(outs['big'] if a['hm'] is big else outs['filtered']), p(a['cells']), p(outs['num']), p(outs['flag']), p(outs['state']),
                                       p(a['value']))
        assert rc == 1, change
        rc = lib.jcm_seq_tracks_viterbi(h, p(a['hm']), a['S'], a['T'], a['HH'], a['WW'], a['M'], a['taps'], a['R'], a['rho'], a['D'], p(a['cells']),
                                        p(outs['num']), p(outs['flag']), p(a['value']))
        assert rc == 1, change
    torch.cuda.synchronize()
    for name, t in outs.items():
        assert int((t != 7).sum()) == 0, name
    with pytest.raises(RuntimeError, match=r'jcm_seq_tracks_viterbi failed.*HH \* WW <= 8192'):
        eng.seq_tracks(big[0], 2, 1.0, 0.05)
    with pytest.raises(RuntimeError, match=r'jcm_seq_tracks_filter failed.*1 <= M <= 4'):
        eng.seq_tracks(hm, 5, 1.0, 0.05, mode='filter')
    with pytest.raises(RuntimeError, match=r'jcm_seq_tracks_viterbi failed.*0 <= D <= 64'):
        eng.seq_tracks(hm, 2, 1.0, 0.05, exclude=65)
    # back-pointers no device can hold: JCM_ERR_STATE with the bytes of ONE pass in the message, before anything is read or launched
    rc = lib.jcm_seq_tracks_viterbi(h, p(hm), 1 << 14, 1 << 14, 64, 128, 4, tp, Rr, 0.05, 2, p(outs['cells']), p(outs['num']), p(outs['flag']), p(outs['value']))
    found = re.search(r'need (\d+) bytes of workspace', _lib.last_error())
    assert rc == 2 and found and (1 << 28) * 8192 * 2 <= int(found.group(1)) < (1 << 28) * 8192 * 4, _lib.last_error()
    torch.cuda.synchronize()
    for name, t in outs.items():
        assert int((t != 7).sum()) == 0, name
    # optional outputs may be NULL
    taps = P.seq_taps(1.0, 1, 1)
    t1 = taps.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    cells, value = torch.empty(S, M, T, 2, **i32), torch.empty(S, M, T, device='cuda:0')
    assert lib.jcm_seq_tracks_filter(h, p(hm), S, T, HH, WW, M, t1, 1, 0.05, 2, p(None), p(None), p(cells), p(None), p(None), p(None), p(value)) == 0
    want = TR.seq_tracks_filter(hm.cpu().numpy(), M, taps, 0.05, 2)
    torch.cuda.synchronize()
    assert_array_equal(cells.cpu().numpy(), want['coords'])
    assert_array_equal(value.cpu().numpy(), want['value'])
    assert lib.jcm_seq_tracks_viterbi(h, p(hm), S, T, HH, WW, M, t1, 1, 0.05, 2, p(cells), p(None), p(None), p(value)) == 0
    want = TR.seq_tracks_viterbi(hm.cpu().numpy(), M, taps, 0.05, 2)
    torch.cuda.synchronize()
    assert_array_equal(cells.cpu().numpy(), want['path'])
    assert_array_equal(value.cpu().numpy(), want['value'])
