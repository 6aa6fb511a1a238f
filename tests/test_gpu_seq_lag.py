"""The fixed-lag smoother on the GPU: jcm_seq_smooth_lag (csrc/seq_smooth.hip) against the restatement of its definition
(tests/seq_lag_ref.py, pinned by tests/test_seq_lag_cpu.py): the offline restatement on the truncated clip, per emitted frame.  Every output is
compared bit for bit, as tests/test_gpu_seq_smooth.py compares: the float64 ones as they are, smoothed and conf as the float32 rounding of the
restatement's float64 values, coords exactly (the seeds leave every truncated gamma a clear first maximum)."""
import ctypes

import numpy as np
import pytest
import torch
from numpy.testing import assert_array_equal

import seq_lag_ref as LR
import seq_ref as R
import seq_smooth_ref as SR
import joint_cnn_mrf_amd  # noqa: F401
from joint_cnn_mrf_amd import _lib
from joint_cnn_mrf_amd import predict as P

pytestmark = pytest.mark.gpu
F64 = ('norm', 'mass')
F32 = ('smoothed', 'conf')
I32 = ('coords', 'reset', 'cut', 'lag')
OUTPUTS = F64 + F32 + I32


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
    return {k: v.cpu().numpy() for k, v in r.items() if k != 'state'}


def _same_bits(got, want, keys=OUTPUTS):
    for k in keys:
        assert got[k].shape == want[k].shape, (k, got[k].shape, want[k].shape)
        if k in F64:
            assert_array_equal(got[k].view(np.int64), want[k].view(np.int64), err_msg=k)
        elif k in F32:
            assert_array_equal(got[k].view(np.int32), want[k].view(np.int32), err_msg=k)
        else:
            assert_array_equal(got[k], want[k], err_msg=k)


def _pushed(eng, hm, sigma, rho, Rr, L, splits, flush_last=True):
    """The clip through Engine.seq_smooth_lag by the schedule -> one host dict per push (and the last state)."""
    t = _dev(hm)
    state, at, pushes = None, 0, []
    for i, n in enumerate(splits):
        r = eng.seq_smooth_lag(t[:, at:at + n].contiguous(), sigma, rho, L, radius=Rr, state=state, flush=flush_last and i == len(splits) - 1,
                               want_smoothed=True)
        state, at = r['state'], at + n
        pushes.append(_host(r))
    return pushes, state


def _lags(name):
    T = LR.CASES[name][1]
    return sorted({L for L in (1, 2, T - 1, T + 3) if L >= 1})


SMALL = ('split', 'odd', 'vector', 'clipped', 'one_frame', 'radius0', 'rho0', 'rho1')


@pytest.mark.parametrize('name,L', [(n, L) for n in SMALL for L in _lags(n)] + [('real', 2), ('limit', 1)])
def test_bits_of_the_restatement(eng, name, L):
    hm, taps, Rr, sigma, rho, _, prefixes = LR.case(name)
    S, T, HH, WW, K = hm.shape
    assert LR.gaps_hold(prefixes, HH * WW, Rr)
    want = LR.case_lag(name, L)[0]
    (got,), state = _pushed(eng, hm, sigma, rho, Rr, L, (T,))
    print('%s L=%d: mass within %.3g of 1, %d cuts, %d resets, lags %s' % (name, L, np.abs(got['mass'] - 1.0).max(), got['cut'].sum(), got['reset'].sum(),
                                                                          got['lag'].tolist()))
    assert state is None and got['coords'].shape == (S, T, 2, K)
    _same_bits(got, want)


@pytest.mark.parametrize('name', ('split', 'odd'))
def test_a_spanning_lag_is_the_offline_smoother(eng, name):
    hm, taps, Rr, sigma, rho, _, _ = LR.case(name)
    T = hm.shape[1]
    off = _host(eng.seq_smooth(_dev(hm), sigma, rho, radius=Rr))
    for L in (T - 1, T + 3):
        (got,), _ = _pushed(eng, hm, sigma, rho, Rr, L, (T,))
        _same_bits(got, off, keys=('smoothed', 'coords', 'conf', 'mass', 'cut', 'norm', 'reset'))
        assert_array_equal(got['lag'], np.arange(T - 1, -1, -1))


SCHEDULES = ((1, 1, 1, 1, 1, 1), (2, 4), (4, 2), (6,), (1, 5))


def test_any_split_gives_the_same_bits(eng):
    hm, taps, Rr, sigma, rho, _, _ = LR.case('split')
    S, T, HH, WW, K = hm.shape
    L = 2
    want = LR.joined(LR.case_lag('split', L), OUTPUTS)
    for splits in SCHEDULES:
        pushes, state = _pushed(eng, hm, sigma, rho, Rr, L, splits)
        assert state is None
        assert [p['coords'].shape[1] for p in pushes] == LR.emitted_counts(splits, L), splits
        for p, ref in zip(pushes, LR.case_lag('split', L, splits)):
            _same_bits(p, ref)
        _same_bits(LR.joined(pushes, OUTPUTS), want)
    # a push that emits nothing: zero-length outputs and a state that holds the frame
    r = eng.seq_smooth_lag(_dev(hm[:, :1]), sigma, rho, L, radius=Rr, want_smoothed=True)
    got = _host(r)
    assert got['coords'].shape == (S, 0, 2, K) and got['smoothed'].shape == (S, 0, HH, WW, K) and got['lag'].shape == (0,)
    assert r['state'] is not None and r['state']['hm'].shape == (S, 1, HH, WW, K) and r['state']['belief'].shape == (S * K, 1, HH * WW)
    # without a flush the last L frames stay pending
    pushes, state = _pushed(eng, hm, sigma, rho, Rr, L, (4, 2), flush_last=False)
    assert [p['coords'].shape[1] for p in pushes] == [2, 2] and state['hm'].shape[1] == L
    for p, ref in zip(pushes, LR.case_lag('split', L, (4, 2), flush_last=False)):
        _same_bits(p, ref)
    # a flush with no new frame ends the clip
    rest = _host(eng.seq_smooth_lag(_dev(hm[:, :0]), sigma, rho, L, radius=Rr, state=state, flush=True, want_smoothed=True))
    _same_bits(LR.joined(pushes + [rest], OUTPUTS), want)


def test_zero_frame_splits_the_chain_across_a_push(eng):
    rs = np.random.RandomState(3)
    hm = (rs.rand(1, 5, 3, 9, 1) + 0.05).astype(np.float32)
    hm[0, 2] = 0.0
    taps = P.seq_taps(1.0, 1, 1)
    pushes, _ = _pushed(eng, hm, 1.0, 0.05, 1, 3, (2, 3))
    assert [p['coords'].shape[1] for p in pushes] == [0, 5]
    got = LR.joined(pushes, OUTPUTS)
    assert_array_equal(got['reset'][0, :, 0], [0, 0, 2, 0, 0])
    _same_bits(got, LR.joined(LR.seq_smooth_lag(hm, taps, 0.05, 3, (2, 3)), OUTPUTS))
    # beta = 1 behind the zero frame: frames 0 and 1 are what the clip's first two frames give alone
    head = _host(eng.seq_smooth(_dev(hm[:, :2]), 1.0, 0.05, radius=1))
    for k in ('smoothed', 'coords', 'conf', 'mass'):
        assert_array_equal(got[k][:, :2], head[k], err_msg=k)


def test_sequence_joint_and_frame_index_one_launch(eng):
    """S = 2, K = 3, E = 5 in one backward launch: every (s, k, e) group writes its own frame."""
    hm, taps, Rr, sigma, rho, _, _ = LR.case('odd')
    assert hm.shape[:2] == (2, 5) and hm.shape[4] == 3
    (got,), _ = _pushed(eng, hm, sigma, rho, Rr, 1, (5,))
    assert got['coords'].shape == (2, 5, 2, 3)
    _same_bits(got, LR.case_lag('odd', 1)[0])
    assert len({got['smoothed'][s, e, :, :, k].tobytes() for s in range(2) for e in range(5) for k in range(3)}) == 30


def test_two_sequences_are_two_calls(eng):
    hm, taps, Rr, sigma, rho, _, _ = LR.case('odd')
    both, _ = _pushed(eng, hm, sigma, rho, Rr, 2, (2, 3))
    for s in range(2):
        state, at = None, 0
        for i, n in enumerate((2, 3)):
            r = eng.seq_smooth_lag(_dev(hm[s, at:at + n]), sigma, rho, 2, radius=Rr, state=state, flush=i == 1, want_smoothed=True)      # 4-d: no S axis
            state, at = r['state'], at + n
            one = _host(r)
            assert one['coords'].shape == (both[i]['coords'].shape[1], 2, hm.shape[4])
            for k in OUTPUTS:
                assert_array_equal(one[k], both[i][k] if k == 'lag' else both[i][k][s], err_msg=k)


def test_refused_arguments_touch_nothing(eng):
    """Each JCM_ERR_ARG case: status 1, nothing launched, sentinel-filled outputs and window left as they were."""
    S, W, HH, WW, K, Rr, L = 1, 3, 5, 7, 2, 1, 1
    hm = torch.rand(S, W, HH, WW, K, device='cuda:0')
    big = torch.rand(1, 1, 1, SR.MAX_HW + 1, 1, device='cuda:0')
    taps = P.seq_taps(1.0, 16, 16)
    tp = taps.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    f = lambda shape, dtype=torch.float32: torch.full(shape, 7, dtype=dtype, device='cuda:0')
    outs = {'belief': f((S * K, W, HH * WW), torch.float64), 'norm': f((S, W, K), torch.float64), 'reset': f((S, W, K), torch.int32),
            'smoothed': f((S, W, HH, WW, K)), 'coords': f((S, W, 2, K), torch.int32), 'conf': f((S, W, K)), 'mass': f((S, W, K), torch.float64),
            'cut': f((S, W, K), torch.int32), 'big': f((1, 1, 1, SR.MAX_HW + 1, 1)), 'big_belief': f((1, 1, SR.MAX_HW + 1), torch.float64)}
    torch.cuda.synchronize()
    p, lib, h = eng._p, eng._lib, eng._h
    ok = dict(hm=hm, S=S, W=W, P=0, HH=HH, WW=WW, K=K, taps=tp, R=Rr, rho=0.05, L=L, flush=0, belief=outs['belief'], norm=outs['norm'], reset=outs['reset'],
              coords=outs['coords'])
    bad = [dict(S=0), dict(W=0), dict(HH=0), dict(WW=0), dict(K=0), dict(S=-1), dict(W=-1), dict(K=17), dict(R=-1), dict(R=17), dict(rho=-0.01),
           dict(rho=1.01), dict(rho=float('nan')), dict(hm=None), dict(taps=None),
           dict(hm=big, HH=1, WW=SR.MAX_HW + 1, K=1, W=1, flush=1, belief=outs['big_belief']), dict(HH=SR.MAX_HW + 1, WW=1), dict(HH=79, WW=78),
           dict(HH=64, WW=128),
           dict(P=-1), dict(P=W + 1), dict(L=0), dict(L=-1), dict(flush=2), dict(flush=-1), dict(belief=None), dict(norm=None), dict(reset=None),
           dict(coords=None), dict(coords=None, flush=1), dict(coords=None, L=5, flush=1), dict(S=1 << 20, W=1 << 10), dict(S=1 << 28, W=4, K=2)]

    def call(a):
        return lib.jcm_seq_smooth_lag(h, p(a['hm']), a['S'], a['W'], a['P'], a['HH'], a['WW'], a['K'], a['taps'], a['R'], a['rho'], a['L'], a['flush'],
                                      p(a['belief']), p(a['norm']), p(a['reset']), p(outs['big'] if a['hm'] is big else outs['smoothed']), p(a['coords']),
                                      p(outs['conf']), p(outs['mass']), p(outs['cut']))

    for change in bad:
        assert call(dict(ok, **change)) == 1, change
    assert call(dict(ok, L=0)) == 1 and 'jcm_seq_filter' in _lib.last_error()      # lag 0 is the filter, and the message says where it is
    torch.cuda.synchronize()
    for name, t in outs.items():
        assert int((t != 7).sum()) == 0, name
    with pytest.raises(ValueError, match='seq_filter'):
        eng.seq_smooth_lag(hm, 1.0, 0.05, 0)
    with pytest.raises(RuntimeError, match=r'jcm_seq_smooth_lag failed.*HH \* WW <= 6144'):
        eng.seq_smooth_lag(big[0], 1.0, 0.05, 1)
    with pytest.raises(ValueError, match='no pending frame'):
        eng.seq_smooth_lag(hm[:, :0], 1.0, 0.05, 1)
    state = eng.seq_smooth_lag(hm, 1.0, 0.05, 2, radius=Rr)['state']
    for other in (dict(lag=3), dict(sigma=1.5), dict(rho=0.1), dict(hm=hm[:, :, :4].contiguous())):
        with pytest.raises(ValueError, match='state is not'):
            eng.seq_smooth_lag(**dict(dict(hm=hm, sigma=1.0, rho=0.05, lag=2, radius=Rr, state=state), **other))
    # nothing emitted: coords and every other output may be NULL, and the window is filled with the filter's values
    w3 = P.seq_taps(1.0, 1, K)
    rc = lib.jcm_seq_smooth_lag(h, p(hm), S, 1, 0, HH, WW, K, w3.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), 1, 0.05, 1, 0, p(outs['belief']),
                                p(outs['norm']), p(outs['reset']), p(None), p(None), p(None), p(None), p(None))
    assert rc == 0, _lib.last_error()
    torch.cuda.synchronize()
    flt = R.seq_filter(hm[:, :1].cpu().numpy(), w3, 0.05)
    # (a window of one frame: [S,1,K] and [S*K][1][HW] are the front of the buffers)
    assert_array_equal(outs['norm'].cpu().numpy().reshape(-1)[:S * K].reshape(S, 1, K), flt['norm'])
    assert_array_equal(outs['belief'].cpu().numpy().reshape(-1)[:S * K * HH * WW].reshape(S, K, HH, WW), flt['belief'][:, 0].transpose(0, 3, 1, 2))
    assert int((outs['coords'] != 7).sum()) == 0


def test_pending_frames_beyond_the_lag_are_legal(eng):
    """P > L: a caller may hold more pending frames than the lag needs (here the whole clip, emitted by a flush with no new frame)."""
    hm, taps, Rr, sigma, rho, _, _ = LR.case('split')
    S, T, HH, WW, K = hm.shape
    t = _dev(hm)
    tp = taps.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    f = lambda shape, dtype=torch.float32: torch.zeros(shape, dtype=dtype, device='cuda:0')
    win = {'belief': f((S * K, T, HH * WW), torch.float64), 'norm': f((S, T, K), torch.float64), 'reset': f((S, T, K), torch.int32)}
    out = {'smoothed': f((S, T, HH, WW, K)), 'coords': f((S, T, 2, K), torch.int32), 'conf': f((S, T, K)), 'mass': f((S, T, K), torch.float64),
           'cut': f((S, T, K), torch.int32)}
    p, lib, h = eng._p, eng._lib, eng._h

    def call(P_, L, flush, E_out):
        return lib.jcm_seq_smooth_lag(h, p(t), S, T, P_, HH, WW, K, tp, Rr, rho, L, flush, p(win['belief']), p(win['norm']), p(win['reset']),
                                      *(p(out[k]) if E_out else p(None) for k in ('smoothed', 'coords', 'conf', 'mass', 'cut')))

    assert call(0, T, 0, False) == 0, _lib.last_error()      # L = T: the forward launch alone
    assert call(T, 2, 1, True) == 0, _lib.last_error()       # P = W = T > L: the backward launch alone
    got = dict(_host(out), **_host(win))
    want = LR.case_lag('split', 2)[0]
    _same_bits(got, want, keys=('smoothed', 'coords', 'conf', 'mass', 'cut', 'norm', 'reset'))
