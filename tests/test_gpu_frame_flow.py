"""jcm_frame_flow and jcm_hm_flow_pool on the GPU (csrc/frame_flow.hip) against their numpy restatements (tests/frame_flow_ref.py,
pinned by tests/test_frame_flow_cpu.py).  The matching is integer arithmetic with order-free sums and the pooling float64 in one fixed order:
everything is compared bit for bit.  The shapes are the smallest at which each path of the kernels runs -- FF.FLOW_CASES and FF.POOL_CASES say
which --, one full-size pair whose strided loops run past their first trip, and one clip with more work groups than the grid's cap."""
import ctypes

import numpy as np
import pytest
import torch
from numpy.testing import assert_array_equal

import frame_flow_ref as FF
import joint_cnn_mrf_amd  # noqa: F401

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def eng():
    """A bare fp32 handle: the kernels need no parameters."""
    from joint_cnn_mrf_amd.engine import Engine
    e = Engine(device=0)
    yield e
    e.close()


def _dev(a):
    return torch.as_tensor(np.array(a), device='cuda:0')      # a copy: the shared inputs are read-only


def _run(eng, x, rect, D, ref):
    r = eng.frame_flow(x if isinstance(x, torch.Tensor) else _dev(x), rect, ref, search=D)
    torch.cuda.synchronize()
    assert r['flow'].dtype == torch.int32 and r['sad'].dtype == torch.int32
    return r['flow'].cpu().numpy(), r['sad'].cpu().numpy()


def _equal(got, want):
    assert_array_equal(got[0], want[0])
    assert_array_equal(got[1], want[1])


# ------------------------------------------------------------------ the matching
@pytest.mark.parametrize('name', [c[0] for c in FF.FLOW_CASES])
def test_small_cases(eng, name):
    x, rect, D, ref = FF.flow_case(name)
    _equal(_run(eng, x, rect, D, ref), FF.flow_case_expected(name))


def test_ref_on_the_device_and_a_misaligned_base(eng):
    """ref as a device tensor, and the frames at a base one byte off a dword (the luma pass reads bytes: nothing may depend on the alignment)."""
    name = 'cut on every side'
    x, rect, D, ref = FF.flow_case(name)
    buf = torch.zeros(x.size + 8, dtype=torch.uint8, device='cuda:0')
    xd = buf[1:1 + x.size].view(x.shape)
    xd.copy_(torch.as_tensor(x.copy()))
    assert xd.data_ptr() % 4 == 1
    _equal(_run(eng, xd, rect, D, _dev(ref)), FF.flow_case_expected(name))


def test_bars_have_no_say(eng):
    name = 'cut on every side'
    x, rect, D, ref = FF.flow_case(name)
    y0, x0, ch, cw = rect
    y = np.random.default_rng(4).integers(0, 256, size=x.shape).astype(np.uint8)
    y[:, y0:y0 + ch, x0:x0 + cw] = x[:, y0:y0 + ch, x0:x0 + cw]
    _equal(_run(eng, y, rect, D, ref), FF.flow_case_expected(name))


def test_ties(eng):
    flat = np.full((2, 40, 56, 3), 77, np.uint8)
    flat[:, :3] = 200                                         # bars of another value
    ref = np.array([[1], [0]], np.int32)
    for x in (flat, np.stack([FF.noise_clip(1, 40, 56, 3)[0]] * 2)):
        flow, sad = _run(eng, x, (3, 5, 30, 41), 3, ref)
        assert not flow.any() and not sad.any()


def test_planted_motion(eng):
    x, ref = FF.planted_pair(), np.array([[1], [0]], np.int32)
    got = _run(eng, x, FF.PLANT_RECT, FF.PLANT_D, ref)
    _equal(got, FF.frame_flow(x, FF.PLANT_RECT, FF.PLANT_D, ref))
    inside, far = FF.planted_cells()
    for f, sign in ((0, 1), (1, -1)):      # what tests/test_frame_flow_cpu.py asserts of the restatement
        assert (got[0][f, 0][inside[f]] == sign * np.array(FF.PLANT_MOVE)).all() and not got[1][f, 0][inside[f]][:, 0].any()
        assert not got[0][f, 0][far[f]].any()


def test_strided_loops_at_full_size(eng):
    """One pair at 480 x 720, D = 8: six strips of cells a row, 360 work groups a slot, more pixels than one pass of the luma grid's threads."""
    rng = np.random.default_rng(8)
    raw = rng.integers(0, 256, size=(480 + 30, 720 + 30, 3)).astype(np.int64)
    canvas = (sum(raw[j:j + 504, i:i + 744] for j in range(7) for i in range(7)) // 49).astype(np.uint8)
    x = np.stack([canvas[3:483, 14:734], canvas[8:488, 8:728]])      # frame 1 shows the canvas (5, -6) further
    x[1, 200:300, 300:400] = canvas[0:100, 0:100]                    # and something else in the middle
    ref = np.array([[1], [-1]], np.int32)
    got = _run(eng, x, (0, 0, 480, 720), 8, ref)
    _equal(got, FF.frame_flow(x, (0, 0, 480, 720), 8, ref))
    assert tuple(got[0][0, 0, 5, 5]) == (-5, 6) and got[1][0, 0, 5, 5, 0] == 0


def test_more_work_groups_than_the_grid(eng):
    """1700 frames x 8 slots x 5 rows of cells = 68000 work items for a grid of at most 65536 groups: the items past it are reached by the strided
    loop.  Nearly every slot is absent (it is zeroed, which a sentinel shows); the frames that have one are at the clip's end."""
    T, H, W, rect, D = 1700, 40, 56, (3, 5, 30, 41), 2
    x = np.zeros((T, H, W, 3), np.uint8)
    x[-4:] = FF.smooth_clip(4, H, W, 21)
    ref = np.full((T, 8), -1, np.int32)
    ref[-1] = [T - 2, T - 3, -1, T - 4, T, T - 1, T - 2, -1]
    ref[-2, 7] = T - 1
    ref[5, 3] = 1699
    flow = torch.full((T, 8, 5, 7, 2), -7, dtype=torch.int32, device='cuda:0')
    sad = torch.full((T, 8, 5, 7, 2), -9, dtype=torch.int32, device='cuda:0')
    xd, rd = _dev(x), _dev(ref)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    assert eng._lib.jcm_frame_flow(eng._h, p(xd), T, H, W, *rect, D, p(rd), 8, p(flow), p(sad)) == 0
    torch.cuda.synchronize()
    want = FF.frame_flow(x, rect, D, ref)
    assert want[1][-1].any() and want[1][5, 3].any()
    _equal((flow.cpu().numpy(), sad.cpu().numpy()), want)


def test_flow_error_arguments_leave_the_outputs_untouched(eng):
    name = 'cut on every side'
    x, rect, D, ref = FF.flow_case(name)
    T, H, W, R = x.shape[0], x.shape[1], x.shape[2], ref.shape[1]
    xd, rd = _dev(x), _dev(ref)
    flow = torch.full((T, R, H // 8, W // 8, 2), -7, dtype=torch.int32, device='cuda:0')
    sad = torch.full((T, R, H // 8, W // 8, 2), -9, dtype=torch.int32, device='cuda:0')
    p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)
    good = (p(xd), T, H, W) + rect + (D, p(rd), R, p(flow), p(sad))
    cases = {'null x': {0: p(None)}, 'null ref': {9: p(None)}, 'null flow': {11: p(None)}, 'null sad': {12: p(None)}, 'T = 0': {1: 0}, 'T = 65535': {1: 65535},
             'D = 0': {8: 0}, 'D = 17': {8: 17}, 'R = 0': {10: 0}, 'R = 9': {10: 9}, 'H % 8': {2: 36}, 'W % 8': {3: 52}, 'H > 4096': {2: 4104}, 'W > 4096': {3: 4104},
             'y0 < 0': {4: -1}, 'x0 < 0': {5: -1}, 'rows past the frame': {4: 11}, 'columns past the frame': {5: 16}, 'ch = 0': {6: 0}, 'cw = 0': {7: 0}}
    for case, change in cases.items():
        args = list(good)
        for i, v in change.items():
            args[i] = v
        assert eng._lib.jcm_frame_flow(eng._h, *args) == 1, case      # JCM_ERR_ARG
    torch.cuda.synchronize()
    assert (flow == -7).all() and (sad == -9).all()
    assert eng._lib.jcm_frame_flow(eng._h, *good) == 0
    torch.cuda.synchronize()
    _equal((flow.cpu().numpy(), sad.cpu().numpy()), FF.flow_case_expected(name))
    with pytest.raises(ValueError, match='ref must be'):
        eng.frame_flow(xd, rect, ref[:2], search=D)


# ------------------------------------------------------------------ the pooling
def _pool(eng, hm, flow, w):
    out = eng.hm_flow_pool(_dev(hm), _dev(flow), w)
    torch.cuda.synchronize()
    assert out.dtype == torch.float32
    return out.cpu().numpy()


def _same_bits(got, want):
    assert_array_equal(got.view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize('K,N,T', FF.POOL_CASES)
def test_pool_small(eng, K, N, T):
    """5 x 7 maps whose values span the fp32 exponent range; flows of up to five cells either way -- past all four edges, every eighth in both axes."""
    hm, flow = FF.pool_maps(T, 5, 7, K, 100 + K), FF.pool_flow(T, N, 5, 7, 200 + T)
    assert (flow % 8 != 0).all(axis=-1).any() and flow.min() <= -40 + 8 and flow.max() >= 40 - 8
    _same_bits(_pool(eng, hm, flow, FF.POOL_WEIGHTS[N]), FF.hm_flow_pool(hm, flow, FF.POOL_WEIGHTS[N]))


def test_pool_order_of_the_sum(eng):
    """FF.order_case: a sum taken with t + n before t - n gives 0 where the header's order gives 1/3."""
    hm, flow, w = FF.order_case()
    got = _pool(eng, hm, flow, w)
    _same_bits(got, FF.hm_flow_pool(hm, flow, w))
    assert (got[1] == np.float32(1.0 / 3.0)).all()


def test_pool_clip_at_full_size(eng):
    hm, flow = FF.pool_maps(5, 60, 90, 9, 7), FF.pool_flow(5, 2, 60, 90, 8, reach=16)
    w = (1.0, 0.6, 0.3)
    _same_bits(_pool(eng, hm, flow, w), FF.hm_flow_pool(hm, flow, w))
    _same_bits(_pool(eng, hm, flow, (0.5, 0.0, 0.0)), hm)      # w = [w0, 0, ..]: hm's bits


def test_pool_error_arguments_leave_the_output_untouched(eng):
    T, HH, WW, K, N = 3, 5, 7, 2, 2
    hm, flow = _dev(FF.pool_maps(T, HH, WW, K, 1)), _dev(FF.pool_flow(T, N, HH, WW, 2))
    out = torch.full((T, HH, WW, K), -7.0, device='cuda:0')
    big = torch.zeros(1, 91, 91, 1, device='cuda:0')
    p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)
    wp = lambda *w: (ctypes.c_double * len(w))(*w)
    good = [p(hm), T, HH, WW, K, p(flow), N, wp(1.0, 0.5, 0.25), p(out)]
    cases = {'w[0] = 0': {7: wp(0.0, 1.0, 1.0)}, 'a negative weight': {7: wp(1.0, -0.5, 1.0)}, 'a NaN weight': {7: wp(1.0, 1.0, float('nan'))},
             'an infinite weight': {7: wp(float('inf'), 1.0, 1.0)}, 'N = 0': {6: 0}, 'N = 5': {6: 5, 7: wp(1.0, 1.0, 1.0, 1.0, 1.0, 1.0)}, 'out is hm': {8: p(hm)},
             'out overlaps hm': {8: ctypes.c_void_p(hm.data_ptr() + 4 * (T * HH * WW * K - 1))}, 'null hm': {0: p(None)}, 'null flow': {5: p(None)},
             'null w': {7: None}, 'null out': {8: p(None)}, 'T = 0': {1: 0}, 'K = 17': {4: 17}, 'HH * WW > 8192': {0: p(big), 1: 1, 2: 91, 3: 91, 4: 1}}
    keep = hm.clone()
    for case, change in cases.items():
        args = list(good)
        for i, v in change.items():
            args[i] = v
        assert eng._lib.jcm_hm_flow_pool(eng._h, *args) == 1, case      # JCM_ERR_ARG
    torch.cuda.synchronize()
    assert (out == -7.0).all() and torch.equal(hm, keep)
    assert eng._lib.jcm_hm_flow_pool(eng._h, *good) == 0
    torch.cuda.synchronize()
    _same_bits(out.cpu().numpy(), FF.hm_flow_pool(hm.cpu().numpy(), flow.cpu().numpy(), (1.0, 0.5, 0.25)))
    with pytest.raises(ValueError, match='flow must be'):
        eng.hm_flow_pool(hm, flow, (1.0, 1.0))
