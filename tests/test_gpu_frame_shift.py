"""jcm_frame_shift on the GPU (csrc/frame_shift.hip) against its numpy restatement (tests/frame_shift_ref.py, pinned by
tests/test_frame_shift_cpu.py).  Everything is integer arithmetic and every sum is order-free: disp and sad are compared bit for bit.  The shapes
are the smallest at which each path of the kernels runs: the smallest legal rectangle, rows no load width divides, rows that take the dword
loads with ragged ends, a byte-misaligned base, and one full-size pair whose strided loops run past their first trip."""
import ctypes
import functools

import numpy as np
import pytest
import torch
from numpy.testing import assert_array_equal

import frame_shift_ref as FR
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


def _run(eng, x, rect, D, prev=None):
    r = eng.frame_shift(_dev(x), rect, search=D, prev=None if prev is None else _dev(prev))
    torch.cuda.synchronize()
    assert r['disp'].dtype == torch.int32 and r['sad'].dtype == torch.int64
    return r['disp'].cpu().numpy(), r['sad'].cpu().numpy()


def _equal(got, want):
    assert_array_equal(got[0], want[0])
    assert_array_equal(got[1], want[1])


@functools.lru_cache(maxsize=None)
def _mixed(T, H, W, D, seed):
    """Frames that pan, then frames that match nowhere (the tie-break tuple and the coarse winner decide): uint8 [T,H,W,3], never written to."""
    rng = np.random.default_rng(seed)
    m = 4 * D + 3
    canvas = FR.pan_canvas(rng, H + 4 * m, W + 4 * m, box=5)
    pans = [(0, 0)] + [tuple(int(v) for v in rng.integers(-m // 2, m // 2 + 1, size=2)) for _ in range(T - 2)]
    x = np.concatenate([FR.pan_frames(canvas, H, W, (2 * m, 2 * m), pans), rng.integers(0, 256, size=(1, H, W, 3)).astype(np.uint8)])
    x.setflags(write=False)
    return x


def test_smallest_legal_rectangle(eng):
    """D = 1, 24 x 40, rectangle (3, 5, 15, 29): the coarse interior is one row of cells, origin and size are no multiples of 4, and with W % 4 == 0
    the rows take the dword loads with a ragged group at either end."""
    x = _mixed(4, 24, 40, 1, 1)
    _equal(_run(eng, x, (3, 5, 15, 29), 1), FR.frame_shift(x, (3, 5, 15, 29), 1))


def test_bars_have_no_say(eng):
    rect = (3, 5, 15, 29)
    x = _mixed(4, 24, 40, 1, 2)
    want = FR.frame_shift(x, rect, 1)
    rng = np.random.default_rng(3)
    for _ in range(2):
        y = rng.integers(0, 256, size=x.shape).astype(np.uint8)      # other bars in every frame, the same content
        y[:, 3:18, 5:34] = x[:, 3:18, 5:34]
        _equal(_run(eng, y, rect, 1), want)


@pytest.mark.parametrize('W,rect,offset', [(37, (2, 3, 30, 33), 0), (64, (1, 6, 33, 53), 0), (64, (0, 0, 35, 64), 0), (64, (1, 6, 33, 53), 1)])
def test_load_widths(eng, W, rect, offset):
    """W = 37: rows no vector width divides (byte loads).  W = 64: dword loads, with ragged and with whole groups at the ends; and the same frames
    at a base one byte off a dword, which must fall back to bytes."""
    x = _mixed(3, 35, W, 2, W)
    want = FR.frame_shift(x, rect, 2, prev=x[2])
    buf = torch.zeros(x.size + 3 * 35 * W + 8, dtype=torch.uint8, device='cuda:0')
    xd = buf[offset:offset + x.size].view(x.shape)
    pd = buf[offset + x.size:offset + x.size + 3 * 35 * W].view(35, W, 3)
    xd.copy_(torch.as_tensor(x.copy()))
    pd.copy_(xd[2])
    assert xd.data_ptr() % 4 == offset
    r = eng.frame_shift(xd, rect, search=2, prev=pd)
    torch.cuda.synchronize()
    _equal((r['disp'].cpu().numpy(), r['sad'].cpu().numpy()), want)


def test_strided_loops_at_full_size(eng):
    """One pair at 480 x 720, D = 8: more rows than a group's chunk, more columns than a wave, more cells than threads."""
    D = 8
    canvas = FR.pan_canvas(np.random.default_rng(8), 480 + 20, 720 + 30, box=9)
    x = FR.pan_frames(canvas, 480, 720, (3, 30), [(0, 0), (17, -29)])
    got = _run(eng, x, (0, 0, 480, 720), D)
    _equal(got, FR.frame_shift(x, (0, 0, 480, 720), D))
    assert tuple(got[0][1]) == (17, -29) and got[1][1, 0] == 0


@pytest.mark.parametrize('D,H,W,rect', [(1, 48, 60, (3, 5, 41, 50)), (2, 64, 80, (0, 0, 64, 80)), (4, 96, 128, (6, 9, 85, 111))])
def test_known_pans(eng, D, H, W, rect):
    x, pans = FR.pan_clip(D, H, W)
    got = _run(eng, x, rect, D)
    _equal(got, FR.frame_shift(x, rect, D))
    assert_array_equal(got[0][1:], np.array(pans))      # what tests/test_frame_shift_cpu.py asserts of the restatement


def test_ties(eng):
    rect = (3, 5, 15, 29)
    flat = np.full((3, 24, 40, 3), 77, np.uint8)
    flat[:, :3] = 200                                         # bars of another value
    disp, sad = _run(eng, flat, rect, 1)
    assert not disp.any() and not sad.any()
    x = _mixed(4, 24, 40, 1, 5)
    twice = np.stack([x[3], x[3]])
    disp, sad = _run(eng, twice, rect, 1, prev=x[3])
    assert not disp.any() and not sad.any()


def test_split_and_no_prev(eng):
    rect = (1, 2, 30, 37)
    x = _mixed(5, 32, 40, 1, 6)
    whole = _run(eng, x, rect, 1)
    _equal(whole, FR.frame_shift(x, rect, 1))
    assert not whole[0][0].any() and not whole[1][0].any()      # prev == NULL: row 0 is zero
    a, b = _run(eng, x[:2], rect, 1), _run(eng, x[2:], rect, 1, prev=x[1])
    _equal((np.concatenate([a[0], b[0]]), np.concatenate([a[1], b[1]])), whole)
    one = _run(eng, x[:1], rect, 1)                              # T == 1 without prev: no pair at all
    assert not one[0].any() and not one[1].any()


def test_error_arguments_leave_the_outputs_untouched(eng):
    H, W, rect, T = 24, 40, (3, 5, 15, 29), 2
    x = _dev(_mixed(4, H, W, 1, 7)[:T])
    disp = torch.full((T, 2), -7, dtype=torch.int32, device='cuda:0')
    sad = torch.full((T, 2), -9, dtype=torch.int64, device='cuda:0')
    big = torch.zeros(1, 2100, 2100, 3, dtype=torch.uint8, device='cuda:0')
    tall = torch.zeros(1, 4097, 40, 3, dtype=torch.uint8, device='cuda:0')
    p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)
    good = (p(x), T, H, W) + rect + (1, p(None), p(disp), p(sad))
    cases = {'null x': {0: p(None)}, 'null disp': {10: p(None)}, 'null sad': {11: p(None)}, 'T = 0': {1: 0}, 'D = 0': {8: 0}, 'D = 17': {8: 17},
             'y0 < 0': {4: -1}, 'x0 < 0': {5: -1}, 'rows past the frame': {4: 10}, 'columns past the frame': {5: 12}, 'ch below 8D + 7': {6: 14},
             'cw below 8D + 7': {7: 14}, 'ch below 8D + 7 at D = 2': {8: 2, 6: 22}, 'H * W * 1020 >= 2^32': {0: p(big), 1: 1, 2: 2100, 3: 2100},
             'H > 4096': {0: p(tall), 1: 1, 2: 4097}}
    for name, change in cases.items():
        args = list(good)
        for i, v in change.items():
            args[i] = v
        assert eng._lib.jcm_frame_shift(eng._h, *args) == 1, name      # JCM_ERR_ARG
    torch.cuda.synchronize()
    assert (disp == -7).all() and (sad == -9).all()
    assert eng._lib.jcm_frame_shift(eng._h, *good) == 0
    torch.cuda.synchronize()
    want = FR.frame_shift(x.cpu().numpy(), rect, 1)
    _equal((disp.cpu().numpy(), sad.cpu().numpy()), want)
