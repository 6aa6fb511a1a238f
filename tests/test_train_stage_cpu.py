"""The float64 restatements of tests/train_stage_ref.py (the yardstick of test_gpu_train_stages.py) on the CPU: against torch float64 autograd
on tie-free inputs, and on hand-pinned cases for what autograd does not define (ties, half windows, the clamp row, TF's backprop)."""
import numpy as np
import pytest
import torch

import train_stage_ref as R
from oracle import jcm_oracle as O
from oracle import jcm_oracle_torch as OT


def _nchw(a):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64).permute(0, 3, 1, 2)


def _nhwc(t):
    return t.permute(0, 2, 3, 1).detach().numpy()


@pytest.mark.parametrize('shape', [(2, 5, 7, 6), (1, 6, 8, 4), (3, 1, 9, 5), (1, 9, 1, 3)])
def test_bn_forward_backward_vs_autograd(shape):
    """BN(relu(z)) -> 2x2 SAME pool on tie-free inputs (continuous draws, no ReLU zeros inside a window's maximum... a zero never wins: beta-shifted
    ties are avoided by keeping z > 0): y, pool, dz, dgamma, dbeta, dbias of the restatement against torch float64 autograd, pooled and not."""
    rs = np.random.RandomState(sum(shape))
    B, H, W, C = shape
    z = rs.standard_normal(shape) + 0.3
    gamma, beta = rs.uniform(0.5, 1.5, C), 0.1 * rs.standard_normal(C)
    for pooled in (False, True):
        if pooled:
            z = np.abs(z) + 0.01      # no ReLU zeros: no two equal values in a window
        zt = _nchw(z).clone().requires_grad_(True)
        bias = torch.zeros(C, dtype=torch.float64, requires_grad=True)
        g, b = (torch.tensor(v, requires_grad=True) for v in (gamma, beta))
        rt = torch.relu(zt + bias[None, :, None, None])
        mean = rt.mean(dim=(0, 2, 3), keepdim=True)
        var = ((rt - mean) ** 2).mean(dim=(0, 2, 3), keepdim=True)
        yt = (rt - mean) / torch.sqrt(var + R.BN_EPS) * g[None, :, None, None] + b[None, :, None, None]
        out = OT.max_pool_same(yt) if pooled else yt
        dout = rs.standard_normal(tuple(out.shape))
        (out * torch.as_tensor(dout)).sum().backward()
        r = np.maximum(z, 0)
        st = R.bn_stats(r, np.zeros(C), np.ones(C))
        y = R.bn_apply(r, st['mean'], st['rstd'], gamma, beta)
        assert np.abs(y - _nhwc(yt)).max() <= 1e-12
        dp = np.ascontiguousarray(np.transpose(dout, (0, 2, 3, 1)))
        if pooled:
            assert np.array_equal(R.max_pool(y), O.max_pool_same(y)) and np.abs(R.max_pool(y) - _nhwc(out)).max() <= 1e-12
        dy = R.max_pool_bwd(y, dp) if pooled else dp
        got = R.bn_bwd(dy, r, st['mean'], st['rstd'], gamma)
        assert np.abs(got['dz'] - _nhwc(zt.grad)).max() <= 1e-11
        for k, t in (('dgamma', g), ('dbeta', b), ('dbias', bias)):
            assert np.abs(got[k] - t.grad.numpy()).max() <= 1e-11, k


def test_bn_stats_moving_update_and_single_sample():
    """Biased variance for rstd, Bessel-corrected variance into the moving average, decay 0.9; N = 1: variance 0 and no Bessel factor."""
    r = np.array([1.0, 2.0, 6.0]).reshape(3, 1, 1, 1)
    st = R.bn_stats(r, np.array([10.0]), np.array([2.0]))
    assert st['mean'][0] == 3.0 and abs(st['var'][0] - 14.0 / 3.0) < 1e-15
    assert abs(st['rstd'][0] - 1.0 / np.sqrt(14.0 / 3.0 + 1e-3)) < 1e-15
    assert abs(st['mov_mean'][0] - (9.0 + 0.3)) < 1e-14 and abs(st['mov_var'][0] - (1.8 + 0.1 * 7.0)) < 1e-14
    st = R.bn_stats(np.full((1, 1, 1, 2), 5.0), np.zeros(2), np.ones(2))
    assert (st['var'] == 0).all() and np.allclose(st['mov_var'], 0.9, atol=1e-15) and np.allclose(st['rstd'], 1e-3 ** -0.5)


def test_pool_tie_window_goes_to_the_first_maximum():
    """A 2x2 window of four equal values, and one whose maximum stands twice: the gradient goes to the first in row-major order only."""
    y = np.array([[7.0, 7.0, 1.0, 5.0], [7.0, 7.0, 5.0, 2.0]]).reshape(1, 2, 4, 1)
    dp = np.array([3.0, 11.0]).reshape(1, 1, 2, 1)
    assert R.max_pool_argmax(y).reshape(-1).tolist() == [0, 1]
    assert R.max_pool_bwd(y, dp).reshape(2, 4).tolist() == [[3.0, 0.0, 0.0, 11.0], [0.0, 0.0, 0.0, 0.0]]


def test_pool_3x3_half_windows():
    """3x3 -> 2x2: the windows of the last row / column are halves, the corner a single element; -inf padding never wins, negative maxima included."""
    y = -np.arange(1.0, 10.0).reshape(1, 3, 3, 1)
    assert R.max_pool(y).reshape(2, 2).tolist() == [[-1.0, -3.0], [-7.0, -9.0]]
    dp = np.array([[1.0, 2.0], [3.0, 4.0]]).reshape(1, 2, 2, 1)
    assert R.max_pool_bwd(y, dp).reshape(3, 3).tolist() == [[1.0, 0.0, 2.0], [0.0, 0.0, 0.0], [3.0, 0.0, 4.0]]
    y2 = np.arange(1.0, 10.0).reshape(1, 3, 3, 1)
    assert R.max_pool_bwd(y2, dp).reshape(3, 3).tolist() == [[0.0, 0.0, 0.0], [0.0, 1.0, 2.0], [0.0, 3.0, 4.0]]


def test_resize_adjoint_clamp_row():
    """2 -> 4 rows: outputs 0..3 read (row 0), (rows 0, 1 at 1/2), (row 1), (row 1 and the CLAMPED row 1 at 1/2): the last output's two taps land on
    the same source row, which takes its whole gradient."""
    dy = np.array([1.0, 10.0, 100.0, 1000.0]).reshape(1, 4, 1, 1)
    assert R.resize_bwd(dy, 2, 1).reshape(-1).tolist() == [1.0 + 5.0, 5.0 + 100.0 + 1000.0]
    assert R.resize_bwd(dy, 2, 1, scale=0.5).reshape(-1).tolist() == [3.0, 552.5]


@pytest.mark.parametrize('geom', [(30, 45, 60, 90), (13, 19, 25, 37), (7, 10, 25, 37), (8, 12, 31, 46), (5, 5, 5, 5), (1, 1, 3, 4)])
def test_resize_adjoint_is_the_transpose_of_the_oracle_operator(geom):
    h, w, H, W = geom
    rs = np.random.RandomState(h * 100 + W)
    x, dy = rs.standard_normal((2, h, w, 3)), rs.standard_normal((2, H, W, 3))
    xt = _nchw(x).clone().requires_grad_(True)
    out = OT.resize_bilinear_tf1(xt, H, W)
    assert np.abs(_nhwc(out) - O.resize_bilinear_tf1(x, H, W)).max() <= 1e-12
    (out * _nchw(dy)).sum().backward()
    assert np.abs(R.resize_bwd(dy, h, w, scale=1.0 / 3.0) - _nhwc(xt.grad) / 3.0).max() <= 1e-12


@pytest.mark.parametrize('tsum', [1.0, 0.4, 0.0])
def test_softmax_ce_loss_is_the_definition_and_backprop_is_tfs(tsum):
    """The loss is -sum t log softmax(z) (autograd's value); the backprop is gscale * (softmax - t): autograd's gradient gscale * (softmax sum(t) - t)
    only where the target map sums to one -- pinned for a map summing to 0.4 and to 0."""
    rs = np.random.RandomState(3)
    B, HW, K = 2, 37, 3
    z = rs.standard_normal((B, HW, K)) * 5
    t = rs.uniform(0, 1, (B, HW, K + 1))
    t[:, :, :K] *= tsum / t[:, :, :K].sum(axis=1, keepdims=True)
    zt = torch.tensor(z, requires_grad=True)
    lt = -(torch.as_tensor(t[:, :, :K]) * torch.log_softmax(zt, dim=1)).sum(dim=1)
    (0.25 * lt.sum()).backward()
    loss, dz = R.softmax_ce(z, t, gscale=0.25)
    assert np.abs(loss - lt.detach().numpy()).max() <= 1e-12
    p = torch.softmax(torch.as_tensor(z), dim=1).numpy()
    assert np.abs(dz - 0.25 * (p - t[:, :, :K])).max() <= 1e-15
    exact = np.abs(dz - zt.grad.numpy()).max()
    assert exact <= 1e-14 if tsum == 1.0 else exact >= 1e-3


def test_softmax_bwd_vs_autograd():
    rs = np.random.RandomState(4)
    z, g = rs.standard_normal((2, 41, 3)) * 3, rs.standard_normal((2, 41, 5))
    zt = torch.tensor(z, requires_grad=True)
    (torch.softmax(zt, dim=1) * torch.as_tensor(g[:, :, :3])).sum().backward()
    assert np.abs(R.softmax_bwd(torch.softmax(zt, dim=1).detach().numpy(), g) - zt.grad.numpy()).max() <= 1e-14


def test_float32_mode_is_float32_and_close():
    """The float32 mode returns float32 tensors a rounding-level distance away (the yardstick is neither 0 nor large), and the inputs of the GPU
    tests meet the ReLU cap by themselves: post-ReLU draws hold exact zeros and (next to) no near-zeros."""
    rs = np.random.RandomState(5)
    r = R.post_relu(rs, (2, 33, 47, 12))
    assert (r == 0).mean() > 0.3 and R.near_zero(r).mean() <= 1e-3
    dy = rs.standard_normal(r.shape).astype(np.float32)
    gamma = rs.uniform(0.5, 1.5, 12).astype(np.float32)
    s64, s32 = (R.bn_stats(r, np.zeros(12), np.ones(12), dtype=d) for d in (np.float64, np.float32))
    b64, b32 = (R.bn_bwd(dy, r, s64['mean'].astype(np.float32), s64['rstd'].astype(np.float32), gamma, dtype=d) for d in (np.float64, np.float32))
    for a, b in [(s64[k], s32[k]) for k in s64] + [(b64[k], b32[k]) for k in b64]:
        assert b.dtype == np.float32 and a.dtype == np.float64
        assert 0 < np.abs(a - b).max() <= 1e-5 * np.abs(a).max()
    assert R.bound(b32['dz'], b64['dz']) <= 1e-5 * np.abs(b64['dz']).max()
