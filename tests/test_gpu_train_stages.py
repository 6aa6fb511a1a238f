"""The training step's kernels BETWEEN its convolutions (csrc/train_kernels.hip), each held to the float64 restatement of tests/train_stage_ref.py
through its stand-alone entry point (jcm_train_bn_fwd / _bn_bwd / _resize_bwd / _softmax_ce / _softmax_bwd: the host function the step calls, on
caller tensors), at the channel counts, map sizes and inputs that select every kernel variant -- whole steps only ever see C in {16 .. 512} powers of
two, even maps of many pixels, and compare at 1e-4 of max|g|.

fp32 bound, per tensor: |got - ref64| <= 4 max|ref32 - ref64| + 2^-22 max|ref64| (train_stage_ref.bound: the yardstick is the float32 mode of the
restatement, never the kernel).  Every call writes into NaN-filled tensors with NaN guards around them: every element is written, nothing outside
is, and a second identical call is bit-identical.  The achieved errors are printed per case (pytest -s)."""
import ctypes

import numpy as np
import pytest
import torch

import joint_cnn_mrf_amd  # noqa: F401
import train_stage_ref as R
from joint_cnn_mrf_amd import _lib
from oracle import jcm_oracle as O
from test_gpu_random_shapes import check_bf16_layer, layer_params

pytestmark = pytest.mark.gpu

# BatchNorm channel counts: which kernel variant each one selects
BN_C = [(4, 'one channel group: float4 kernels with C4 = 1, 256 lanes of one group in the fused column sums'),
        (6, 'C % 4 != 0: the scalar kernels (bn_apply_kernel, bn_bwd_apply_kernel, col_sum); a pool request is refused'),
        (12, '256 % (C / 4) != 0: bn_bwd_apply4<false> + col_sum (two calls) and max_pool_bwd + the plain kernels behind a pooled gradient'),
        (16, "the model's narrowest layer: every fused form (bn_apply_pool4, bn_bwd_apply4<true>, bn_bwd_pooled)"),
        (96, 'C4 = 24: the two-call / max_pool_bwd fallbacks at a width real layers have; col_reduce with 2 row lanes and idle threads (256 / 96)'),
        (128, 'C4 = 32: fused forms, 8 threads per channel group'),
        (260, 'C > 256: the c0 loop of col_reduce_kernel with a tail of cw = 4; C4 = 65: fallbacks'),
        (512, 'C > 256 with two full passes; C4 = 128: fused forms, 2 threads per channel group')]
# map shapes (B, H, W)
BN_SHAPES = [((1, 1, 1), 'N = 1: no Bessel factor, variance 0; the 4-row unroll of col_reduce has only its tail'),
             ((3, 1, 9), 'H == 1: every window a half window in y'),
             ((1, 9, 1), 'W == 1: every window a half window in x'),
             ((2, 5, 7), 'odd extents: half windows in the last row and column, a single-element corner window'),
             ((1, 6, 8), 'even extents: full windows only'),
             ((2, 33, 47), 'N = 3102: several reduction blocks (C <= 16), odd extents')]
BN_CASES = [pytest.param(c, s, id='C%d_%dx%dx%d' % ((c,) + s)) for c, _ in BN_C for s, _ in BN_SHAPES]
NAN32 = int(np.array(np.nan, np.float32).view(np.int32))


class Handles:
    """One small one-layer handle ('c': 5x5, Cin 16 -- bf16: 32 --, Cout = C, with BatchNorm) per channel count and precision, kept for the module."""

    def __init__(self):
        self.h = {}

    def get(self, C, precision='fp32'):
        from joint_cnn_mrf_amd.engine import Engine
        from joint_cnn_mrf_amd.train import Trainer
        key = (C, precision)
        if key not in self.h:
            p = layer_params(np.random.RandomState(1000 + C), 32 if precision == 'bf16' else 16, C, 5)
            eng = Engine(device=0, precision=precision).load_params(p)
            self.h[key] = (Trainer(eng, use_sm=False), p)
        return self.h[key]

    def close(self):
        for tr, _ in self.h.values():
            tr.eng.close()


@pytest.fixture(scope='module')
def handles():
    hs = Handles()
    yield hs
    hs.close()


class Guarded:
    """A NaN-filled device tensor inside a larger NaN-filled allocation (64 elements in front and behind)."""
    PAD = 64

    def __init__(self, shape, dtype=torch.float32, seed=None):
        n = int(np.prod(shape))
        self.full = torch.full((n + 2 * self.PAD,), float('nan'), dtype=dtype, device='cuda:0')
        self.t = self.full[self.PAD:self.PAD + n].view(*shape)
        if seed is not None:
            self.t.copy_(torch.as_tensor(seed, device='cuda:0').to(dtype))

    def check(self, what, written=True):
        f = self.full.float().cpu()
        assert torch.isnan(f[:self.PAD]).all() and torch.isnan(f[-self.PAD:]).all(), '%s: written outside the tensor' % what
        if written:
            assert not torch.isnan(self.t).any(), '%s: %d entries left unwritten' % (what, int(torch.isnan(self.t).sum()))
        return self.t.float().cpu().numpy()


def _dev(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a), device='cuda:0').to(dtype)


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.int32 if a.dtype == np.float32 else np.int64), b.view(np.int32 if b.dtype == np.float32 else np.int64))


def _report(tag, pairs):
    """pairs: (name, got, ref32, ref64).  Prints err and bound per tensor, asserts the bound.  -> {name: err / max|ref64|}."""
    bad, out = [], {}
    for name, got, r32, r64 in pairs:
        r64 = np.asarray(r64, np.float64)
        err, bnd = float(np.abs(np.asarray(got, np.float64).reshape(r64.shape) - r64).max()), R.bound(r32, r64)
        out[name] = err / max(float(np.abs(r64).max()), 1e-300)
        print('  %-22s %-8s err %.3e  bound %.3e  (err / max|ref| %.2e)' % (tag, name, err, bnd, out[name]))
        if not err <= bnd:
            bad.append((name, err, bnd))
    assert not bad, '%s: outside 4 max|ref32 - ref64| + 2^-22 max|ref64|: %s' % (tag, bad)
    return out


def _set_moving(tr, p):
    tr.eng.update_tensor('c/BatchNorm/moving_mean', p['c/BatchNorm/moving_mean'], refresh=False)
    tr.eng.update_tensor('c/BatchNorm/moving_variance', p['c/BatchNorm/moving_variance'], refresh=False)


def bn_fwd_checked(tr, p, rd, pool):
    """jcm_train_bn_fwd twice from the same moving statistics into guarded NaN tensors: everything written, nothing outside, bit-identical.
    -> y, pool (or None), mean, rstd, moving_mean, moving_variance (numpy float32; y / pool hold the bf16 values on a bf16 handle)."""
    e = tr.eng
    B, H, W, C = rd.shape
    res = []
    for _ in range(2):
        _set_moving(tr, p)
        y, mean, rstd = Guarded(rd.shape, rd.dtype), Guarded((C,)), Guarded((C,))
        po = Guarded((B, (H + 1) // 2, (W + 1) // 2, C), rd.dtype) if pool else None
        _lib.check(tr._lib.jcm_train_bn_fwd(e._h, b'c', e._p(rd), B, H, W, e._p(y.t), e._p(po.t if pool else None), e._p(mean.t), e._p(rstd.t)), 'jcm_train_bn_fwd')
        torch.cuda.synchronize()
        res.append([y.check('y'), po.check('pool') if pool else None, mean.check('mean'), rstd.check('rstd'),
                    tr.get_tensor('c/BatchNorm/moving_mean', (C,)), tr.get_tensor('c/BatchNorm/moving_variance', (C,))])
    for a, b in zip(*res):
        assert (a is None and b is None) or _same_bits(a, b), 'a second identical forward call is not bit-identical'
    return res[0]


def bn_bwd_checked(tr, dyd, rd, yd, mean, rstd, dy_scale, pooled):
    """jcm_train_bn_bwd twice into a guarded NaN dz and a NaN gradient buffer: dz and exactly the gamma / beta / biases slices are written.
    -> dz, dgamma, dbeta, dbias (numpy float32)."""
    e = tr.eng
    B, H, W, C = rd.shape
    sl = {n.split('/')[-1]: (o, c) for n, o, c in tr.layout}
    res = []
    for _ in range(2):
        dz = Guarded(rd.shape, rd.dtype)
        grads = torch.full((tr.n_elements,), float('nan'), dtype=torch.float32, device='cuda:0')
        _lib.check(tr._lib.jcm_train_bn_bwd(e._h, b'c', e._p(dyd), ctypes.c_float(dy_scale), int(pooled), e._p(rd), e._p(yd), e._p(mean), e._p(rstd), B, H, W,
                                            e._p(grads), e._p(dz.t)), 'jcm_train_bn_bwd')
        torch.cuda.synchronize()
        g = grads.cpu().numpy()
        keep = np.ones(g.size, bool)
        out = [dz.check('dz')]
        for n in ('gamma', 'beta', 'biases'):
            o, c = sl[n]
            keep[o:o + c] = False
            assert np.isfinite(g[o:o + c]).all(), 'd%s has unwritten or non-finite entries' % n
            out.append(g[o:o + c].copy())
        assert (g[keep].view(np.int32) == NAN32).all(), 'gradient elements outside gamma / beta / biases were written'
        res.append(out)
    for a, b in zip(*res):
        assert _same_bits(a, b), 'a second identical backward call is not bit-identical'
    return res[0]


def _fwd_refs(r, p):
    """float64 / float32 restatement of the forward stage on the values r.  -> {dtype: (stats, y)}"""
    out = {}
    for d in (np.float64, np.float32):
        st = R.bn_stats(r, p['c/BatchNorm/moving_mean'], p['c/BatchNorm/moving_variance'], dtype=d)
        out[d] = (st, R.bn_apply(r, st['mean'], st['rstd'], p['c/BatchNorm/gamma'], p['c/BatchNorm/beta'], dtype=d))
    return out


def _bwd_refs(dy, r, mean, rstd, gamma, dy_scale):
    return {d: R.bn_bwd(dy, r, mean, rstd, gamma, dy_scale=dy_scale, dtype=d) for d in (np.float64, np.float32)}


def _check_dz(tag, got, refs, r):
    """dz and the parameter gradients against the restatement; dz outside the near-zero entries of r (<= 0.1 % of them); dz == 0 exactly where r <= 0."""
    dz = got[0]
    assert not dz[r <= 0].any(), '%s: dz != 0 where r <= 0' % tag
    nz = R.near_zero(r)
    assert nz.mean() <= 1e-3
    ok = ~nz
    return _report(tag, [('dz', dz[ok], refs[np.float32]['dz'][ok], refs[np.float64]['dz'][ok])] +
                   [(k, g, refs[np.float32][k], refs[np.float64][k]) for k, g in zip(('dgamma', 'dbeta', 'dbias'), got[1:])])


@pytest.mark.parametrize('C,shape', BN_CASES)
def test_bn_stage_fp32(handles, C, shape):
    """BatchNorm forward (statistics, moving averages, y, the fused or separate pool) and backward (plain with dy_scale = 1/3, pooled, and plain on the
    host-made pool gradient) of an fp32 handle against the float64 restatement; pool_out == max pool of the returned y bit for bit; the pooled and
    the unpooled backward meet the same bound with the same dz zero pattern; C % 4 != 0 refuses the pool with a message that says why."""
    tr, p = handles.get(C)
    B, H, W = shape
    rs = np.random.RandomState(C * 100 + H * 10 + W)
    r = R.post_relu(rs, (B, H, W, C))
    gamma = p['c/BatchNorm/gamma']
    rd = _dev(r)
    pool = C % 4 == 0
    tag = 'C%d %dx%dx%d' % (C, B, H, W)
    y, po, mean, rstd, mm, mv = bn_fwd_checked(tr, p, rd, pool)
    ref = _fwd_refs(r, p)
    (s64, y64), (s32, y32) = ref[np.float64], ref[np.float32]
    _report(tag + ' fwd', [('y', y, y32, y64), ('mean', mean, s32['mean'], s64['mean']), ('rstd', rstd, s32['rstd'], s64['rstd']),
                           ('mov_mean', mm, s32['mov_mean'], s64['mov_mean']), ('mov_var', mv, s32['mov_var'], s64['mov_var'])])
    if pool:
        assert _same_bits(po, R.max_pool(y)), 'pool_out is not the max pool of the returned y'
        y2 = bn_fwd_checked(tr, p, rd, False)[0]
        assert _same_bits(y, y2), 'y differs between the fused-pool and the plain apply kernel'
    else:
        with pytest.raises(RuntimeError, match=r'C % 4 == 0'):
            tr.bn_forward('c', rd, pool=True)
    # ---- backward, on the statistics of the float64 restatement rounded to fp32 (the stage alone: no forward error in its inputs)
    m32, r32 = s64['mean'].astype(np.float32), s64['rstd'].astype(np.float32)
    md, sd, yd = _dev(m32), _dev(r32), _dev(y)
    sc = float(np.float32(1.0 / 3.0))
    dy = (rs.standard_normal(r.shape) * 1e-3).astype(np.float32)
    _check_dz(tag + ' bwd', bn_bwd_checked(tr, _dev(dy), rd, None, md, sd, sc, False), _bwd_refs(dy, r, m32, r32, gamma, sc), r)
    dp = (rs.standard_normal(po.shape if pool else (B, (H + 1) // 2, (W + 1) // 2, C)) * 1e-3).astype(np.float32)
    if not pool:
        with pytest.raises(RuntimeError, match=r'C % 4 == 0'):
            tr.bn_backward('c', _dev(dp), rd, y=yd, mean=md, rstd=sd, pooled=True)
        return
    dyf = R.max_pool_bwd(y, dp)
    refs = _bwd_refs(dyf, r, m32, r32, gamma, 1.0)
    gp = bn_bwd_checked(tr, _dev(dp), rd, yd, md, sd, 1.0, True)
    gu = bn_bwd_checked(tr, _dev(dyf), rd, None, md, sd, 1.0, False)
    _check_dz(tag + ' pooled', gp, refs, r)
    _check_dz(tag + ' unpool', gu, refs, r)
    assert np.array_equal(gp[0] == 0, gu[0] == 0), 'the dz zero patterns of the pooled and the unpooled backward differ'


@pytest.mark.parametrize('C', [4, 12, 16, 96, 512])
@pytest.mark.parametrize('shape', [(2, 5, 7), (2, 33, 47)], ids=lambda s: '%dx%dx%d' % s)
def test_bn_pooled_backward_ties(handles, C, shape):
    """Ties: r on the grid {0, 1/2, 1} (ReLU zeros included), so every window of y holds equal values -- and dp, mean, rstd dyadic, so both column
    sums are EXACT in any order.  The pooled backward must then equal, bit for bit in dz, dgamma and dbeta, the plain backward on the pool gradient the
    host routed to the FIRST maximum of each window: the other slots carry the dy = 0 expression, a gradient at a later maximum shows as a changed bit.
    Both are also held to the float64 restatement."""
    tr, p = handles.get(C)
    B, H, W = shape
    rs = np.random.RandomState(7 * C + H)
    r = (rs.randint(0, 3, (B, H, W, C)) * 0.5).astype(np.float32)
    rd = _dev(r)
    y = bn_fwd_checked(tr, p, rd, True)[0]
    k = R.max_pool_argmax(y)
    tied = sum(((np.pad(y, ((0, 0), (0, H % 2), (0, W % 2), (0, 0)), constant_values=-np.inf)[:, dy::2, dx::2] == R.max_pool(y)).astype(int)) for dy in (0, 1) for dx in (0, 1))
    assert (tied > 1).mean() > 0.3 and len(np.unique(k)) >= min(4, (1 + (H > 1)) * (1 + (W > 1)))      # many windows with a repeated maximum, every slot a winner somewhere
    dp = (rs.randint(-31, 32, k.shape) * 2.0 ** -10).astype(np.float32)
    m32, r32 = np.full(C, 0.5, np.float32), (2.0 ** rs.randint(-1, 2, C)).astype(np.float32)
    md, sd = _dev(m32), _dev(r32)
    dyf = R.max_pool_bwd(y, dp)
    gp = bn_bwd_checked(tr, _dev(dp), rd, _dev(y), md, sd, 1.0, True)
    gu = bn_bwd_checked(tr, _dev(dyf), rd, None, md, sd, 1.0, False)
    for n, a, b in zip(('dz', 'dgamma', 'dbeta'), gp, gu):
        assert _same_bits(a, b), '%s: the pooled backward differs from the plain one on the first-maximum gradient (%d entries)' % (n, int((a != b).sum()))
    refs = _bwd_refs(dyf, r, m32, r32, p['c/BatchNorm/gamma'], 1.0)
    _check_dz('C%d %dx%dx%d ties' % ((C,) + shape), gp, refs, r)


@pytest.mark.parametrize('C,shape', [(12, (1, 1024, 1400)), (96, (1, 344, 512))], ids=['C12', 'C96'])
def test_bn_carried_channel_index(handles, C, shape):
    """N C / 4 just above 16384 x 256 float4s with C / 4 = 3 and 24: bn_apply4_kernel and bn_bwd_apply4_kernel<false> take a second grid stride with
    cstep = stride % C4 != 0 (1 and 16), the carried channel group wraps.  The tensor is a 4096-row block repeated (350 and 43 times), so its
    statistics, y and dz are those of the block: the float64 restatement runs on the block, the column sums scale with the repeat count."""
    tr, p = handles.get(C)
    B, H, W = shape
    N, NB = B * H * W, 4096
    reps = N // NB
    assert N % NB == 0 and N * C // 4 > 16384 * 256 and (16384 * 256) % (C // 4) != 0
    rs = np.random.RandomState(C)
    rb = R.post_relu(rs, (1, 1, NB, C))
    dyb = (rs.standard_normal(rb.shape) * 1e-3).astype(np.float32)
    rd, dyd = _dev(np.tile(rb.reshape(NB, C), (reps, 1)).reshape(B, H, W, C)), _dev(np.tile(dyb.reshape(NB, C), (reps, 1)).reshape(B, H, W, C))
    e = tr.eng
    y, mean, rstd = Guarded(rd.shape), Guarded((C,)), Guarded((C,))
    _lib.check(tr._lib.jcm_train_bn_fwd(e._h, b'c', e._p(rd), B, H, W, e._p(y.t), None, e._p(mean.t), e._p(rstd.t)), 'jcm_train_bn_fwd')
    ref = _fwd_refs(rb, p)
    (s64, y64), (s32, y32) = ref[np.float64], ref[np.float32]
    yg = y.check('y').reshape(reps, NB, C)
    assert (yg == yg[0]).all(), 'y is not periodic with the block: %d entries' % int((yg != yg[0]).sum())
    _report('C%d carried fwd' % C, [('y', yg[0], y32, y64), ('mean', mean.check('mean'), s32['mean'], s64['mean']), ('rstd', rstd.check('rstd'), s32['rstd'], s64['rstd'])])
    m32, r32 = s64['mean'].astype(np.float32), s64['rstd'].astype(np.float32)
    dz = Guarded(rd.shape)
    grads = torch.full((tr.n_elements,), float('nan'), dtype=torch.float32, device='cuda:0')
    md, sd = _dev(m32), _dev(r32)
    _lib.check(tr._lib.jcm_train_bn_bwd(e._h, b'c', e._p(dyd), ctypes.c_float(1.0), 0, e._p(rd), None, e._p(md), e._p(sd), B, H, W, e._p(grads), e._p(dz.t)), 'jcm_train_bn_bwd')
    zg = dz.check('dz').reshape(reps, NB, C)
    assert (zg == zg[0]).all(), 'dz is not periodic with the block: %d entries' % int((zg != zg[0]).sum())
    refs = _bwd_refs(dyb, rb, m32, r32, p['c/BatchNorm/gamma'], 1.0)
    g = {n.split('/')[-1]: grads[o:o + c].cpu().numpy() for n, o, c in tr.layout}
    scaled = {d: dict(refs[d], **{k: refs[d][k] * reps for k in ('dgamma', 'dbeta', 'dbias')}) for d in refs}
    _check_dz('C%d carried bwd' % C, [zg[0].reshape(rb.shape), g['gamma'], g['beta'], g['biases']], scaled, rb)


def test_bn_variance_conditioning(handles):
    """|mean| / std of 1, 1e2 and 1e3 (four channels each, std 1).  OpStats rounds each square to fp32 before it widens it (the reference's fp32
    graph forms the squares in fp32 too), so ss / N - m^2 carries up to 2^-24 x^2 per term: the variance is held to 2^-23 (mean^2 + var), the moving
    variance (started at 0: 0.1 x the Bessel-corrected variance) and rstd = 1 / sqrt(var + eps) to that bound propagated, or to the regular bound
    where that is larger (ratio 1); y to the regular bound plus the rstd allowance times max |r - mean| |gamma|.  The mean has no such term.
    Figures on these inputs: DESIGN.md 4.5a."""
    tr, p = handles.get(12)
    rs = np.random.RandomState(11)
    B, H, W, C = 2, 33, 47, 12
    N = B * H * W
    ratio = np.repeat([1.0, 1e2, 1e3], 4)
    r = (rs.standard_normal((B, H, W, C)) + ratio).astype(np.float32)
    p0 = dict(p, **{'c/BatchNorm/moving_mean': np.zeros(C, np.float32), 'c/BatchNorm/moving_variance': np.zeros(C, np.float32)})
    y, _, mean, rstd, mm, mv = bn_fwd_checked(tr, p0, _dev(r), False)
    ref = _fwd_refs(r, p0)
    (s64, y64), (s32, y32) = ref[np.float64], ref[np.float32]
    dvar = 2.0 ** -23 * (s64['mean'] ** 2 + s64['var'])
    ve = s64['var'] + R.BN_EPS
    drstd = np.maximum(np.abs(1 / np.sqrt(ve - dvar) - 1 / np.sqrt(ve)), np.abs(1 / np.sqrt(ve + dvar) - 1 / np.sqrt(ve)))
    dmv = (1 - R.BN_DECAY) * N / (N - 1.0) * dvar
    dy = np.abs(r.astype(np.float64) - s64['mean']).reshape(-1, C).max(axis=0) * np.abs(p['c/BatchNorm/gamma']) * drstd
    bad = []
    for i, q in enumerate((1, 1e2, 1e3)):
        g = slice(4 * i, 4 * i + 4)
        _report('|mean|/std %g' % q, [('mean', mean[g], s32['mean'][g], s64['mean'][g])])
        for name, got, r32, r64, extra in (('rstd', rstd[g], s32['rstd'][g], s64['rstd'][g], drstd[g].max()), ('mov_var', mv[g], s32['mov_var'][g], s64['mov_var'][g], dmv[g].max()),
                                           ('y', y[..., g], y32[..., g], y64[..., g], R.bound(y32[..., g], y64[..., g]) + dy[g].max())):
            err, bnd = float(np.abs(got.astype(np.float64) - r64).max()), max(R.bound(r32, r64), extra)
            print('  |mean|/std %-6g %-8s err %.3e  bound %.3e  (regular bound %.3e)' % (q, name, err, bnd, R.bound(r32, r64)))
            if not err <= bnd:
                bad.append((q, name, err, bnd))
    assert not bad, bad
    _set_moving(tr, p)


# ------------------------------------------------------------------------------------------------ bf16 handle
@pytest.mark.parametrize('C', [8, 16, 96])
@pytest.mark.parametrize('shape', [s for s, _ in BN_SHAPES], ids=lambda s: '%dx%dx%d' % s)
def test_bn_stage_bf16(handles, C, shape):
    """The same stages on a bf16 handle (bn_apply_kernel<bf16>, max_pool_2x2, max_pool_bwd, bn_bwd_apply_kernel<bf16>; statistics and sums in
    fp32 / double): tensors rounded once to bf16, the restatement on those values rounded to bf16 -- check_bf16_layer: one ulp plus slack, <= 2 %
    of the entries rounded differently; statistics and parameter gradients meet the fp32 bound."""
    tr, p = handles.get(C, 'bf16')
    B, H, W = shape
    rs = np.random.RandomState(C * 100 + H * 10 + W + 1)
    gamma = p['c/BatchNorm/gamma']
    tag = 'bf16 C%d %dx%dx%d' % (C, B, H, W)
    rd = _dev(R.post_relu(rs, (B, H, W, C)), torch.bfloat16)
    r = rd.float().cpu().numpy()
    with pytest.raises(RuntimeError):
        _lib.check(tr._lib.jcm_train_bn_fwd(tr.eng._h, b'nolayer', tr.eng._p(rd), B, H, W, tr.eng._p(rd), None, None, None), 'jcm_train_bn_fwd')
    with pytest.raises(TypeError):
        tr.bn_forward('c', rd.float())      # fp32 tensors on a bf16 handle
    y, po, mean, rstd, mm, mv = bn_fwd_checked(tr, p, rd, True)
    ref = _fwd_refs(r, p)
    (s64, y64), (s32, _) = ref[np.float64], ref[np.float32]
    _report(tag + ' fwd', [('mean', mean, s32['mean'], s64['mean']), ('rstd', rstd, s32['rstd'], s64['rstd']),
                           ('mov_mean', mm, s32['mov_mean'], s64['mov_mean']), ('mov_var', mv, s32['mov_var'], s64['mov_var'])])
    check_bf16_layer(y.astype(np.float64), O.bf16_round(y64))
    assert _same_bits(po, R.max_pool(y)), 'pool_out is not the max pool of the returned y'
    m32, r32 = s64['mean'].astype(np.float32), s64['rstd'].astype(np.float32)
    md, sd = _dev(m32), _dev(r32)
    for pooled in (False, True):
        src = _dev(rs.standard_normal(po.shape if pooled else r.shape) * 1e-3, torch.bfloat16)
        dy = R.max_pool_bwd(y, src.float().cpu().numpy()) if pooled else src.float().cpu().numpy()
        dz, dga, dbe, dbi = bn_bwd_checked(tr, src, rd, _dev(y, torch.bfloat16) if pooled else None, md, sd, 1.0, pooled)
        refs = _bwd_refs(dy, r, m32, r32, gamma, 1.0)
        assert not dz[r <= 0].any()
        check_bf16_layer(dz.astype(np.float64), O.bf16_round(refs[np.float64]['dz']))
        # the bias gradient sums the ROUNDED dz the kernel stored
        _report(tag + (' pooled' if pooled else ' bwd'), [('dgamma', dga, refs[np.float32]['dgamma'], refs[np.float64]['dgamma']),
                                                         ('dbeta', dbe, refs[np.float32]['dbeta'], refs[np.float64]['dbeta'])])
        want = dz.astype(np.float64).reshape(-1, C).sum(axis=0)
        assert (np.abs(dbi - want) <= 2.0 ** -22 * max(np.abs(want).max(), 1e-30)).all(), 'dbias is not the column sum of the stored dz'


# ------------------------------------------------------------------------------------------------ resize adjoint
RESIZE_PAIRS = [(30, 45, 60, 90), (15, 23, 60, 90), (13, 19, 25, 37), (7, 10, 25, 37), (16, 23, 31, 46), (8, 12, 31, 46), (5, 5, 5, 5), (1, 1, 3, 4)]


def resize_bwd_checked(tr, dyd, h, w, scale):
    e = tr.eng
    B, H, W, C = dyd.shape
    res = []
    for _ in range(2):
        dx = Guarded((B, h, w, C), dyd.dtype)
        _lib.check(tr._lib.jcm_train_resize_bwd(e._h, e._p(dyd), B, h, w, H, W, C, ctypes.c_float(scale), e._p(dx.t)), 'jcm_train_resize_bwd')
        torch.cuda.synchronize()
        res.append(dx.check('dx'))
    assert _same_bits(*res), 'a second identical call is not bit-identical'
    return res[0]


@pytest.mark.parametrize('C', [4, 6, 16])      # 4, 16: resize_bwd4_kernel (one and four channel groups); 6: the scalar kernel
@pytest.mark.parametrize('geom', RESIZE_PAIRS, ids=lambda g: '%dx%d-%dx%d' % g)
def test_resize_adjoint_fp32(handles, geom, C):
    """resize_bilinear_bwd against the float64 transpose of the oracle's operator, at the model's three merges (x2 and x4 of 60x90), the odd maps of
    200x296 and 248x368 images (ratios that are no integers: fractional taps, the clamped last row and column), the identity and 1x1, with scale 1 and
    1/3; and <resize(x), dy> == <x, resize_bwd(dy)> with the library's own forward: at ratio 4 a source pixel gathers up to 8 x 8 outputs in fp32, so
    the two sides differ by less than (64 + 4) 2^-24 < 2^-17 of sum |terms|."""
    h, w, H, W = geom
    tr, _ = handles.get(4)
    rs = np.random.RandomState(h * 1000 + W * 10 + C)
    dy = rs.standard_normal((2, H, W, C)).astype(np.float32)
    x = rs.standard_normal((2, h, w, C)).astype(np.float32)
    for scale in (1.0, float(np.float32(1.0 / 3.0))):
        dx = resize_bwd_checked(tr, _dev(dy), h, w, scale)
        _report('%dx%d <- %dx%d C%d x%.2f' % (h, w, H, W, C, scale), [('dx', dx, R.resize_bwd(dy, h, w, scale, np.float32), R.resize_bwd(dy, h, w, scale))])
    up = tr.eng.resize_bilinear(_dev(x), H, W).cpu().numpy().astype(np.float64)
    lhs, rhs = float((up * dy).sum()) * scale, float((x.astype(np.float64) * dx).sum())
    assert abs(lhs - rhs) <= 2.0 ** -17 * float(np.abs(up * dy).sum()) * scale, (lhs, rhs)


@pytest.mark.parametrize('geom', RESIZE_PAIRS, ids=lambda g: '%dx%d-%dx%d' % g)
def test_resize_adjoint_bf16(handles, geom):
    """resize_bwd_kernel<bf16> at C = 8: bf16 dy, fp32 arithmetic, dx rounded to bf16."""
    h, w, H, W = geom
    tr, _ = handles.get(8, 'bf16')
    dyd = _dev(np.random.RandomState(h + W).standard_normal((2, H, W, 8)), torch.bfloat16)
    dx = resize_bwd_checked(tr, dyd, h, w, float(np.float32(1.0 / 3.0)))
    check_bf16_layer(dx.astype(np.float64), O.bf16_round(R.resize_bwd(dyd.float().cpu().numpy(), h, w, float(np.float32(1.0 / 3.0)))))


# ------------------------------------------------------------------------------------------------ losses
def _loss_inputs(rs, HW, K):
    """Four images: logits at scale 1, at scale 40 (exp over its whole range), constant, scale 1; the target map of (image b, joint k) sums to
    (1, 0.4, 0)[(b + k) % 3] (a blob inside the map, one clipped by its border, none)."""
    B = 4
    z = rs.standard_normal((B, HW, K))
    z[1] *= 40
    z[2] = 3.0
    t = rs.uniform(0.01, 1, (B, HW, K + 1))
    sums = np.array([[(1.0, 0.4, 0.0)[(b + k) % 3] for k in range(K)] for b in range(B)])
    t[:, :, :K] *= (sums / t[:, :, :K].sum(axis=1))[:, None, :]
    return z.astype(np.float32), t.astype(np.float32), sums


@pytest.mark.parametrize('K', [1, 9])
@pytest.mark.parametrize('HW', [1, 255, 256, 257, 5400])
def test_softmax_ce_stage(handles, HW, K):
    """softmax_ce at map sizes around the block's 256 threads and the model's 5400, one and nine joints: the loss per map and
    dz (+)= gscale (softmax - target) -- TF's backprop: a map whose target sums to 0.4 or to 0 tells it from the derivative -- with ldz in {K, 16}
    (columns >= K keep their NaN), written and accumulated."""
    tr, _ = handles.get(4)
    e = tr.eng
    rs = np.random.RandomState(HW * 10 + K)
    z, t, sums = _loss_inputs(rs, HW, K)
    B = z.shape[0]
    assert np.abs(t[:, :, :K].astype(np.float64).sum(axis=1) - sums).max() <= 1e-5
    gscale = float(np.float32(1.0 / (B * K)))
    ref = {d: R.softmax_ce(z, t, gscale, dtype=d) for d in (np.float64, np.float32)}
    zd, td = _dev(z), _dev(t)
    for ldz in sorted({K, 16}):
        for acc in (0, 1):
            seed = rs.standard_normal((B, HW, K)).astype(np.float32) * 1e-2
            res = []
            for _ in range(2):
                loss, dz = Guarded((B, K)), Guarded((B, HW, ldz))
                if acc:
                    dz.t[:, :, :K] = _dev(seed)
                _lib.check(tr._lib.jcm_train_softmax_ce(e._h, e._p(zd), e._p(td), B, HW, K, K + 1, ctypes.c_float(gscale), e._p(loss.t), e._p(dz.t), ldz, acc),
                           'jcm_train_softmax_ce')
                torch.cuda.synchronize()
                d = dz.check('dz', written=False)
                assert np.isnan(d[:, :, K:]).all() and not np.isnan(d[:, :, :K]).any(), 'dz: columns >= K written or columns < K left'
                res.append((loss.check('loss'), d[:, :, :K].copy()))
            assert _same_bits(res[0][0], res[1][0]) and _same_bits(res[0][1], res[1][1]), 'a second identical call is not bit-identical'
            add = seed if acc else 0
            _report('HW%d K%d ldz%d acc%d' % (HW, K, ldz, acc),
                    [('loss', res[0][0], ref[np.float32][0], ref[np.float64][0]),
                     ('dz', res[0][1], (ref[np.float32][1] + np.float32(add)).astype(np.float32), ref[np.float64][1] + add)])


@pytest.mark.parametrize('K', [1, 9])
@pytest.mark.parametrize('HW', [1, 255, 256, 257, 5400])
def test_softmax_bwd_stage(handles, HW, K):
    """softmax_bwd: dz += p (g - sum_px p g) per map, g with a stride of 10, dz with a stride of 16 and seeded; its columns >= K keep their NaN."""
    tr, _ = handles.get(4)
    e = tr.eng
    rs = np.random.RandomState(HW * 10 + K + 5)
    z, _, _ = _loss_inputs(rs, HW, K)
    B = z.shape[0]
    p = (R.softmax_ce(z, np.zeros((B, HW, K)), 1.0)[1]).astype(np.float32)      # softmax - 0
    g = rs.standard_normal((B, HW, 10)).astype(np.float32)
    seed = rs.standard_normal((B, HW, K)).astype(np.float32) * 1e-2
    res = []
    for _ in range(2):
        dz = Guarded((B, HW, 16))
        dz.t[:, :, :K] = _dev(seed)
        pd, gd = _dev(p), _dev(g)
        _lib.check(tr._lib.jcm_train_softmax_bwd(e._h, e._p(pd), e._p(gd), B, HW, K, 10, e._p(dz.t), 16), 'jcm_train_softmax_bwd')
        torch.cuda.synchronize()
        d = dz.check('dz', written=False)
        assert np.isnan(d[:, :, K:]).all() and not np.isnan(d[:, :, :K]).any()
        res.append(d[:, :, :K].copy())
    assert _same_bits(*res)
    _report('softmax_bwd HW%d K%d' % (HW, K), [('dz', res[0], (R.softmax_bwd(p, g, np.float32) + seed).astype(np.float32), R.softmax_bwd(p, g) + seed)])


def test_trainer_stage_wrappers(handles):
    """Trainer.bn_forward / bn_backward / resize_backward / softmax_ce / softmax_backward are the entry points above (same bits), with shape checks."""
    tr, p = handles.get(16)
    rs = np.random.RandomState(2)
    r = R.post_relu(rs, (2, 5, 7, 16))
    rd = _dev(r)
    ref = bn_fwd_checked(tr, p, rd, True)
    _set_moving(tr, p)
    y, po, mean, rstd = tr.bn_forward('c', rd, pool=True)
    for a, b in zip(ref[:4], (y, po, mean, rstd)):
        assert _same_bits(a, b.cpu().numpy())
    _set_moving(tr, p)
    dp = _dev(rs.standard_normal(po.shape) * 1e-3)
    want = bn_bwd_checked(tr, dp, rd, y, mean, rstd, 1.0, True)
    got = tr.bn_backward('c', dp, rd, y=y, pooled=True)      # mean / rstd: what the handle kept
    for a, b in zip(want, got):
        assert _same_bits(a, b.cpu().numpy())
    with pytest.raises(ValueError):
        tr.bn_backward('c', dp, rd, pooled=False)
    with pytest.raises(RuntimeError, match='not a conv layer with BatchNorm'):
        tr.bn_forward('conv9', rd)
    dy = _dev(rs.standard_normal((2, 25, 37, 16)))
    assert _same_bits(tr.resize_backward(dy, 13, 19, 0.5).cpu().numpy(), resize_bwd_checked(tr, dy, 13, 19, 0.5))
    z, t, _ = _loss_inputs(rs, 257, 9)
    dz = torch.zeros((4, 257, 16), device='cuda:0')
    loss = tr.softmax_ce(_dev(z), _dev(t), gscale=0.5, dz=dz).cpu().numpy()
    l64, d64 = R.softmax_ce(z, t, 0.5)
    assert np.abs(loss - l64).max() <= 1e-5 * np.abs(l64).max() and np.abs(dz.cpu().numpy()[:, :, :9] - d64).max() <= 1e-6 and not dz[:, :, 9:].any()
    pr = _dev(d64 / 0.5 + t[:, :, :9])
    out = tr.softmax_backward(pr, _dev(rs.standard_normal((4, 257, 10))), torch.zeros((4, 257, 9), device='cuda:0'))
    assert np.isfinite(out.cpu().numpy()).all()
    with pytest.raises(ValueError):
        tr.softmax_ce(_dev(z), _dev(t[:, :100]))
