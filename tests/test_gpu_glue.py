"""The inference glue of csrc/glue.hip and csrc/multiscale.hip, kernel by kernel, against float64 and -- where the code promises it -- against the float32
NumPy evaluation bit for bit: the four three-branch merge kernels (through jcm_upsample_merge3, which launches what the tower launches), the bilinear
resize, the fp32 2x2 max pool, spatial softmax / arg-max on the fused and on the general route, the multi-scale window resize and the group mean.  Shapes,
inputs and references: glue_ref.py (held to itself by test_glue_cpu.py).

The float32 bound of a merged value.  u = 2^-24, M = the largest input magnitude.  One bilinear value: each x-lerp tl + (tr - tl) * tx rounds a difference
of magnitude <= 2M, a product of magnitude <= 2M and a sum of magnitude <= M, scaled by tx <= 1: at most (2 + 2 + 1) u M = 5 u M.  The y-lerp is a convex
combination of the two x-lerps -- it passes on at most 5 u M -- and adds the same three roundings, 5 u M: one lerp carries at most 10 roundings of size
u M.  The merge: x1 + u2 (magnitude <= 2M) and + u3 (<= 3M) round by 2 u M and 3 u M and carry 10 u M from each resized branch; the third divides all of it
by 3 and, correctly rounded (div3), adds u M: (10 + 10 + 2 + 3) / 3 + 1 < 10 u M.  The bar is 12 u M for the merge and 10 u M for the resize alone.

bf16 kernels compute the same float32 value from bf16 inputs and round it once: bit-identical to bf16_round of the float32 evaluation, and against bf16_round
of the float64 one at most one bf16 ulp apart (glue_ref.one_bf16_ulp_apart says what that means next to a power of two and for signed inputs) on a share
of entries of at most 4 x the share on which those two references differ from each other -- a share computed per case, below 0.1 % everywhere
(test_glue_cpu.py).

Measured on an MI355X (printed by every merge case; the table is in CHANGELOG.md): fp32 at most 1.03 x 2^-24 M from float64 (signed inputs; 0.95 on relu
inputs), bf16 differing shares between 0 and 4.2e-4 and on every case EQUAL to the reference-against-reference share, because no entry of any kernel differs
from the float32 evaluation: the bit equality the code promises holds as stated, so it is asserted without exception.  Resize: at most 1.69 x 2^-24 M.
"""
import ctypes
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest
import torch

import joint_cnn_mrf_amd  # noqa: F401
import glue_ref as R
from joint_cnn_mrf_amd import _lib
from oracle import jcm_oracle as O
from oracle import multiscale_oracle as MO

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64
KERNELS = ('f32', 'bf16x4', 'bf16x8', 'planar')


def dev(a, bf16=False):
    t = torch.as_tensor(np.ascontiguousarray(a, dtype=f32), device='cuda:0')
    return t.to(torch.bfloat16) if bf16 else t


def host(t):
    return t.float().cpu().numpy()


@pytest.fixture(scope='module')
def eng():
    """A handle without parameters: none of these kernels reads any.  A bf16 handle beside it shows that jcm_upsample_merge3 does not look at the precision."""
    from joint_cnn_mrf_amd.engine import Engine
    e = Engine(device=0)
    e.finalize()
    yield e
    e.close()


# ------------------------------------------------------------------------------------------------ merge
def run_merge(eng, kernel, xs):
    """The three NHWC float32 arrays through the kernel `kernel` -> NHWC float32 (bf16 kernels: the bf16 result, widened)."""
    bf = kernel != 'f32'
    if kernel == 'planar':
        return R.planar_to_nhwc(host(eng.upsample_merge3(*(dev(R.nhwc_to_planar(x), True) for x in xs), planar=True)))
    ts = [dev(x, bf) for x in xs]
    if bf:
        assert all(np.array_equal(host(t), x) for t, x in zip(ts, xs))      # the inputs were bf16 values already
    out = eng.upsample_merge3(*ts)
    assert out.dtype == ts[0].dtype and out.shape == ts[0].shape
    return host(out)


def check_merge(label, kernel, got, xs, signed, ref32=None, ref64=None):
    """The assertions of the module docstring; the figures are printed before they are asserted.  ref32 / ref64: the float32 and float64 evaluations,
    computed here unless the caller has them."""
    M = R.input_max(xs)
    ref32 = R.merge3_ref(*xs, f32) if ref32 is None else ref32
    ref64 = R.merge3_ref(*xs, f64) if ref64 is None else ref64
    assert got.shape == ref64.shape and np.isfinite(got).all()
    if kernel == 'f32':
        err = float(np.abs(got.astype(f64) - ref64).max()) / (R.U32 * M)
        nbits = int((got.view(np.uint32) != ref32.view(np.uint32)).sum())
        print('merge %-6s %-34s max err %.2f x 2^-24 M, %d entries differ from the float32 evaluation' % (kernel, label, err, nbits))
        assert err <= 12, (label, err)
        assert nbits == 0, (label, nbits)
        return
    r32, r64 = R.bf16_round(ref32), R.bf16_round(ref64).astype(f32)
    share, ref_share = float((got != r64).mean()), float((r32 != r64).mean())
    nbits = int((got.view(np.uint32) != r32.view(np.uint32)).sum())
    print('merge %-6s %-34s differing share %.3e (reference against reference %.3e), %d entries differ from the rounded float32 evaluation'
          % (kernel, label, share, ref_share, nbits))
    assert R.one_bf16_ulp_apart(got, r64, R.bf16_slack(xs, signed)), label
    assert share <= 4 * ref_share, (label, share, ref_share)
    assert nbits == 0, (label, nbits)


@pytest.mark.parametrize('shape', [s for s, _ in R.MERGE_SHAPES], ids=lambda s: '%dx%dx%d_%dx%d_%dx%d' % s)
@pytest.mark.parametrize('kernel', KERNELS)
def test_merge_vs_references(eng, kernel, shape):
    """Every row of the shape table at every channel count of the kernel, relu(N(0,1)) inputs as the tower's: the float64 bound, bit identity with the
    float32 evaluation (module docstring); planar in addition bit-identical to the NHWC bf16x8 kernel on the same values."""
    for C in R.MERGE_CHANNELS[kernel]:
        xs = R.merge_inputs(shape, C, kernel != 'f32')
        got = run_merge(eng, kernel, xs)
        check_merge('%s C=%d' % (shape, C), kernel, got, xs, False)
        if kernel == 'planar':
            assert np.array_equal(got, run_merge(eng, 'bf16x8', xs)), (shape, C)


@pytest.mark.parametrize('kernel', KERNELS)
def test_merge_signed_inputs(eng, kernel):
    """N(0,1) inputs, where the three terms cancel: the model's geometry and the 488 x 712 one."""
    for shape in (R.MERGE_SHAPES[0][0], R.MERGE_SHAPES[1][0]):
        C = R.MERGE_CHANNELS[kernel][1]
        xs = R.merge_inputs(shape, C, kernel != 'f32', signed=True)
        check_merge('%s C=%d signed' % (shape, C), kernel, run_merge(eng, kernel, xs), xs, True)


@pytest.mark.parametrize('case', R.BLOCK_CASES, ids=lambda c: '%d_units' % c['units'])
def test_merge_bf16x8_block_counts(eng, case):
    """upsample_merge3_bf16x8_kernel gives block b the span of block (b % 8) * (n / 8) + b / 8 when the grid n is a multiple of 8: 8 blocks with a partial
    last one, 16 exact ones, and 7 blocks (no remap).  Every output entry must be written once, by the right span."""
    xs = R.merge_inputs(case['shape'], 8, True)
    check_merge('%d units, %d blocks' % (case['units'], case['blocks']), 'bf16x8', run_merge(eng, 'bf16x8', xs), xs, False)


@pytest.mark.parametrize('kernel', KERNELS)
def test_merge_past_the_grid_cap(eng, kernel):
    """More than 16384 * 256 units: the grid-stride loop makes a second, partial lap (13 images of the model's geometry; about 34 M elements, the smallest
    tensor that gets there).  The references are built image by image."""
    shape, C = R.LAP_SHAPE, R.LAP_CHANNELS[kernel]
    assert R.units(kernel, shape, C) > R.GRID_CAP * R.BLOCK
    xs = R.merge_inputs(shape, C, kernel != 'f32')
    got = run_merge(eng, kernel, xs)
    with ThreadPoolExecutor(8) as pool:      # NumPy releases the interpreter lock inside its loops
        per_image = list(pool.map(lambda b: [R.merge3_ref(*(x[b:b + 1] for x in xs), dt) for dt in (f32, f64)], range(shape[0])))
    ref32, ref64 = (np.concatenate([r[i] for r in per_image]) for i in (0, 1))
    check_merge('%s C=%d' % (shape, C), kernel, got, xs, False, ref32, ref64)
    lap2 = R.GRID_CAP * R.BLOCK * R.UNIT_CHANNELS[kernel]      # the first element of the second lap, in the kernel's own element order
    flat = (R.nhwc_to_planar(got) if kernel == 'planar' else got).reshape(-1)
    assert flat.size > lap2 and np.abs(flat[lap2:]).max() > 0


def test_merge_entry_refuses_what_it_cannot_run(eng):
    """JCM_ERR_ARG = 1 before any launch; the binding raises TypeError / ValueError on tensors that do not fit together; a bf16 handle runs the fp32
    kernel on fp32 tensors (the precision of the handle plays no part)."""
    from joint_cnn_mrf_amd.engine import Engine
    x = dev(np.zeros((1, 4, 4, 8), f32))
    p, o = eng._p(x), eng._p(torch.empty_like(x))
    call = eng._lib.jcm_upsample_merge3
    good = dict(x1=p, x2=p, H2=4, W2=4, x3=p, H3=4, W3=4, B=1, H=4, W=4, C=8, is_bf16=0, planar=0, out=o)
    order = ('x1', 'x2', 'H2', 'W2', 'x3', 'H3', 'W3', 'B', 'H', 'W', 'C', 'is_bf16', 'planar', 'out')
    assert call(eng._h, *[good[k] for k in order]) == 0
    null = ctypes.c_void_p(0)
    for bad in (dict(x1=null), dict(x2=null), dict(x3=null), dict(out=null), dict(B=0), dict(H=0), dict(W=-1), dict(H2=0), dict(W2=0), dict(H3=0), dict(W3=0),
                dict(C=0), dict(C=6), dict(C=2), dict(planar=1), dict(planar=1, is_bf16=1, C=12), dict(B=65536, H=65536, W=4),
                dict(B=1 << 16, H=1 << 8, W=1 << 8, C=4),      # 2^32 units exactly
                dict(B=1 << 20, H=1 << 10, W=1 << 3, C=8), dict(B=1 << 20, H=1 << 10, W=1 << 3, C=16, is_bf16=1), dict(B=1 << 30, H2=1 << 30, W2=1 << 30)):
        a = dict(good)
        a.update(bad)
        assert call(eng._h, *[a[k] for k in order]) == 1, bad
        assert 'upsample_merge3' in _lib.last_error()
    xb = x.to(torch.bfloat16)
    with pytest.raises(TypeError):
        eng.upsample_merge3(x, xb, x)
    with pytest.raises(TypeError):
        eng.upsample_merge3(x.double(), x.double(), x.double())
    with pytest.raises(TypeError):
        eng.upsample_merge3(x.view(1, 1, 4, 4, 8), x.view(1, 1, 4, 4, 8), x.view(1, 1, 4, 4, 8), planar=True)
    with pytest.raises(ValueError):
        eng.upsample_merge3(x, x[..., :4].contiguous(), x)
    with pytest.raises(ValueError):
        eng.upsample_merge3(x, x, torch.cat([x, x]))
    with pytest.raises(ValueError):
        eng.upsample_merge3(x[..., :6].contiguous(), x[..., :6].contiguous(), x[..., :6].contiguous())
    with pytest.raises(ValueError):
        eng.upsample_merge3(xb, xb, xb, planar=True)      # four dimensions
    engb = Engine(device=0, precision='bf16')
    try:
        xs = R.merge_inputs(R.MERGE_SHAPES[2][0], 12, False)
        assert np.array_equal(host(engb.upsample_merge3(*(dev(v) for v in xs))), R.merge3_ref(*xs, f32))
    finally:
        engb.close()


# ------------------------------------------------------------------------------------------------ resize, pool
@pytest.mark.parametrize('shape', [s for s, _ in R.RESIZE_SHAPES], ids=lambda s: '%dx%dx%dx%d_to_%dx%d' % s)
def test_resize_vs_references(eng, shape):
    """resize_kernel_c4 / resize_kernel_c1: within 10 * 2^-24 * M of float64 (one lerp, module docstring) and bit-identical to the float32 oracle."""
    B, H, W, C, OH, OW = shape
    x = np.random.RandomState(H + OW).standard_normal((B, H, W, C)).astype(f32)
    got = host(eng.resize_bilinear(dev(x), OH, OW))
    err = float(np.abs(got.astype(f64) - O.resize_bilinear_tf1(x.astype(f64), OH, OW)).max()) / (R.U32 * float(np.abs(x).max()))
    nbits = int((got.view(np.uint32) != O.resize_bilinear_tf1(x, OH, OW).view(np.uint32)).sum())
    print('resize %s: max err %.2f x 2^-24 M, %d entries differ from the float32 oracle' % (shape, err, nbits))
    assert got.shape == (B, OH, OW, C) and err <= 10 and nbits == 0


@pytest.mark.parametrize('shape', R.POOL_SHAPES, ids=lambda s: '%dx%dx%dx%d' % s)
def test_max_pool_fp32_is_exact(eng, shape):
    """Odd heights and widths, a dimension of 1: bit-identical to O.max_pool_same on N(0,1), on a map with -inf entries (a window of -inf only gives -inf)
    and on an all-negative map -- the padding of an odd extent must never win."""
    rs = np.random.RandomState(sum(shape))
    x = rs.standard_normal(shape).astype(f32)
    holes = x.copy()
    holes[rs.random_sample(shape) < 0.6] = -np.inf
    for a in (x, holes, -np.abs(x) - f32(1)):
        got = host(eng.max_pool(dev(a)))
        ref = O.max_pool_same(a)
        assert got.shape == ref.shape == (shape[0], (shape[1] + 1) // 2, (shape[2] + 1) // 2, shape[3])
        assert np.array_equal(got, ref)
    assert np.isneginf(O.max_pool_same(holes)).any() and (O.max_pool_same(-np.abs(x) - f32(1)) < 0).all()


def test_max_pool_refuses_six_channels(eng):
    x = dev(np.zeros((1, 4, 4, 6), f32))
    out = torch.empty((1, 2, 2, 6), device='cuda:0')
    assert eng._lib.jcm_max_pool(eng._h, eng._p(x), 1, 4, 4, 6, eng._p(out)) == 1


# ------------------------------------------------------------------------------------------------ softmax / arg-max
def check_softmax(eng, H, W, K, fused):
    B = 2
    for kind in R.SOFTMAX_KINDS:
        z, want = R.softmax_data(kind, B, H, W, K)
        zd = dev(z)
        prob_t, coords_t = eng.softmax_argmax(zd)
        prob, coords = host(prob_t), coords_t.cpu().numpy()
        ref = O.spatial_softmax(z.astype(f64))
        np.testing.assert_allclose(prob, ref, rtol=2e-5, atol=1e-12, err_msg=kind)
        assert np.abs(prob.astype(f64).sum(axis=(1, 2)) - 1).max() <= 1e-5, kind
        assert np.array_equal(coords, O.argmax_coords(prob)), kind
        if kind == 'neg_inf':
            assert not prob[np.isneginf(z)].any()      # exactly 0
        if want is not None:
            assert np.array_equal(coords, R.coords_of(want, W)), kind
        assert torch.equal(eng.spatial_softmax(zd), prob_t), kind
        assert np.array_equal(eng.argmax_coords(prob_t).cpu().numpy(), coords), kind
        if fused:
            none, only = eng.softmax_argmax(zd, want_prob=False)
            assert none is None and torch.equal(only, coords_t), kind
        else:
            with pytest.raises(RuntimeError, match='without a probability output'):
                eng.softmax_argmax(zd, want_prob=False)


@pytest.mark.parametrize('hw', R.FUSED_MAPS, ids=lambda s: '%dx%d' % s)
def test_fused_softmax_argmax_by_quad_count(eng, hw):
    """softmax_argmax_kernel<9> (K = 9, B = 2) at maps chosen by how many quads fill the register sets j = 0 and j = 1 (glue_ref.FUSED_QUADS): probabilities
    against float64 at rtol 2e-5 / atol 1e-12, each map sums to 1 within 1e-5, the coordinates are np.argmax of the returned probabilities, the
    coordinates-only call returns the same ones, planted ties go to the earlier pixel, -inf pixels get exactly 0."""
    assert R.takes_fused(hw[0] * hw[1], 9)
    check_softmax(eng, hw[0], hw[1], 9, True)


@pytest.mark.parametrize('hwk', R.GENERAL_MAPS, ids=lambda s: '%dx%dx%d' % s)
def test_general_softmax_argmax(eng, hwk):
    """spatial_softmax_kernel + argmax_kernel: HW > 5632, HW % 4 == 2, other joint counts with HW below, at and above one work group's 256 threads.  The
    same assertions; a call without a probability output is refused, as jcm_softmax_argmax documents."""
    H, W, K = hwk
    assert not R.takes_fused(H * W, K)
    check_softmax(eng, H, W, K, False)


def test_argmax_of_all_neg_inf_is_the_origin(eng):
    hm = np.full((2, 7, 9, 3), -np.inf, f32)
    assert not eng.argmax_coords(dev(hm)).cpu().numpy().any()


# ------------------------------------------------------------------------------------------------ window resize, group mean
@pytest.mark.parametrize('kind', R.WINDOW_DATA)
@pytest.mark.parametrize('shape', R.WINDOW_SOURCES, ids=lambda s: '%dx%dx%dx%d' % s)
def test_window_resize_vs_oracle(eng, shape, kind):
    """Engine.window_resize against MO.resize_skimage(MO.take_window(...)): strictly positive data, signed data (0 inside [min, max]: the plain clip) and
    strictly negative data (the padded zeros are the window's maximum and must come out as exact zeros; a crop has 0 outside [min, max]).  Hand-written
    windows that pad on one side, on all, crop to a pixel, to a row, lie wholly outside, plus the tables' own; to the source's size and to an odd one.
    Bars of test_gpu_multiscale.py: atol 2e-7 for the image (values in [-1, 1]), rtol 1e-6 / atol 1e-9 for the heat maps."""
    N, H, W, C = shape
    src = R.window_source(shape, kind)
    wins = R.hand_windows(H, W) + MO.scale_windows(MO.PAD_ARRAY, MO.CROP_ARRAY, H, W) + MO.back_windows(MO.PAD_ARRAY, MO.CROP_ARRAY, H, W)
    full = [(i % N,) + tuple(w) for i, w in enumerate(wins)]
    bars = dict(atol=2e-7, rtol=0) if C == 3 else dict(atol=1e-9, rtol=1e-6)
    for oh, ow in ((H, W), R.ODD_TARGET):
        got = host(eng.window_resize(dev(src), full, oh, ow))
        assert got.shape == (len(full), oh, ow, C)
        zeros = 0
        for i, (si, *win) in enumerate(full):
            ref = MO.resize_skimage(MO.take_window(src[si], win), oh, ow)
            np.testing.assert_allclose(got[i], ref, err_msg='%s window %d %s -> %dx%d' % (kind, i, win, oh, ow), **bars)
            assert not got[i][ref == 0].any(), (kind, i, win)
            zeros += int((ref == 0).sum())
        assert zeros > 0
        print('window_resize %s %s -> %dx%d: %d exact zeros of the reference' % (shape, kind, oh, ow, zeros))


@pytest.mark.parametrize('G', [1, 3, 8])
def test_group_mean_vs_float64(eng, G):
    rs = np.random.RandomState(G)
    x = rs.standard_normal((2 * G, 7, 11, 9)).astype(f32)      # 693 trailing entries: no multiple of 256
    got = host(eng.group_mean(dev(x), G))
    np.testing.assert_allclose(got, x.reshape(2, G, 7, 11, 9).mean(axis=1, dtype=f64), rtol=1e-6, atol=1e-12)
