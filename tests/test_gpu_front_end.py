"""The first launches of every forward pass, kernel by kernel, against the float64 oracle: conv1_<res> + pool1 (at full width ONE fused MFMA kernel of
csrc/conv1_mfma.hip per handle type, with a byte-source twin each) and, on bf16 handles, conv2_<res> + pool2 with the pool's horizontal half in conv2's
epilogue.  Engine.conv1_pool / Engine.conv2_pool run the dispatch functions the tower itself calls (pd_tower.hip: conv1_pool_stage, pool2_layout,
pool2_launch), so what is measured here is what jcm_pd_forward launches.  Shapes and references: front_end_ref.py (checked by test_front_end_cpu.py).

Bars and the worst values measured on an MI355X over every case of this file (printed by each test; relative to max|ref|):

    kernel                                  bar                                       measured worst
    conv1_mfma_pool_split_kernel (+ _u8)    max|got - ref| <= 2e-5 max|ref|           3.5e-07 (table), 2.2e-07 (2560 patches), 2.4e-07 (range cases)
    conv1_mfma_pool_f32_kernel   (+ _u8)    max|got - ref| <= 2e-5 max|ref|           4.5e-07
    conv1_5x5s2_kernel + pool, fp32         max|got - ref| <= 2e-5 max|ref|           3.7e-07
    conv1_mfma_pool_kernel       (+ _u8)    one bf16 ulp, <= 2 % rounded differently  1.7e-03 (one ulp), 2.4e-04 of the entries differ
    conv1_5x5s2_kernel + pool, bf16         one bf16 ulp, <= 2 % rounded differently  6.7e-05 (one ulp of a small entry), 1.8e-04 of the entries differ
    conv2 + pool2 (bf16 handle)             one bf16 ulp, <= 2 % rounded differently  2.8e-03 (one ulp), 9.9e-05 of the entries differ

The fp32 bar is the one test_conv_layer_random_shape holds the split and exact routes to: dropping any one of the split kernel's three part products costs
about 2^-11 = 5e-4 and fails it.  The bf16 bar is check_bf16_layer at its default arguments: with 75-term sums, fp32 against float64 accumulation flips
about 1e-4 of the entries, so the 2 % cap leaves no room to hide a wrong tile.  Bytes against the float call on float32(k) / float32(255): bit identity.

conv2 + pool2, which arm each shape takes (takes_c5strip, i.e. conv5_strip_bf16.hip's make_geom: a 768-slot strip plus four window rows of pitch P = W + 2
must fit 1544 slots, and (ceil((772 + 5 P - 1) / P) + 1) * 2 * ceil(P / 64) window-table entries must fit 96), the same at every resolution and batch here:

    120 x 180 (B 1)   conv2 strip (60 entries), conv3 on 60 x 90 strip (56)   -> planar (pl23), even width: horizontal half in conv2's epilogue (hp)
     60 x  91 (B 2)   conv2 strip (56), conv3 on 30 x 46 strip (44)           -> planar (pl23), odd width: hp off, the 2x2 pool kernel on the planar map
     15 x  23 (B 2)   conv2 strip (72), conv3 on 8 x 12 NOT (122 entries)     -> NHWC throughout, the 2x2 pool kernel
"""
import ctypes

import numpy as np
import pytest
import torch

import joint_cnn_mrf_amd  # noqa: F401
import front_end_ref as R
from joint_cnn_mrf_amd import _lib
from oracle import jcm_oracle as O
from test_gpu_random_shapes import check_bf16_layer
from test_gpu_u8 import as_float, byte_images, unaligned

pytestmark = pytest.mark.gpu
f32 = np.float32
GENERIC = 'conv1_5x5s2_kernel'
# handle -> (Engine keywords, the fused kernel such a handle takes where both sub-sampled extents are multiples of 4)
HANDLES = {'fp32': (dict(), 'conv1_mfma_pool_split_kernel'),
           'fp32_chain': (dict(conv9_fft=False), 'conv1_mfma_pool_f32_kernel'),
           'bf16': (dict(precision='bf16'), 'conv1_mfma_pool_kernel')}
WORST = {}      # kernel label -> [worst relative error, worst share of entries that differ at all]


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), device='cuda:0')


@pytest.fixture(scope='module')
def engines():
    from joint_cnn_mrf_amd.engine import Engine
    p = R.front_end_params()
    e = {name: Engine(device=0, **kw).load_params(p) for name, (kw, _) in HANDLES.items()}
    yield e
    for eng in e.values():
        eng.close()
    for label in sorted(WORST):
        print('front end, worst over the module: %-44s rel %.3e  differing %.3e' % ((label,) + tuple(WORST[label])))


def held_to_oracle(label, got, ref, bf):
    """got (device tensor) against the float64 reference under the bar of its handle type; the figures are printed before they are asserted."""
    g = got.float().cpu().numpy().astype(np.float64)
    assert g.shape == ref.shape, (g.shape, ref.shape)
    assert got.dtype == (torch.bfloat16 if bf else torch.float32)
    assert np.isfinite(g).all()
    err = float(np.abs(g - ref).max() / np.abs(ref).max())
    differ = float((g != ref).mean())
    w = WORST.setdefault(label + (', bf16' if bf else ', fp32'), [0.0, 0.0])
    w[0], w[1] = max(w[0], err), max(w[1], differ if bf else 0.0)
    print('%-40s %s rel err %.3e%s' % (label, 'bf16' if bf else 'fp32', err, ', differing %.3e' % differ if bf else ''))
    if bf:
        check_bf16_layer(g, ref)
    else:
        assert err <= 2e-5, '%s: %.3e' % (label, err)


def refs(x, p, scope, sub):
    return {False: R.conv1_pool_ref(x, p, scope, sub), True: R.conv1_pool_ref(x, p, scope, sub, emulate='bf16')}


@pytest.mark.parametrize('B', R.BATCHES)
@pytest.mark.parametrize('sub', R.SUBS)
@pytest.mark.parametrize('row', R.SHAPES, ids=lambda r: '%dx%d' % r['hw'])
def test_conv1_pool_vs_oracle(engines, row, sub, B):
    """Every row of the shape table, read at every sub-th pixel of a sub * H x sub * W image (the strided addressing (gy * sub) * W0 + gx * sub), on the
    three handle types: the kernel is the one the row is there for, the float call is within the bar of the oracle, the byte calls (aligned, and
    starting at an odd address) equal the float call on float32(k) / float32(255) bit for bit -- and that float call is itself held to the oracle."""
    H, W = row['hw']
    scope = 'conv1_' + R.RES_OF_SUB[sub]
    p = R.front_end_params()
    rs = np.random.RandomState(1000 * H + 10 * W + sub + B)
    x = rs.standard_normal((B, sub * H, sub * W, 3)).astype(f32)
    k = byte_images(4, sub * H, sub * W, seed=H + W + sub)[4 - B:]      # B = 1: a random image; B = 3: all 255, the full ramp, a random image
    xk = as_float(k)
    ref_x, ref_k = refs(x, p, scope, sub), refs(xk, p, scope, sub)
    assert ref_x[False].shape == (B,) + row['pooled'] + (64,)
    xd, xkd, kd = dev(x), dev(xk), (dev(k), unaligned(k, 1))
    for name, (_, fused) in HANDLES.items():
        eng, bf = engines[name], name == 'bf16'
        kernel = fused if row['fused'] else GENERIC
        assert eng.conv_kernel_name(scope, B, H, W) == kernel      # H, W: the layer's own input extents
        held_to_oracle(kernel, eng.conv1_pool(xd, scope, sub), ref_x[bf], bf)
        want = eng.conv1_pool(xkd, scope, sub)
        held_to_oracle(kernel, want, ref_k[bf], bf)
        for kb in kd:
            got = eng.conv1_pool(kb, scope, sub)
            assert got.dtype == want.dtype and torch.equal(got, want), (name, kb.data_ptr() % 4)


def test_conv1_pool_persistent_loop(engines):
    """160 images of 128 x 128: 2560 patches, more than the 2048 work groups of 256 threads the chip can hold, so every work group of the persistent
    kernels walks t += gridDim.x and consumes a window it prefetched during the previous patch.  Four images against the oracle; EVERY image bit for
    bit against the same image run alone (16 patches: no work group takes a second one); bytes against floats."""
    c = R.PERSISTENT
    B, (H, W) = c['B'], c['hw']
    p = R.front_end_params()
    rs = np.random.RandomState(160)
    x = rs.standard_normal((B, H, W, 3)).astype(f32)
    k = rs.randint(0, 256, (B, H, W, 3)).astype(np.uint8)
    pick = list(c['compare'])
    ref = refs(x[pick], p, 'conv1_fullres', 1)
    xd, kd, xkd = dev(x), dev(k), dev(as_float(k))
    for name, (_, fused) in HANDLES.items():
        eng, bf = engines[name], name == 'bf16'
        assert eng.conv_kernel_name('conv1_fullres', B, H, W) == fused
        got = eng.conv1_pool(xd, 'conv1_fullres')
        held_to_oracle(fused + ' (2560 patches)', got[pick], ref[bf], bf)
        for b in range(B):
            assert torch.equal(eng.conv1_pool(xd[b:b + 1], 'conv1_fullres')[0], got[b]), (name, b)
        assert torch.equal(eng.conv1_pool(kd, 'conv1_fullres'), eng.conv1_pool(xkd, 'conv1_fullres')), name


def _range_images(case):
    rs = np.random.RandomState(64)
    x = rs.standard_normal((2, 64, 96, 3)).astype(f32)
    if case == 'halves':      # windows on the seam hold both ranges; each window is lifted by its own largest value
        x[:, :, :48] *= f32(1e-6)
        x[:, :, 48:] *= f32(255)
    elif case == 'zero_window':      # patch (1, 1) reads rows and columns 32 - 1 .. 32 - 1 + 34 (rows 64, 65 are padding): an all-zero window takes the no-scaling branch
        x[:, 31:, 31:66] = 0
    else:
        x *= f32(case)
    return x


@pytest.mark.parametrize('case', ['halves', 'zero_window', 1e-9, 3e7], ids=lambda c: str(c))
def test_conv1_split_kernel_is_range_free(engines, case):
    """conv1_mfma_pool_split_kernel lifts every 35 x 35 window into the fp16 range by the window's OWN power of two (none for a window whose largest value
    is zero, vanishing or not finite): the kernel inherits fp32's range whatever the image holds.  The gains are those of test_split16_is_range_free."""
    x = _range_images(case)
    if case == 'zero_window':
        g = R.conv1_geometry(64, 96)
        y0 = R.PATCH * 2 - g['pad'][0]
        assert y0 == 31 and y0 + 35 >= 64 and not x[:, y0:, y0:y0 + 35].any() and x[:, y0 - 1].all() and x[:, :, y0 - 1].all() and x[:, :, y0 + 35].all()
    eng = engines['fp32']
    assert eng.conv_kernel_name('conv1_fullres', 2, 64, 96) == 'conv1_mfma_pool_split_kernel'
    ref = R.conv1_pool_ref(x, R.front_end_params(), 'conv1_fullres')
    held_to_oracle('conv1_mfma_pool_split_kernel (range: %s)' % case, eng.conv1_pool(dev(x), 'conv1_fullres'), ref, False)


# (B, h, w) -> the kernel conv3 takes on the pooled map; conv2 takes conv5_strip_bf16_kernel on all three (module docstring: which of pl23 / hp follows)
CONV2_SHAPES = {(1, 120, 180): 'conv5_strip_bf16_kernel', (2, 60, 91): 'conv5_strip_bf16_kernel', (2, 15, 23): 'conv_igemm_bf16_kernel'}


@pytest.mark.parametrize('shape', sorted(CONV2_SHAPES), ids=lambda s: 'B%d_%dx%d' % s)
@pytest.mark.parametrize('res', ['fullres', 'halfres', 'quarterres'])
def test_conv2_pool_bf16_vs_oracle(engines, res, shape):
    """conv2_<res> + pool2 of a bf16 handle, as the tower runs them: planar activations where conv2 and conv3 both take the strip kernel, the pool's
    horizontal half in conv2's epilogue on an even width (vpool_2x1_bf16_kernel finishes it).  Against the oracle in bf16 arithmetic; with option
    bf16_hpool = 0 (the 2x2 pool kernel on the full-width map) the result must not change by a bit -- the max of rounded values is the rounded max."""
    B, h, w = shape
    c2, c3 = 'conv2_' + res, 'conv3_' + res
    p = R.front_end_params()
    rs = np.random.RandomState(h * 1000 + w + len(res))
    p1 = O.bf16_round(np.maximum(rs.standard_normal((B, h, w, 64)), 0).astype(f32))
    ref = R.conv2_pool_ref(p1, p, c2)
    eng = engines['bf16']
    assert eng.conv_kernel_name(c2, B, h, w) == 'conv5_strip_bf16_kernel'
    assert eng.conv_kernel_name(c3, B, (h + 1) // 2, (w + 1) // 2) == CONV2_SHAPES[shape]
    p1d = dev(p1).to(torch.bfloat16)
    assert np.array_equal(p1d.float().cpu().numpy(), p1)
    got = eng.conv2_pool(p1d, c2)
    held_to_oracle('conv2 + pool2 %dx%d' % (h, w), got, ref, True)
    eng.set_option('bf16_hpool', 0)
    try:
        plain = eng.conv2_pool(p1d, c2)
    finally:
        eng.set_option('bf16_hpool', 1)
    assert torch.equal(plain, got)


def test_front_end_entries_refuse_what_they_cannot_run(engines):
    """Arguments are checked before any launch (JCM_ERR_ARG = 1), a wrong dtype is a TypeError of the binding, and an fp32 handle says why it has no
    conv2 + pool2 (JCM_ERR_STATE)."""
    eng, engb = engines['fp32'], engines['bf16']
    x = dev(np.zeros((1, 8, 8, 3), f32))
    out = torch.empty((1, 2, 2, 64), device='cuda:0')
    for bad in (dict(sub=3), dict(sub=0), dict(H=6, sub=4), dict(B=0), dict(B=65536), dict(W=0)):
        a = dict(B=1, H=8, W=8, sub=1)
        a.update(bad)
        assert eng._lib.jcm_conv1_pool(eng._h, b'conv1_fullres', eng._p(x), 0, a['B'], a['H'], a['W'], a['sub'], eng._p(out)) == 1, bad
    assert eng._lib.jcm_conv1_pool(eng._h, b'conv2_fullres', eng._p(x), 0, 1, 8, 8, 1, eng._p(out)) == 1      # not a Cin = 3 layer
    assert 'Cin = 3' in _lib.last_error()
    assert eng._lib.jcm_conv1_pool(eng._h, b'nothing', eng._p(x), 0, 1, 8, 8, 1, eng._p(out)) == 2            # JCM_ERR_STATE: no such layer
    assert eng._lib.jcm_conv1_pool(eng._h, b'conv1_fullres', ctypes.c_void_p(0), 0, 1, 8, 8, 1, eng._p(out)) == 1
    with pytest.raises(ValueError, match='sub must be'):
        eng.conv1_pool(x, 'conv1_fullres', sub=3)
    for bad in (x.double(), x.half(), x.to(torch.int8)):
        with pytest.raises(TypeError, match='x must be torch.float32'):
            eng.conv1_pool(bad, 'conv1_fullres')
    p1 = torch.zeros((1, 8, 8, 64), dtype=torch.bfloat16, device='cuda:0')
    with pytest.raises(TypeError, match='p1 must be torch.bfloat16'):
        engb.conv2_pool(p1.float(), 'conv2_fullres')
    with pytest.raises(RuntimeError, match='this is an fp32 handle'):
        eng.conv2_pool(p1, 'conv2_fullres')
    o2 = torch.empty((1, 4, 4, 128), dtype=torch.bfloat16, device='cuda:0')
    assert engb._lib.jcm_conv2_pool(engb._h, b'conv1_fullres', engb._p(p1), 1, 8, 8, engb._p(o2)) == 1      # scope must be conv2_<res>
    assert engb._lib.jcm_conv2_pool(engb._h, b'conv2_nowhere', engb._p(p1), 1, 8, 8, engb._p(o2)) == 2
    assert engb._lib.jcm_conv2_pool(engb._h, b'conv2_fullres', engb._p(p1), 1, 0, 8, engb._p(o2)) == 1
