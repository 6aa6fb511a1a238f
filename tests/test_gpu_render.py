"""The pose renderer on the GPU (csrc/render.hip): jcm_render_poses and Engine.render_poses against the numpy restatement
tests/render_ref.py (pinned by tests/test_render_cpu.py), bit for bit and with no tolerance, on ragged batches at odd byte offsets; and every
argument error, each of which must leave a pre-filled output untouched."""
import ctypes

import numpy as np
import pytest
import torch
from numpy.testing import assert_array_equal

import fit_ref as F
import render_ref as R
import joint_cnn_mrf_amd  # noqa: F401
from joint_cnn_mrf_amd import _lib

pytestmark = pytest.mark.gpu
ERR_ARG = 1
FILL = 0x5A
WHITE = 0xFFFFFF
SIZES = ((1, 1), (1, 7), (5, 3), (40, 60), (70, 90), (200, 300))      # 200 x 300 is eight tiles of 8192 pixels, cut inside rows


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), device='cuda:0')


@pytest.fixture(scope='module')
def eng():
    """A handle without parameters: the renderer needs none."""
    from joint_cnn_mrf_amd.engine import Engine
    e = Engine(device=0)
    yield e
    e.close()


def _i32(a):
    return np.ascontiguousarray(a, np.int32).ctypes.data_as(ctypes.POINTER(ctypes.c_int32))


def _call(e, buf, desc, prims, heat=None, in_place=False, B=None, NP=None, src_bytes=None, null=(), out_shift=None):
    """jcm_render_poses at the C ABI on a packed buffer -> (status, out (host), was the pre-filled out left untouched?).  heat: dict(hm, geom,
    heat_mask, heat_gain, stride) with hm a host array.  out_shift: out = src + out_shift bytes, a partial overlap."""
    from joint_cnn_mrf_amd.engine import Engine
    p = Engine._p
    desc = np.ascontiguousarray(desc, np.int64)
    prims = np.ascontiguousarray(np.asarray(prims, np.int64).reshape(-1, 8), np.int32)
    n = len(buf)
    if out_shift is not None:
        both = torch.full((2 * n,), FILL, dtype=torch.uint8, device='cuda:0')
        src, out = both[:n], both[out_shift:out_shift + n]
        src.copy_(_dev(buf))
        before = both.cpu().numpy()
    else:
        src = _dev(buf)
        out = src if in_place else torch.full((n,), FILL, dtype=torch.uint8, device='cuda:0')
    h = dict(hm=None, geom=None, heat_mask=None, heat_gain=0, stride=0) if heat is None else dict(heat)
    hm = None if h['hm'] is None else _dev(np.asarray(h['hm'], np.float32))
    hh, hw, K = (0, 0, 0) if hm is None else hm.shape[1:]
    hh, hw, K = h.get('hh', hh), h.get('hw', hw), h.get('K', K)
    geom = None if h['geom'] is None else np.ascontiguousarray(h['geom'], np.int32)
    mask = None if h['heat_mask'] is None else np.ascontiguousarray(h['heat_mask'], np.uint8)
    torch.cuda.synchronize()
    st = e._lib.jcm_render_poses(e._h, p(None if 'src' in null else src), n if src_bytes is None else src_bytes,
                                 None if 'desc' in null else desc.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), len(desc) if B is None else B,
                                 p(None if 'out' in null else out), None if ('prims' in null or len(prims) == 0) else _i32(prims),
                                 len(prims) if NP is None else NP, p(hm), int(hh), int(hw), int(K), int(h['stride']),
                                 None if geom is None else _i32(geom), None if mask is None else mask.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)),
                                 int(h['heat_gain']))
    torch.cuda.synchronize()
    if out_shift is not None:
        return st, None, bool((both.cpu().numpy() == before).all())
    got = out.cpu().numpy()
    return st, got, bool((got == (buf if in_place else FILL)).all())


def _want(buf, desc, prims, in_place=False, **heat):
    return R.render_packed(buf, desc, buf if in_place else np.full(len(buf), FILL, np.uint8), prims, **heat)


def capsules(rs, sizes, n, rmax=200):
    """n seeded random capsules over the images, sorted by image: ends up to three pixels outside, any colour, any alpha."""
    rows = []
    for b in np.sort(rs.randint(0, len(sizes), n)):
        h, w = sizes[b]
        rows.append((b, rs.randint(-48, 16 * h + 48), rs.randint(-48, 16 * w + 48), rs.randint(-48, 16 * h + 48), rs.randint(-48, 16 * w + 48),
                     rs.randint(0, rmax + 1), rs.randint(0, 1 << 24), rs.randint(0, 256)))
    return np.array(rows, np.int64).reshape(-1, 8)


@pytest.fixture(scope='module')
def six():
    rs = np.random.RandomState(5)
    images = [rs.randint(0, 256, (h, w, 3)).astype(np.uint8) for h, w in SIZES]
    buf, desc = F.pack(images)
    assert (desc[:, 0] % 2 == 1).all() and len({int(o) % 16 for o in desc[:, 0]}) > 2
    return images, buf, desc


def test_no_primitives_is_a_bit_copy(eng, six):
    images, buf, desc = six
    st, got, _ = _call(eng, buf, desc, [])
    assert st == 0, _lib.last_error()
    for (o, h, w), im in zip(desc, images):
        assert_array_equal(got[o:o + 3 * h * w], im.reshape(-1))
    assert_array_equal(got, _want(buf, desc, []))      # the bytes between the images keep the pre-filled value
    assert (got == FILL).sum() >= len(buf) - sum(im.size for im in images)


def test_closed_forms(eng):
    images = [np.zeros((9, 9, 3), np.uint8)] * 2
    buf, desc = F.pack(images)
    prims = [(0, 64, 64, 64, 64, 8, WHITE, 255), (1, 64, 32, 64, 96, 16, WHITE, 255)]
    st, got, _ = _call(eng, buf, desc, prims)
    assert st == 0, _lib.last_error()
    disc, limb = (got[o:o + 243].reshape(9, 9, 3) for o in desc[:, 0])
    want = np.zeros((9, 9, 3), np.uint8)
    want[4, 4] = 191
    assert_array_equal(disc, want)
    assert (limb[4, 2:7] == 255).all() and (limb[3, 2:7] == 128).all() and (limb[5, 2:7] == 128).all() and not limb[2].any() and not limb[6].any()
    assert_array_equal(got, _want(buf, desc, prims))


def test_edges_corners_and_degenerate(eng, six):
    """Image 3 (40 x 60) between images without a primitive: capsules across every edge and corner, one wholly outside, r = 0, a == b, alpha 0,
    and two opaque discs on one pixel; image 5 (eight tiles) gets one long diagonal."""
    _, buf, desc = six
    H, W = 16 * 39, 16 * 59
    prims = [(3, -40, 300, 60, 320, 30, 0xFF0000, 255), (3, H - 20, 500, H + 90, 480, 25, 0x00FF00, 200), (3, 300, -50, 280, 40, 20, 0x0000FF, 255),
             (3, 100, W - 10, 130, W + 80, 35, 0xFFFF00, 128), (3, -30, -30, 30, 30, 40, 0xFF00FF, 255), (3, -20, W + 20, 40, W - 40, 40, 0x00FFFF, 255),
             (3, H + 20, -20, H - 30, 30, 40, WHITE, 90), (3, H + 10, W + 10, H - 20, W - 20, 33, 0x123456, 255),
             (3, -400, -400, -300, 2000, 50, WHITE, 255), (3, 320, 480, 330, 520, 0, WHITE, 255), (3, 402, 642, 402, 642, 0, WHITE, 255),
             (3, 200, 200, 200, 200, 37, 0x808080, 255), (3, 500, 100, 400, 300, 60, WHITE, 0),
             (3, 480, 800, 480, 800, 64, 0xFF0000, 255), (3, 480, 800, 480, 800, 64, 0x0000FF, 255),
             (5, -100, -100, 16 * 199 + 100, 16 * 299 + 100, 90, 0x40C0FF, 170)]
    st, got, _ = _call(eng, buf, desc, prims)
    assert st == 0, _lib.last_error()
    o, h, w = desc[3]
    assert tuple(got[o:o + 3 * h * w].reshape(h, w, 3)[30, 50]) == (0, 0, 255)      # the later opaque disc wins
    assert_array_equal(got, _want(buf, desc, prims))
    for b in (0, 1, 2, 4):
        o, h, w = desc[b]
        assert_array_equal(got[o:o + 3 * h * w], buf[o:o + 3 * h * w])


def test_256_primitives_on_one_image(eng, six):
    _, buf, desc = six
    prims = capsules(np.random.RandomState(8), [SIZES[4]], 256, rmax=120)
    prims[:, 0] = 4
    st, got, _ = _call(eng, buf, desc, prims)
    assert st == 0, _lib.last_error()
    assert_array_equal(got, _want(buf, desc, prims))


def test_200_random_capsules(eng, six):
    _, buf, desc = six
    prims = capsules(np.random.RandomState(9), SIZES, 200)
    st, got, _ = _call(eng, buf, desc, prims)
    assert st == 0, _lib.last_error()
    want = _want(buf, desc, prims)
    assert_array_equal(got, want)
    st, got, _ = _call(eng, buf, desc, prims, in_place=True)      # out == src
    assert st == 0, _lib.last_error()
    assert_array_equal(got, _want(buf, desc, prims, in_place=True))


def test_65_images_cross_the_launch_boundary(eng):
    rs = np.random.RandomState(10)
    images = [rs.randint(0, 256, (3, 5, 3)).astype(np.uint8) for _ in range(65)]
    buf, desc = F.pack(images)
    prims = [(b, 16, 0, 16, 64, 12, rgb, 255) for b, rgb in ((0, 0xFF0000), (62, 0x00FF00), (63, 0x0000FF), (64, WHITE))]
    prims.append((64, 0, 32, 32, 32, 8, 0x102030, 180))
    st, got, _ = _call(eng, buf, desc, prims)
    assert st == 0, _lib.last_error()
    assert_array_equal(got, _want(buf, desc, prims))
    o = desc[64, 0]
    assert tuple(got[o:o + 45].reshape(3, 5, 3)[1, 0]) == (255, 255, 255)


def test_tiles_inside_one_row(eng):
    """2 x 9000: a row is wider than a tile, so tiles lie inside one row and are culled by column as well."""
    rs = np.random.RandomState(12)
    images = [rs.randint(0, 256, (2, 9000, 3)).astype(np.uint8)]
    buf, desc = F.pack(images)
    prims = [(0, 8, 16 * 8100, 24, 16 * 8300, 40, 0xFF8000, 255), (0, 0, -100, 16, 16 * 9000, 6, 0x00FF80, 150), (0, 16, 16 * 8191, 16, 16 * 8192, 10, WHITE, 255)]
    st, got, _ = _call(eng, buf, desc, prims)
    assert st == 0, _lib.last_error()
    assert_array_equal(got, _want(buf, desc, prims))


@pytest.fixture(scope='module')
def tinted():
    """A portrait, a landscape and a frame-sized source for 6 x 9 maps at stride 8 (a 48 x 72 frame), their letterbox geometries from fit_ref."""
    rs = np.random.RandomState(13)
    sizes = ((70, 33), (31, 90), (48, 72), (5, 3))
    images = [rs.randint(0, 200, (h, w, 3)).astype(np.uint8) for h, w in sizes]
    buf, desc = F.pack(images)
    geom = np.array([F.geometry(h, w, 48, 72) for h, w in sizes], np.int32)
    assert geom[0, 1] > 0 and geom[1, 0] > 0 and geom[2].tolist() == [0, 0, 48, 72]      # bars left/right, bars top/bottom, none
    hm9 = rs.rand(4, 6, 9, 9).astype(np.float32) ** 4
    hm9[:, :, :, 4] = 0.0         # an all-zero map: M = 0, the joint adds nothing
    hm9[3] = 0.0                  # an image whose maps are all zero
    hm9[1, :, :, 2] -= 0.5        # negative values clamp at 0
    return sizes, buf, desc, geom, hm9, rs.rand(4, 6, 9, 1).astype(np.float32)


@pytest.mark.parametrize('gain', (0, 128, 255))
def test_tint(eng, tinted, gain):
    from joint_cnn_mrf_amd.predict import HEAT_MASK
    sizes, buf, desc, geom, hm9, hm1 = tinted
    for hm, mask in ((hm9, HEAT_MASK), (hm1, (7,))):
        heat = dict(hm=hm, geom=geom, heat_mask=mask, heat_gain=gain, stride=8)
        st, got, _ = _call(eng, buf, desc, [], heat=heat)
        assert st == 0, _lib.last_error()
        assert_array_equal(got, _want(buf, desc, [], **heat))
        if gain == 0:
            assert_array_equal(got, _want(buf, desc, []))


def test_tint_and_capsules(eng, tinted):
    from joint_cnn_mrf_amd.predict import HEAT_MASK
    sizes, buf, desc, geom, hm9, _ = tinted
    prims = capsules(np.random.RandomState(14), sizes, 40, rmax=100)
    heat = dict(hm=hm9, geom=geom, heat_mask=HEAT_MASK, heat_gain=255, stride=8)
    for in_place in (False, True):
        st, got, _ = _call(eng, buf, desc, prims, heat=heat, in_place=in_place)
        assert st == 0, _lib.last_error()
        assert_array_equal(got, _want(buf, desc, prims, in_place=in_place, **heat))


def test_engine_render_poses(eng, tinted):
    """Engine.render_poses: host arrays and device tensors mixed, the maps as one tensor and as a list of views, geom as fit_images returns it."""
    from joint_cnn_mrf_amd.predict import HEAT_MASK
    sizes, buf, desc, geom, hm9, _ = tinted
    images = [buf[o:o + 3 * h * w].reshape(h, w, 3).copy() for o, h, w in desc]
    prims = capsules(np.random.RandomState(15), sizes, 30, rmax=100)
    mixed = [images[0], _dev(images[1]), torch.from_numpy(images[2]), _dev(images[3])]
    got = eng.render_poses(mixed, prims)
    assert [tuple(g.shape) for g in got] == [(h, w, 3) for h, w in sizes] and all(g.dtype == torch.uint8 and g.is_cuda for g in got)
    for g, want in zip(got, R.render(images, prims)):
        assert_array_equal(g.cpu().numpy(), want)
    for g, im in zip(eng.render_poses(images, np.zeros((0, 8), np.int32)), images):
        assert_array_equal(g.cpu().numpy(), im)
    geom6 = np.concatenate([geom, np.array(sizes, np.int32)], axis=1)
    hm = _dev(hm9)
    want = R.render(images, prims, hm=hm9, geom=geom, heat_mask=HEAT_MASK, heat_gain=200, stride=8)
    for maps in (hm, [hm[b] for b in range(4)]):
        got = eng.render_poses(images, prims, hm=maps, geom=geom6, heat_mask=HEAT_MASK, heat_gain=200)
        for g, w in zip(got, want):
            assert_array_equal(g.cpu().numpy(), w)
    with pytest.raises(ValueError):
        eng.render_poses(images, prims[:, :7])
    with pytest.raises(ValueError):
        eng.render_poses(images, prims, hm=hm)
    with pytest.raises(ValueError):
        eng.render_poses(images, prims, hm=hm, geom=geom6[:3], heat_mask=HEAT_MASK)
    with pytest.raises(RuntimeError):
        eng.render_poses(images, prims[::-1])      # out of order: the library refuses it


def test_argument_errors(eng, tinted):
    from joint_cnn_mrf_amd.predict import HEAT_MASK
    sizes, buf, desc, geom, hm9, _ = tinted
    ok = [(0, 10, 10, 40, 40, 8, WHITE, 255), (2, 10, 10, 40, 40, 8, WHITE, 255)]
    heat = dict(hm=hm9, geom=geom, heat_mask=HEAT_MASK, heat_gain=255, stride=8)

    def bad_desc(b, col, v):
        d = desc.copy()
        d[b, col] = v
        return d

    def bad_prim(col, v, row=1):
        p = np.array(ok, np.int64)
        p[row, col] = v
        return p

    cases = [dict(null=('src',)), dict(null=('desc',)), dict(null=('out',)), dict(B=0), dict(B=-1),
             dict(desc=bad_desc(1, 1, 0)), dict(desc=bad_desc(1, 2, 16385)), dict(desc=bad_desc(0, 1, 16385)), dict(desc=bad_desc(0, 0, -1)),
             dict(desc=bad_desc(3, 0, len(buf) - 44)), dict(src_bytes=len(buf) - 1), dict(out_shift=1), dict(out_shift=len(buf) - 1),
             dict(NP=-1), dict(null=('prims',), NP=2),
             dict(prims=bad_prim(0, 4)), dict(prims=bad_prim(0, -1, row=0)), dict(prims=bad_prim(0, 1, row=0)[::-1]),
             dict(prims=[(1, 0, 0, 0, 0, 1, 0, 255)] * 257),
             dict(prims=bad_prim(1, (1 << 20) + 1)), dict(prims=bad_prim(4, -(1 << 20) - 1)), dict(prims=bad_prim(5, -1)), dict(prims=bad_prim(5, (1 << 16) + 1)),
             dict(prims=bad_prim(7, 256)), dict(prims=bad_prim(7, -1)), dict(prims=bad_prim(6, 0x1000000)), dict(prims=bad_prim(6, -1)),
             dict(heat=dict(heat, geom=None)), dict(heat=dict(heat, heat_mask=None)), dict(heat=dict(heat, K=0)), dict(heat=dict(heat, K=17)),
             dict(heat=dict(heat, hh=0)), dict(heat=dict(heat, hw=0)), dict(heat=dict(heat, stride=0)), dict(heat=dict(heat, heat_gain=256)),
             dict(heat=dict(heat, heat_gain=-1)), dict(heat=dict(heat, geom=np.where(np.arange(4)[None, :] == 2, 0, geom))),
             dict(heat=dict(heat, geom=np.where(np.arange(4)[None, :] == 3, 0, geom)))]
    for kw in cases:
        kw = dict(kw)
        st, _, untouched = _call(eng, buf, kw.pop('desc', desc), kw.pop('prims', ok), **kw)
        assert st == ERR_ARG and untouched and 'render_poses' in _lib.last_error(), (kw, st, _lib.last_error())
    # the limits themselves are accepted
    edge = [(0, 1 << 20, -(1 << 20), 0, 0, 1 << 16, WHITE, 255)] + [(1, 0, 0, 0, 0, 1, 0, 255)] * 256
    st, got, _ = _call(eng, buf, desc, edge)
    assert st == 0, _lib.last_error()
    assert_array_equal(got, _want(buf, desc, edge))
