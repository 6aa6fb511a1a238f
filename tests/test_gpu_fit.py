"""The letterbox fit on the GPU (csrc/fit.hip): jcm_fit_images against the float64 restatement tests/fit_ref.py (pinned by
tests/test_fit_cpu.py), bit for bit, for byte and float outputs; the geometry it reports; the reduction limit; and every argument error, each of
which must leave a pre-filled output untouched."""
import ctypes

import numpy as np
import pytest
import torch
from numpy.testing import assert_array_equal

import fit_ref as F
import joint_cnn_mrf_amd  # noqa: F401
from joint_cnn_mrf_amd import _lib

pytestmark = pytest.mark.gpu
ERR_ARG = 1


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), device='cuda:0')


@pytest.fixture(scope='module')
def eng():
    """A handle without parameters: the fit needs none."""
    from joint_cnn_mrf_amd.engine import Engine
    e = Engine(device=0)
    yield e
    e.close()


def _call(e, buf, desc, OH, OW, pad=0, f32=False, C=3, B=None, src_bytes=None, fill=0x5A, null=(), want_geom=True):
    """jcm_fit_images at the C ABI on a packed buffer -> (status, out (host), geom (host), was the pre-filled out left untouched?)."""
    from joint_cnn_mrf_amd.engine import Engine
    p = Engine._p
    B = len(desc) if B is None else B
    n = max(len(desc), 1)
    src = _dev(buf)
    out = torch.full((n, OH, OW, C), fill, dtype=torch.float32 if f32 else torch.uint8, device='cuda:0')
    geom = np.full((n, 4), -77, np.int32)
    desc = np.ascontiguousarray(desc, np.int64)
    torch.cuda.synchronize()
    st = e._lib.jcm_fit_images(e._h, p(None if 'src' in null else src), len(buf) if src_bytes is None else src_bytes,
                               None if 'desc' in null else desc.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), B, C, OH, OW, pad, int(f32),
                               p(None if 'out' in null else out), geom.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)) if want_geom else None)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    return st, got, geom, bool((got == fill).all()) and bool((geom == -77).all())


@pytest.fixture(scope='module')
def small():
    """The seven cases of the table as one ragged batch at odd byte offsets, and their float64 restatement for both pad bytes, computed once."""
    images = F.kat_images()[:4] + F.kat_images()[4:5]      # the 12x18 frame
    buf12, desc12 = F.pack(images)
    images24 = F.kat_images()[5:]
    buf24, desc24 = F.pack(images24)
    assert (desc12[:, 0] % 2 == 1).all() and (desc24[:, 0] % 2 == 1).all()
    ref = {(hw, pad): F.fit_batch(ims, hw[0], hw[1], pad) for hw, ims in (((12, 18), images), ((24, 36), images24)) for pad in (0, 114)}
    return {(12, 18): (buf12, desc12), (24, 36): (buf24, desc24)}, ref


@pytest.mark.parametrize('pad', (0, 114))
@pytest.mark.parametrize('f32', (False, True), ids=('u8', 'f32'))
def test_small_cases_bit_for_bit(eng, small, pad, f32):
    """The table's cases, each frame one ragged call at odd byte offsets: bytes equal fit_ref's, floats equal byte / float32(255), geom the table."""
    packed, ref = small
    for hw, kat in (((12, 18), F.GEOMETRY_KAT[:5]), ((24, 36), F.GEOMETRY_KAT[5:])):
        buf, desc = packed[hw]
        want, wgeom = ref[(hw, pad)]
        st, got, geom, _ = _call(eng, buf, desc, hw[0], hw[1], pad=pad, f32=f32)
        assert st == 0, _lib.last_error()
        assert_array_equal(geom, np.array([k[2] for k in kat], np.int32))
        assert_array_equal(geom, wgeom)
        if f32:
            assert got.dtype == np.float32
            assert_array_equal(got.view(np.uint32), F.as_f32(want).view(np.uint32))
        else:
            assert_array_equal(got, want)


@pytest.mark.parametrize('pad', (0, 114))
def test_seven_ragged_in_one_call(eng, pad):
    """All seven images as ONE ragged call, B = 7, odd offsets.  A call has one frame, so this one is 24x36: the table's last two cases keep their
    rectangles, the first five land where fit_ref says.  The source bytes around the images (0xEE fillers) never show."""
    images = F.kat_images()
    buf, desc = F.pack(images)
    want, wgeom = F.fit_batch(images, 24, 36, pad)
    for f32 in (False, True):
        st, got, geom, _ = _call(eng, buf, desc, 24, 36, pad=pad, f32=f32)
        assert st == 0, _lib.last_error()
        assert_array_equal(geom, wgeom)
        assert_array_equal(got.view(np.uint32) if f32 else got, F.as_f32(want).view(np.uint32) if f32 else want)
    assert_array_equal(wgeom[5:], np.array([k[2] for k in F.GEOMETRY_KAT[5:]], np.int32))


@pytest.fixture(scope='module')
def full_frame():
    rs = np.random.RandomState(11)
    images = [rs.randint(0, 256, (211, 317, 3)).astype(np.uint8), rs.randint(0, 256, (1000, 700, 3)).astype(np.uint8)]
    images.append(images[0])
    return images, F.fit_batch(images, 480, 720, 0)


def test_full_frame_cases(eng, full_frame):
    """An output frame wider than any strip (23 strips of 32 columns): an enlargement with bars top and bottom, a portrait reduction of 2.08
    with bars left and right, and the first image again at another offset: equal outputs for equal images."""
    images, (want, wgeom) = full_frame
    buf, desc = F.pack(images)
    st, got, geom, _ = _call(eng, buf, desc, 480, 720)
    assert st == 0, _lib.last_error()
    assert_array_equal(geom, wgeom)
    assert geom.tolist()[:2] == [[0, 0, 479, 720], [0, 192, 480, 336]]
    assert_array_equal(got, want)
    assert_array_equal(got[0], got[2])


def test_engine_fit_images(eng, full_frame):
    """Engine.fit_images: host arrays and device tensors mixed, the float output, an out tensor, geom with the source sizes; bad inputs."""
    images, (want, wgeom) = full_frame
    mixed = [images[0], _dev(images[1]), torch.from_numpy(images[2])]
    x, geom = eng.fit_images(mixed)
    xf, _ = eng.fit_images(mixed, dtype=torch.float32)
    out = torch.empty((3, 480, 720, 3), dtype=torch.uint8, device='cuda:0')
    xo, _ = eng.fit_images(mixed, pad=9, out=out)
    torch.cuda.synchronize()
    assert x.dtype == torch.uint8 and tuple(x.shape) == (3, 480, 720, 3) and xo is out
    assert_array_equal(x.cpu().numpy(), want)
    assert_array_equal(xf.cpu().numpy().view(np.uint32), F.as_f32(want).view(np.uint32))
    assert geom.dtype == np.int32
    assert_array_equal(geom, np.concatenate([wgeom, np.array([im.shape[:2] for im in images], np.int32)], axis=1))
    assert int(out[0, 479, 0, 0]) == 9 and int(out[1, 0, 0, 0]) == 9
    with pytest.raises(ValueError):
        eng.fit_images([])
    with pytest.raises(TypeError):
        eng.fit_images([images[0].astype(np.float32)])
    with pytest.raises(ValueError):
        eng.fit_images([images[0][..., 0]])
    with pytest.raises(ValueError):
        eng.fit_images([images[0][..., :2]])
    with pytest.raises(TypeError):
        eng.fit_images(mixed, dtype=torch.float16)
    with pytest.raises(TypeError):
        eng.fit_images(['a.png'])


def test_more_images_than_one_launch(eng):
    """70 images take two launches (64 travel in one launch's arguments): the same small image everywhere gives the same frame everywhere."""
    images = F.kat_images()
    many = [images[i % 7] for i in range(70)]
    x, geom = eng.fit_images(many, out_hw=(24, 36), pad=3)
    torch.cuda.synchronize()
    want, _ = F.fit_batch(images, 24, 36, 3)
    got = x.cpu().numpy()
    for i in range(70):
        assert_array_equal(got[i], want[i % 7], err_msg=str(i))


def test_reduction_limit(eng):
    """(1, 576) -> 12x18 is a reduction of exactly 32 and is accepted; (1, 595) -> 12x18 (cw = 18: 595 > 576) is JCM_ERR_ARG."""
    rs = np.random.RandomState(5)
    img = rs.randint(0, 256, (1, 576, 3)).astype(np.uint8)
    buf, desc = F.pack([img])
    st, got, geom, _ = _call(eng, buf, desc, 12, 18, pad=1)
    assert st == 0, _lib.last_error()
    want, wgeom = F.fit_batch([img], 12, 18, 1)
    assert_array_equal(geom, wgeom)
    assert_array_equal(got, want)
    buf, desc = F.pack([rs.randint(0, 256, (1, 595, 3)).astype(np.uint8)])
    st, _, _, untouched = _call(eng, buf, desc, 12, 18)
    assert st == ERR_ARG and untouched and 'reduction' in _lib.last_error()


def test_argument_errors_leave_the_outputs_untouched(eng):
    """Every error case of jcm.h, built from valid arguments with one thing wrong; no pointer the kernel would fault on is ever passed."""
    images = F.kat_images()[:2]
    buf, desc = F.pack(images)
    ok = dict(OH=12, OW=18)
    st, _, _, untouched = _call(eng, buf, desc, **ok)
    assert st == 0 and not untouched

    def bad_desc(i, j, v):
        d = desc.copy()
        d[i, j] = v
        return d
    cases = [dict(null=('src',)), dict(null=('desc',)), dict(null=('out',)), dict(B=0), dict(B=-1), dict(C=0), dict(C=5), dict(OH=0), dict(OH=4097),
             dict(OW=0), dict(OW=4097), dict(pad=-1), dict(pad=256),
             dict(desc=bad_desc(1, 1, 0)), dict(desc=bad_desc(1, 1, 16385)), dict(desc=bad_desc(0, 2, 0)), dict(desc=bad_desc(0, 2, 16385)),
             dict(desc=bad_desc(0, 0, -1)), dict(desc=bad_desc(1, 0, len(buf) - images[1].size + 1)), dict(src_bytes=len(buf) - 1),
             dict(desc=bad_desc(1, 0, 2 ** 40)),
             dict(desc=np.array([(0, 3, 200)], np.int64), OH=4, OW=4)]      # 200 > 32 * 4
    for kw in cases:
        args = dict(ok, desc=desc)
        args.update(kw)
        d = args.pop('desc')
        st, _, _, untouched = _call(eng, buf, d, args.pop('OH'), args.pop('OW'), **args)
        assert st == ERR_ARG and untouched, kw
        assert 'fit_images' in _lib.last_error(), kw
    # B * OH * OW * C >= 2^31 is refused before anything is read or written: out and src here are far smaller than such a call would need
    from joint_cnn_mrf_amd.engine import Engine
    p = Engine._p
    src, out = _dev(buf), torch.full((16,), 0x5A, dtype=torch.uint8, device='cuda:0')
    big = np.tile(desc[:1], (43, 1))
    st = eng._lib.jcm_fit_images(eng._h, p(src), len(buf), big.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), 43, 3, 4096, 4096, 0, 0, p(out), None)
    torch.cuda.synchronize()
    assert st == ERR_ARG and bool((out == 0x5A).all()) and '2^31' in _lib.last_error()
    # out overlapping src
    st = eng._lib.jcm_fit_images(eng._h, p(src), len(buf), desc.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), 1, 3, 1, 1, 0, 0, p(src), None)
    assert st == ERR_ARG and 'overlaps' in _lib.last_error()
    # a null geom is accepted
    st, got, geom, _ = _call(eng, buf, desc, 12, 18, want_geom=False)
    assert st == 0 and (geom == -77).all()
    assert_array_equal(got, F.fit_batch(images, 12, 18, 0)[0])
