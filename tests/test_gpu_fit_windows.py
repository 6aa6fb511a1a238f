"""The fit of windows of images on the GPU (csrc/fit.hip): jcm_fit_windows against the float64 restatement
tests/fit_windows_ref.py -- the padded crop, then tests/fit_ref.py's fit -- bit for bit, for byte and float outputs: every placement of a window
against its image's edges, every filter shape, the batching, the argument errors (each of which must leave pre-filled outputs untouched) and
Engine.fit_windows.  No tolerance anywhere: bytes are equal or the test fails."""
import ctypes

import numpy as np
import pytest
import torch
from numpy.testing import assert_array_equal

import fit_ref as F
import fit_windows_ref as W
import joint_cnn_mrf_amd  # noqa: F401
from joint_cnn_mrf_amd import _lib

pytestmark = pytest.mark.gpu
ERR_ARG = 1
FRAMES = ((12, 18), (24, 36))


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), device='cuda:0')


def _i64(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))


def _i32(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))


@pytest.fixture(scope='module')
def eng():
    """A handle without parameters: the fit needs none."""
    from joint_cnn_mrf_amd.engine import Engine
    e = Engine(device=0)
    yield e
    e.close()


def _call(e, buf, desc, OH, OW, pad=0, f32=False, C=3, NW=None, src_bytes=None, fill=0x5A, null=(), want_geom=True, src=None):
    """jcm_fit_windows at the C ABI on a packed buffer -> (status, out (host), geom (host), were the pre-filled out and geom left untouched?)."""
    from joint_cnn_mrf_amd.engine import Engine
    p = Engine._p
    NW = len(desc) if NW is None else NW
    n = max(len(desc), 1)
    src = _dev(buf) if src is None else src
    out = torch.full((n, OH, OW, C), fill, dtype=torch.float32 if f32 else torch.uint8, device='cuda:0')
    geom = np.full((n, 4), -77, np.int32)
    desc = np.ascontiguousarray(desc, np.int64)
    torch.cuda.synchronize()
    st = e._lib.jcm_fit_windows(e._h, p(None if 'src' in null else src), len(buf) if src_bytes is None else src_bytes,
                                None if 'desc' in null else _i64(desc), NW, C, OH, OW, pad, int(f32), p(None if 'out' in null else out),
                                _i32(geom) if want_geom else None)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    return st, got, geom, bool((got == fill).all()) and bool((geom == -77).all())


def _same(got, want, f32):
    if f32:
        assert got.dtype == np.float32
        assert_array_equal(got.view(np.uint32), F.as_f32(want).view(np.uint32))
    else:
        assert_array_equal(got, want)


# (name, (image index, y0, x0, h, w)); image 0 is 40 x 60, image 1 is 70 x 90, image 2 is 210 x 210
PLACEMENT = (
    ('inside', (0, 5, 7, 20, 30)), ('inside odd', (0, 11, 13, 9, 17)),
    ('flush top', (0, 0, 10, 15, 20)), ('flush bottom', (0, 25, 10, 15, 20)), ('flush left', (0, 10, 0, 15, 20)), ('flush right', (0, 10, 40, 15, 20)),
    ('across top', (0, -6, 10, 15, 20)), ('across bottom', (0, 31, 10, 15, 20)), ('across left', (0, 10, -7, 15, 20)),
    ('across right', (0, 10, 47, 15, 20)),
    ('corner top left', (0, -5, -6, 15, 20)), ('corner top right', (0, -5, 46, 15, 20)), ('corner bottom left', (0, 30, -6, 15, 20)),
    ('corner bottom right', (0, 30, 46, 15, 20)),
    ('around the image', (0, -4, -5, 48, 70)), ('whole image', (0, 0, 0, 40, 60)),
    ('1 x 1', (0, 3, 4, 1, 1)), ('1 x 1 last pixel', (0, 39, 59, 1, 1)), ('one pixel wide', (0, 2, 59, 30, 1)), ('one pixel high', (0, 39, -3, 1, 30)),
    ('one pixel of the image in a corner', (1, 69, 89, 9, 14)),
)
SHAPES = (
    ('enlarging 5 x 7', (1, 33, 41, 5, 7)), ('enlarging across the corner', (1, -2, -3, 5, 7)),
    ('reducing 37 x 53', (1, 20, 30, 37, 53)), ('reducing 37 x 53 across the right edge', (1, 9, 61, 37, 53)),
    ('200 rows of a 3-wide strip', (2, 7, 101, 200, 3)), ('200 rows across the bottom', (2, 40, 208, 200, 3)),
    ('3 rows of 200 columns', (2, 99, -11, 3, 200)), ('150 x 31', (2, -9, 190, 150, 31)), ('150 x 31 inside', (2, 33, 77, 150, 31)),
) + tuple(('left edge at column %d' % x0, (0, 3, x0, 12, 18)) for x0 in (1, 2, 3, 4))
CASES = PLACEMENT + SHAPES


@pytest.fixture(scope='module')
def sources():
    rs = np.random.RandomState(17)
    images = [rs.randint(0, 256, s + (3,)).astype(np.uint8) for s in ((40, 60), (70, 90), (210, 210))]
    buf, desc = F.pack(images)
    assert (desc[:, 0] % 2 == 1).all()
    return images, buf, desc


@pytest.fixture(scope='module')
def placed(sources):
    """The restatement of every case for both frames and both pad bytes, computed once."""
    images = sources[0]
    wins = np.array([w for _, w in CASES], np.int64)
    return wins, {(hw, pad): W.fit_windows(images, wins, hw[0], hw[1], pad) for hw in FRAMES for pad in (0, 114)}


def test_the_cases_cover_every_alignment(sources):
    """The four left-edge windows start at the four byte alignments mod 4 (an odd image offset, three bytes a pixel)."""
    _, _, desc = sources
    assert sorted(int(desc[0, 0] + (3 * 60 + x0) * 3) % 4 for x0 in (1, 2, 3, 4)) == [0, 1, 2, 3]


@pytest.mark.parametrize('pad', (0, 114))
@pytest.mark.parametrize('f32', (False, True), ids=('u8', 'f32'))
@pytest.mark.parametrize('hw', FRAMES, ids=('12x18', '24x36'))
def test_placements_and_filter_shapes(eng, sources, placed, hw, f32, pad):
    """Every placement and every filter shape as ONE ragged call: more than six windows of image 0 beside windows of images 1 and 2."""
    _, buf, desc = sources
    wins, ref = placed
    want, wgeom = ref[(hw, pad)]
    st, got, geom, _ = _call(eng, buf, W.desc7(desc, wins), hw[0], hw[1], pad=pad, f32=f32)
    assert st == 0, _lib.last_error()
    assert_array_equal(geom, wgeom)
    for i, (name, _) in enumerate(CASES):
        if f32:
            assert_array_equal(got[i].view(np.uint32), F.as_f32(want[i]).view(np.uint32), err_msg=name)
        else:
            assert_array_equal(got[i], want[i], err_msg=name)


def test_padded_samples_take_part_in_the_filter(placed):
    """The restatement itself: a window across an edge differs between pad 0 and pad 114 inside its content rectangle, not only in the bars."""
    wins, ref = placed
    i = [n for n, _ in CASES].index('across left')
    (a, g), (b, _) = ref[((24, 36), 0)], ref[((24, 36), 114)]
    y0, x0, ch, cw = g[i]
    assert (a[i, y0:y0 + ch, x0:x0 + cw] != b[i, y0:y0 + ch, x0:x0 + cw]).any()


@pytest.mark.parametrize('C', (1, 3, 4))
def test_channel_counts(eng, C):
    rs = np.random.RandomState(23 + C)
    images = [rs.randint(0, 256, (19, 27, C)).astype(np.uint8), rs.randint(0, 256, (50, 31, C)).astype(np.uint8)]
    buf, desc = F.pack(images)
    wins = np.array([(0, 2, 3, 10, 15), (0, -3, 20, 12, 18), (1, 45, -5, 12, 18), (1, -1, -1, 52, 33), (0, 6, 5, 5, 7), (1, 0, 1, 50, 29)], np.int64)
    for pad in (0, 114):
        want, wgeom = W.fit_windows(images, wins, 12, 18, pad)
        for f32 in (False, True):
            st, got, geom, _ = _call(eng, buf, W.desc7(desc, wins), 12, 18, pad=pad, f32=f32, C=C)
            assert st == 0, _lib.last_error()
            assert_array_equal(geom, wgeom)
            _same(got, want, f32)


def test_more_windows_than_one_launch(eng, sources, placed):
    """150 windows take three launches (64 travel in one launch's arguments): the cases again, cycled."""
    _, buf, desc = sources
    wins, ref = placed
    want, wgeom = ref[((24, 36), 114)]
    idx = np.arange(150) % len(wins)
    st, got, geom, _ = _call(eng, buf, W.desc7(desc, wins[idx]), 24, 36, pad=114)
    assert st == 0, _lib.last_error()
    assert_array_equal(geom, wgeom[idx])
    assert_array_equal(got, want[idx])


@pytest.mark.parametrize('pad', (0, 114))
@pytest.mark.parametrize('f32', (False, True), ids=('u8', 'f32'))
def test_whole_image_windows_equal_fit_images(eng, pad, f32):
    """The seven images of fit_ref's table, each as the window (0, 0, h, w): the bits and the geometry of jcm_fit_images in the same process."""
    from joint_cnn_mrf_amd.engine import Engine
    p = Engine._p
    images = F.kat_images()
    buf, desc = F.pack(images)
    wins = np.array([(i, 0, 0, im.shape[0], im.shape[1]) for i, im in enumerate(images)], np.int64)
    st, got, geom, _ = _call(eng, buf, W.desc7(desc, wins), 24, 36, pad=pad, f32=f32)
    assert st == 0, _lib.last_error()
    src = _dev(buf)
    out = torch.full((7, 24, 36, 3), 0x5A, dtype=torch.float32 if f32 else torch.uint8, device='cuda:0')
    g2 = np.full((7, 4), -77, np.int32)
    assert eng._lib.jcm_fit_images(eng._h, p(src), len(buf), _i64(desc), 7, 3, 24, 36, pad, int(f32), p(out), _i32(g2)) == 0, _lib.last_error()
    torch.cuda.synchronize()
    assert_array_equal(geom, g2)
    assert_array_equal(got.view(np.uint32) if f32 else got, out.cpu().numpy().view(np.uint32) if f32 else out.cpu().numpy())
    _same(got, F.fit_batch(images, 24, 36, pad)[0], f32)


def test_full_frame_window_across_the_right_edge(eng):
    """A 500 x 700 window across the right edge of a 1080 x 1920 photo into the tower's frame: 23 strips, a reduction, pad columns on the right."""
    rs = np.random.RandomState(29)
    img = rs.randint(0, 256, (1080, 1920, 3), dtype=np.uint8)
    buf, desc = F.pack([img])
    win = (0, 301, 1501, 500, 700)
    want, wgeom = W.fit_windows([img], [win], 480, 720, 114)
    st, got, geom, _ = _call(eng, buf, W.desc7(desc, [win]), 480, 720, pad=114)
    assert st == 0, _lib.last_error()
    assert_array_equal(geom, wgeom)
    assert_array_equal(got, want)


def test_window_of_a_large_source(eng):
    """A 200 x 300 window at the far corner of a 4000 x 6000 source (72 MB; byte offsets beyond 2^26): the restatement sees the pre-cropped window
    only.  Two windows: one inside, one across the bottom right corner."""
    rs = np.random.RandomState(31)
    img = rs.randint(0, 256, (4000, 6000, 3), dtype=np.uint8)
    lead = np.full(1, 0xEE, np.uint8)
    src = torch.cat([torch.from_numpy(lead), torch.from_numpy(img.reshape(-1))]).to('cuda:0')
    nbytes = 1 + img.size
    wins = [(0, 3701, 5603, 200, 300), (0, 3850, 5800, 200, 300)]
    desc = np.array([(1, 4000, 6000) + w[1:] for w in wins], np.int64)
    crops = [W.window(img, *w[1:], pad=114) for w in wins]
    want, wgeom = F.fit_batch(crops, 480, 720, 114)
    st, got, geom, _ = _call(eng, np.empty(nbytes, np.uint8)[:0], desc, 480, 720, pad=114, src=src, src_bytes=nbytes)
    assert st == 0, _lib.last_error()
    assert_array_equal(geom, wgeom)
    assert_array_equal(got, want)


def test_reduction_limit(eng):
    """A 1 x 576 window into 12 x 18 is a reduction of exactly 32 and is accepted; 1 x 595 (cw = 18: 595 > 576) is JCM_ERR_ARG."""
    rs = np.random.RandomState(5)
    img = rs.randint(0, 256, (1, 600, 3)).astype(np.uint8)
    buf, desc = F.pack([img])
    win = (0, 0, -10, 1, 576)
    st, got, geom, _ = _call(eng, buf, W.desc7(desc, [win]), 12, 18, pad=1)
    assert st == 0, _lib.last_error()
    want, wgeom = W.fit_windows([img], [win], 12, 18, 1)
    assert_array_equal(geom, wgeom)
    assert_array_equal(got, want)
    st, _, _, untouched = _call(eng, buf, W.desc7(desc, [(0, 0, 0, 1, 595)]), 12, 18)
    assert st == ERR_ARG and untouched and 'reduction' in _lib.last_error()


def test_argument_errors_leave_the_outputs_untouched(eng, sources):
    """Every error case of jcm.h, built from valid arguments with one thing wrong; no pointer the kernel would fault on is ever passed."""
    images, buf, desc = sources
    good = W.desc7(desc, [(0, -5, -6, 15, 20), (1, 20, 30, 37, 53)])
    ok = dict(OH=12, OW=18)
    st, _, _, untouched = _call(eng, buf, good, **ok)
    assert st == 0 and not untouched

    def bad(i, j, v):
        d = good.copy()
        d[i, j] = v
        return d
    cases = [dict(null=('src',)), dict(null=('desc',)), dict(null=('out',)), dict(NW=0), dict(NW=-1), dict(C=0), dict(C=5), dict(OH=0), dict(OH=4097),
             dict(OW=0), dict(OW=4097), dict(pad=-1), dict(pad=256),
             # a window that shares no pixel with its 40 x 60 image: below, above, right, left -- by one row or column, and by far
             dict(desc=bad(0, 3, 40)), dict(desc=bad(0, 3, -15)), dict(desc=bad(0, 4, 60)), dict(desc=bad(0, 4, -20)),
             dict(desc=bad(0, 3, 2 ** 62)), dict(desc=bad(0, 4, -2 ** 62)),
             dict(desc=bad(0, 5, 0)), dict(desc=bad(1, 6, 0)), dict(desc=bad(0, 5, -3)),              # wh = 0, ww = 0
             dict(desc=bad(1, 6, 16385)), dict(desc=bad(1, 5, 16385)),
             dict(desc=bad(1, 6, 53 * 40)),                                                           # 2120 columns into 18: above 32
             dict(desc=bad(1, 1, 0)), dict(desc=bad(1, 2, 0)), dict(desc=bad(1, 1, 2 ** 24 + 1)),       # the image's own sides
             dict(desc=bad(0, 0, -1)), dict(desc=bad(1, 0, len(buf) - images[1].size + 1)), dict(src_bytes=int(good[1, 0]) + images[1].size - 1),
             dict(desc=bad(1, 0, 2 ** 40))]
    for kw in cases:
        args = dict(ok, desc=good)
        args.update(kw)
        d = args.pop('desc')
        st, _, _, untouched = _call(eng, buf, d, args.pop('OH'), args.pop('OW'), **args)
        assert st == ERR_ARG and untouched, kw
        assert 'fit_windows' in _lib.last_error(), kw
    st, _, _, _ = _call(eng, buf, bad(0, 3, 40), **ok)
    assert st == ERR_ARG and 'shares no pixel' in _lib.last_error()
    # NW * OH * OW * C >= 2^31 is refused before anything is read or written: out and src here are far smaller than such a call would need
    from joint_cnn_mrf_amd.engine import Engine
    p = Engine._p
    src, out = _dev(buf), torch.full((16,), 0x5A, dtype=torch.uint8, device='cuda:0')
    big = np.ascontiguousarray(np.tile(good[:1], (43, 1)))
    st = eng._lib.jcm_fit_windows(eng._h, p(src), len(buf), _i64(big), 43, 3, 4096, 4096, 0, 0, p(out), None)
    torch.cuda.synchronize()
    assert st == ERR_ARG and bool((out == 0x5A).all()) and '2^31' in _lib.last_error()
    # out overlapping src
    before = src.clone()
    st = eng._lib.jcm_fit_windows(eng._h, p(src), len(buf), _i64(good), 1, 3, 1, 1, 0, 0, p(src), None)
    torch.cuda.synchronize()
    assert st == ERR_ARG and 'overlaps' in _lib.last_error() and bool((src == before).all())
    # a null geom is accepted
    st, got, geom, _ = _call(eng, buf, good, 12, 18, want_geom=False)
    assert st == 0 and (geom == -77).all()
    assert_array_equal(got, W.fit_windows(images, [(0, -5, -6, 15, 20), (1, 20, 30, 37, 53)], 12, 18, 0)[0])


def test_engine_fit_windows(eng, sources, placed):
    """Engine.fit_windows: host arrays and device tensors mixed give the bits of the C call; the float output, an out tensor, geom with the
    window sizes; bad inputs."""
    images, buf, desc = sources
    wins, ref = placed
    want, wgeom = ref[((24, 36), 114)]
    mixed = [images[0], _dev(images[1]), torch.from_numpy(images[2])]
    x, geom = eng.fit_windows(mixed, wins, out_hw=(24, 36), pad=114)
    xf, _ = eng.fit_windows(mixed, wins.astype(np.int32), out_hw=(24, 36), pad=114, dtype=torch.float32)
    out = torch.empty((len(wins), 24, 36, 3), dtype=torch.uint8, device='cuda:0')
    xo, _ = eng.fit_windows(list(images), wins.tolist(), out_hw=(24, 36), pad=114, out=out)
    torch.cuda.synchronize()
    st, got, _, _ = _call(eng, buf, W.desc7(desc, wins), 24, 36, pad=114)
    assert st == 0, _lib.last_error()
    assert x.dtype == torch.uint8 and tuple(x.shape) == (len(wins), 24, 36, 3) and xo is out
    assert_array_equal(x.cpu().numpy(), got)
    assert_array_equal(xo.cpu().numpy(), got)
    assert_array_equal(got, want)
    assert_array_equal(xf.cpu().numpy().view(np.uint32), F.as_f32(want).view(np.uint32))
    assert geom.dtype == np.int32
    assert_array_equal(geom, np.concatenate([wgeom, wins[:, 3:].astype(np.int32)], axis=1))
    with pytest.raises(ValueError):
        eng.fit_windows([], wins)
    with pytest.raises(TypeError):
        eng.fit_windows([images[0].astype(np.float32)], [(0, 0, 0, 4, 4)])
    with pytest.raises(ValueError):
        eng.fit_windows(mixed, [(3, 0, 0, 4, 4)])
    with pytest.raises(ValueError):
        eng.fit_windows(mixed, [(-1, 0, 0, 4, 4)])
    with pytest.raises(ValueError):
        eng.fit_windows(mixed, [(0, 0, 0, 4)])
    with pytest.raises(ValueError):
        eng.fit_windows(mixed, np.array([(0, 0, 0, 4.0, 4.0)]))
    with pytest.raises(TypeError):
        eng.fit_windows(mixed, wins, dtype=torch.float16)
    with pytest.raises(RuntimeError):
        eng.fit_windows(mixed, [(0, 40, 0, 4, 4)])      # disjoint: the library refuses it
