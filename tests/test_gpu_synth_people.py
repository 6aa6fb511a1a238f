"""Rendered people on the GPU (csrc/synth_people.hip): jcm_synth_people and Engine.synth_people against the numpy restatement
tests/synth_people_ref.py (pinned by tests/test_synth_people_cpu.py), every byte and with no tolerance, at the smallest shapes where the kernel can
go wrong; every argument error; dataset.render_people and DeviceDataset.rerender_people."""
import ctypes
import os

import numpy as np
import pytest
import torch
from numpy.testing import assert_array_equal

import synth_people_ref as R
import joint_cnn_mrf_amd  # noqa: F401
from joint_cnn_mrf_amd import data, dataset, synth

pytestmark = pytest.mark.gpu
ERR_ARG = 1
FILL = 0x5A
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope='module')
def eng():
    """A handle without parameters: the renderer needs none."""
    from joint_cnn_mrf_amd.engine import Engine
    e = Engine(device=0)
    yield e
    e.close()


@pytest.fixture(scope='module')
def poses():
    return np.load(os.path.join(HERE, 'golden', 'flic_train_xy.npy'))


def _scene(rs, H, W, n, first=0, a=None):
    """A random record and n primitives for an H x W frame: capsules and quadrilaterals of every size, centred up to half a frame OUTSIDE the
    image, so that some cross each edge and some miss the image altogether."""
    rec = R.record(seed=int(rs.randint(-2 ** 31, 2 ** 31 - 1)), c0=rs.randint(0, 256, 3), c1=rs.randint(0, 256, 3), amp=rs.randint(0, 120, 4),
                   a=int(rs.randint(1, 9)) if a is None else a, n=n, first=first)
    prims = []
    for _ in range(n):
        cy, cx = rs.uniform(-0.5, 1.5) * H * 16, rs.uniform(-0.5, 1.5) * W * 16
        ext = rs.uniform(0.02, 0.6) * max(H, W) * 16
        kw = dict(col=rs.randint(0, 256, 3), tamp=int(rs.randint(0, 80)), ts=int(rs.randint(0, 4)), tseed=int(rs.randint(0, 2 ** 31 - 1)))
        if rs.random_sample() < 0.5:
            d = rs.uniform(-1, 1, 2) * ext
            prims.append(R.capsule(int(cy - d[0]), int(cx - d[1]), int(cy + d[0]), int(cx + d[1]), int(rs.uniform(0, 0.3) * ext), **kw))
        else:      # a convex quadrilateral: four points of an ellipse in angular order (either winding)
            ang = np.sort(rs.uniform(0, 2 * np.pi, 4))[::int(rs.choice([-1, 1]))]
            ry, rx = rs.uniform(0.2, 1, 2) * ext
            prims.append(R.quad([(int(cy + ry * np.sin(t)), int(cx + rx * np.cos(t))) for t in ang], **kw))
    return rec, np.array(prims, np.int32).reshape(-1, R.PRIM_INTS)


def _batch(rs, H, W, counts, **kw):
    recs, prims, first = [], [], 0
    for n in counts:
        r, p = _scene(rs, H, W, n, first, **kw)
        first += n
        recs.append(r)
        prims.append(p)
    return np.stack(recs), np.concatenate(prims)


def _run(e, recs, prims, H, W, dtype=torch.uint8, offset=0):
    """Engine.synth_people into a pre-filled buffer with a guard on either side of the output (at `offset` bytes): -> host array; the guards hold."""
    n = recs.shape[0] * H * W * 3
    es = 1 if dtype == torch.uint8 else 4
    buf = torch.full((offset + n * es + 64,), FILL, dtype=torch.uint8, device='cuda:0')
    out = buf[offset:offset + n * es].view(dtype).view(recs.shape[0], H, W, 3)
    got = e.synth_people(recs, prims, H, W, out=out, dtype=dtype)
    assert got.data_ptr() == out.data_ptr()
    host = buf.cpu().numpy()
    assert (host[:offset] == FILL).all() and (host[offset + n * es:] == FILL).all(), 'bytes outside the output were written'
    return got.cpu().numpy()


@pytest.mark.parametrize('H,W,counts,offset', [
    (37, 53, (5,), 0),            # smaller than a tile row, an odd byte count, lattice cells larger than the image; every octave's lattice in LDS
    (37, 53, (3, 0), 5),          # an output at a byte offset that is no multiple of 16, and a second image behind an odd byte count
    (70, 131, (9,), 0),           # 9170 pixels: the second tile starts mid-row; the first spans rows
    (70, 131, (0, 1, 64), 3),     # B = 3: no primitive, one, the most; three seeds
    (1, 9000, (4,), 1),           # one row of two tiles: culling by columns
    (3000, 3, (4,), 0),           # a tile of 2731 rows
])
def test_every_byte_equals_the_restatement(eng, H, W, counts, offset):
    recs, prims = _batch(np.random.RandomState(H * 1000 + W + len(counts)), H, W, counts)
    assert_array_equal(_run(eng, recs, prims, H, W, offset=offset), R.render_batch(recs, prims, H, W))


def test_full_frame_and_a_primitive_over_many_tiles(eng):
    """One image of 480 x 720 (43 tiles; the one-pixel octave is hashed per pixel here, not from LDS) with a capsule and a quadrilateral whose
    boxes cover most of the frame, a quadrilateral with three collinear vertices (a triangle), one with all four on a line, and random ones."""
    H, W = 480, 720
    rs = np.random.RandomState(7)
    rec, prims = _scene(rs, H, W, 12)
    big = [R.capsule(16 * 40, 16 * 30, 16 * 440, 16 * 690, 16 * 90, (200, 30, 40), 60, 3, 11),
           R.quad([(-16 * 50, 16 * 100), (16 * 20, 16 * 800), (16 * 500, 16 * 600), (16 * 470, -16 * 30)], (10, 220, 90), 40, 2, 12),
           R.quad([(16 * 100, 16 * 100), (16 * 100, 16 * 200), (16 * 100, 16 * 300), (16 * 250, 16 * 200)], (250, 250, 0), 0, 0, 0),
           R.quad([(16 * 300, 16 * 100), (16 * 310, 16 * 200), (16 * 320, 16 * 300), (16 * 330, 16 * 400)], (0, 0, 0), 0, 0, 0)]
    prims = np.concatenate([np.array(big, np.int32), prims])
    rec[16] = prims.shape[0]
    got = _run(eng, rec[None], prims, H, W)
    assert_array_equal(got, R.render_batch(rec[None], prims, H, W))


def test_without_sensor_noise_and_without_octaves(eng):
    H, W = 37, 53
    recs, prims = _batch(np.random.RandomState(3), H, W, (6, 6), a=0)
    recs[1, 7:11] = 0
    assert_array_equal(_run(eng, recs, prims, H, W), R.render_batch(recs, prims, H, W))


@pytest.mark.parametrize('H,W,offset', [(37, 53, 0), (70, 131, 4), (70, 131, 12)])
def test_float_output_is_the_byte_over_255(eng, H, W, offset):
    recs, prims = _batch(np.random.RandomState(H + offset), H, W, (7, 2))
    u8 = R.render_batch(recs, prims, H, W)
    got = _run(eng, recs, prims, H, W, dtype=torch.float32, offset=offset)
    assert_array_equal(got.view(np.uint32), (u8.astype(np.float32) / np.float32(255)).view(np.uint32))


def _status(e, recs, prims, H, W, B=None, NP=None, null=()):
    """jcm_synth_people at the C ABI with a pre-filled 64-byte out, which an error must leave untouched -> the error text."""
    from joint_cnn_mrf_amd import _lib
    i32 = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))      # noqa: E731
    recs, prims = np.ascontiguousarray(recs, np.int32).reshape(-1, R.REC_INTS), np.ascontiguousarray(prims, np.int32).reshape(-1, R.PRIM_INTS)
    out = torch.full((64,), FILL, dtype=torch.uint8, device='cuda:0')
    st = e._lib.jcm_synth_people(e._h, None if 'records' in null else i32(recs), recs.shape[0] if B is None else B,
                                 i32(prims) if prims.shape[0] and 'prims' not in null else None, prims.shape[0] if NP is None else NP, H, W, 0,
                                 None if 'out' in null else ctypes.c_void_p(out.data_ptr()))
    assert st == ERR_ARG
    assert (out.cpu().numpy() == FILL).all()
    return _lib.last_error()


def test_each_error_text(eng):
    ok = R.record(n=1)
    cap = R.capsule(0, 0, 16, 16, 8, (1, 2, 3))

    def rec(**kw):
        r = ok.copy()
        for k, v in kw.items():
            r[int(k[1:])] = v
        return r

    def prim(**kw):
        p = cap.copy()
        for k, v in kw.items():
            p[int(k[1:])] = v
        return p
    cases = [
        (dict(recs=ok, prims=cap, null=('records',)), 'null pointer'),
        (dict(recs=ok, prims=cap, null=('out',)), 'null pointer'),
        (dict(recs=ok, prims=cap, NP=1, null=('prims',)), 'prims with NP > 0'),
        (dict(recs=ok, prims=cap, NP=-1), 'NP >= 0'),
        (dict(recs=ok, prims=cap, B=0), 'outside 1..65535'),
        (dict(recs=ok, prims=cap, H=0), 'H and W >= 1'),
        (dict(recs=ok, prims=cap, H=65536, W=32768), 'over the int32 range'),
        (dict(recs=rec(_16=65), prims=cap), 'n = 65 primitives outside 0..64'),
        (dict(recs=rec(_16=-1), prims=cap), 'n = -1 primitives outside 0..64'),
        (dict(recs=rec(_17=1), prims=cap), 'do not lie inside the 1 of prims'),
        (dict(recs=rec(_17=-1), prims=cap), 'do not lie inside'),
        (dict(recs=rec(_2=256), prims=cap), 'background colour 256 outside 0..255'),
        (dict(recs=rec(_8=256), prims=cap), 'octave amplitude 256 outside 0..255'),
        (dict(recs=rec(_9=-1), prims=cap), 'octave amplitude -1 outside 0..255'),
        (dict(recs=rec(_12=9), prims=cap), 'octave shift 9 outside 0..8'),
        (dict(recs=rec(_13=-1), prims=cap), 'octave shift -1 outside 0..8'),
        (dict(recs=rec(_15=256), prims=cap), 'sensor-noise amplitude 256 outside 0..255'),
        (dict(recs=ok, prims=prim(_0=2)), 'kind 2 is neither'),
        (dict(recs=ok, prims=prim(_5=-1)), 'r = -1 outside 0..2^16'),
        (dict(recs=ok, prims=prim(_3=(1 << 20) + 1)), 'outside +-2^20'),
        (dict(recs=ok, prims=prim(_10=300)), 'colour 300 outside 0..255'),
        (dict(recs=ok, prims=prim(_12=256)), 'texture amplitude 256 outside 0..255'),
        (dict(recs=ok, prims=prim(_13=9)), 'texture shift 9 outside 0..8'),
    ]
    for kw, text in cases:
        kw = dict(dict(H=8, W=8), **kw)
        msg = _status(eng, **kw)
        assert msg.startswith('synth_people: ') and text in msg, (kw, msg)
    with pytest.raises(ValueError, match=r'records must be an integer array \[\.,20\]'):
        eng.synth_people(np.zeros((1, 19), np.int32), cap[None], 8, 8)
    with pytest.raises(ValueError, match=r'out must be \[1,8,8,3\]'):
        eng.synth_people(ok[None], cap[None], 8, 8, out=torch.zeros((1, 8, 9, 3), dtype=torch.uint8, device='cuda:0'))
    with pytest.raises(RuntimeError, match='n = 65 primitives'):
        eng.synth_people(rec(_16=65)[None], cap[None], 8, 8)


def test_render_people_is_people_batch_plus_the_restatement(eng, poses):
    idx = [5, 900, 17, 3000, 42, 7, 1234, 2]
    x, y, cells = dataset.render_people(eng, poses, idx, seed=9, batch=3)      # batches of 3, 3 and 2 from ONE generator
    rng = np.random.RandomState(9)
    parts = [synth.people_batch(rng, poses, idx[lo:lo + 3]) for lo in (0, 3, 6)]
    assert x.dtype == np.uint8 and x.shape == (8, 480, 720, 3) and y.dtype == np.float32 and y.shape == (8, 60, 90, 10) and cells.shape == (8, 10, 2)
    assert_array_equal(x, np.concatenate([R.render_batch(p[0], p[1], 480, 720) for p in parts]))
    assert_array_equal(y, np.concatenate([p[4] for p in parts]))
    assert_array_equal(cells, np.concatenate([p[3] for p in parts]))
    xf, yf, _ = dataset.render_people(eng, poses, idx[:2], seed=9, image_dtype='float32', batch=3)
    assert_array_equal(xf.view(np.uint32), (x[:2].astype(np.float32) / np.float32(255)).view(np.uint32))
    assert_array_equal(yf, y[:2])


def test_rerender_people_draws_again_in_place(eng, poses):
    idx = [11, 2000, 333, 64]
    x, y, cells = dataset.render_people(eng, poses, idx, seed=1)
    ds = dataset.DeviceDataset(x, y, device=0, image_dtype='uint8', cells=cells)
    ptr = ds.x.data_ptr()
    assert ds.rerender_people(eng, poses, idx, seed=2, batch=3) is ds
    x2, y2, cells2 = dataset.render_people(eng, poses, idx, seed=2, batch=3)
    assert ds.x.data_ptr() == ptr
    assert_array_equal(ds.x.cpu().numpy(), x2)
    assert (x2 != x).any()
    assert_array_equal(ds.y.cpu().numpy(), y2)
    assert_array_equal(ds.cells.cpu().numpy(), cells2)
    # the same poses: with the similarity switched off (scale 1, no shift; the mirror remains) every scene's cells are those of its pose or of its mirror image
    ds.rerender_people(eng, poses, idx, seed=3, scale=(1.0, 1.0), shift=0.0)
    plain = data.joint_cells(poses[idx])
    mirrored = data.joint_cells(np.stack([synth._mirror(p, 720) for p in poses[idx]]))
    got = ds.cells.cpu().numpy()
    for i in range(len(idx)):
        assert (got[i] == plain[i]).all() or (got[i] == mirrored[i]).all(), i
    assert_array_equal(ds.y.cpu().numpy(), data.target_heat_maps(got))
    with pytest.raises(ValueError, match='3 indices for a set of 4'):
        ds.rerender_people(eng, poses, idx[:3], seed=2)
