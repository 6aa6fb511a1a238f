"""The antialiased affine sample on the GPU (csrc/augment_affine.hip behind jcm_augment_affine_aa*) against its numpy restatement
tests/affine_aa_ref.py: images bit for bit, maps those of the plain entry; its indexed and byte forms, the argument contract, and its way through
Trainer, TowerTrainer and the command line.

The rows compared bit for bit leave the contrast factor at 1 (a brightness delta is there): with another factor the plain entry's own test
(tests/test_gpu_affine.py) holds the restatement's colour step to 1e-6, not to the bit, and the colour step is the plain entry's code.  A row with
factor 1.2 is held to that 1e-6 here too, and to the plain entry bit for bit where the widths are all 1.
Sizes: 16 x 24 (several work groups per image only at 40 x 56: 2240 pixels, 9 groups of 256, the last one partial); B = 17 takes two launches."""
import ctypes

import numpy as np
import pytest
import torch

import affine_aa_ref as A
import affine_ref as R
import joint_cnn_mrf_amd  # noqa: F401
from joint_cnn_mrf_amd import _lib, augmentation, synth

pytestmark = pytest.mark.gpu

f32 = np.float32
PI9 = np.pi / 9
# (flip, delta, factor, angle, scale, tx, ty) -> the widths 1, 2, 4/3, 4, 2, 4/3, 1, 10/3
PARAM_SETS = np.array([
    [0, 0.0, 1.0, 0.0, 1.0, 0.0, 0.0],                      # identity: width 1, the plain form
    [0, 0.0, 1.0, 0.0, 0.5, 0.0, 0.0],                      # scale 0.5
    [1, 0.0, 1.0, 0.0, 0.75, 0.0, 0.0],                     # scale 0.75, flipped
    [0, 0.0, 1.0, PI9, 0.25, 0.0, 0.0],                     # scale 0.25, the widest filter, rotated: the source lies inside the frame, pad around it
    [1, 0.05, 1.0, -PI9, 0.5, 0.3, -0.2],                   # rotated, flipped, moved so that part of the window is outside the source
    [0, -0.1, 1.0, 0.1, 0.75, -0.45, 0.45],                 # ... far outside: joints leave to the left and at the bottom
    [0, 0.0, 1.0, 0.2, 1.5, 0.1, 0.0],                      # scale 1.5: width 1
    [0, 0.0, 1.0, 0.3, 0.3, 0.45, 0.45],
], np.float64)
# (H, W, B, first row of PARAM_SETS, pad)
CASES = [(16, 24, 1, 4, 0.5), (16, 24, 3, 1, 0.5), (16, 24, 17, 1, 0.25), (40, 56, 3, 3, 0.0)]


def dev(a):
    return torch.as_tensor(np.array(a), device='cuda:0')      # (a copy: the shared cases are read-only)


def engine(**kw):
    from joint_cnn_mrf_amd.engine import Engine
    return Engine(device=0, **kw)


_CASES = {}


def case(H, W, B, first, pad):
    """One case's inputs and the restatement's answer, made once: (xb uint8, x float32, cells, colour, geom, width, x_ref, y_ref)."""
    key = (H, W, B, first, pad)
    if key not in _CASES:
        rs = np.random.RandomState(100 * H + B)
        xb = rs.randint(0, 256, (B, H, W, 3)).astype(np.uint8)
        cells = np.stack([rs.randint(0, H // 8 + 1, (B, 10)), rs.randint(0, W // 8 + 1, (B, 10))], axis=2).astype(np.int32)
        x = xb.astype(f32) / f32(255)
        col, g = augmentation.affine_geometry(PARAM_SETS[(np.arange(B) + first) % len(PARAM_SETS)], H, W)
        w = augmentation.affine_footprint(g)
        xr, yr, _ = A.augment(x, cells, col, g, w, pad)
        out = (xb, x, cells, col, g, w, xr, yr)
        for a in out:
            a.setflags(write=False)
        _CASES[key] = out
    return _CASES[key]


def same_bits(a, b):
    return np.array_equal(np.asarray(a, f32).view(np.uint32), np.asarray(b, f32).view(np.uint32))


@pytest.mark.parametrize('H,W,B,first,pad', CASES)
def test_images_bit_for_bit_against_the_restatement_and_maps_of_the_plain_entry(H, W, B, first, pad):
    xb, x, cells, col, g, w, xr, yr = case(H, W, B, first, pad)
    assert (w[:min(B, 3)] != 1).any() and (B < 17 or (w[16] != 1 and (w[:16] == 1).any()))      # the widths are mixed; the second launch has a wide one
    eng = engine()
    xg, yg = eng.augment_affine(dev(x), dev(cells), col, g, pad=pad, width=w)
    xp, yp = eng.augment_affine(dev(x), dev(cells), col, g, pad=pad)
    xg, yg, xp, yp = xg.cpu().numpy(), yg.cpu().numpy(), xp.cpu().numpy(), yp.cpu().numpy()
    eng.close()
    assert same_bits(yg, yp) and same_bits(yg, yr)
    for b in range(B):
        assert same_bits(xg[b], xr[b]), 'image %d (width %g): largest difference %g' % (b, w[b], np.abs(xg[b] - xr[b]).max())
        assert same_bits(xg[b], xp[b]) == (w[b] == 1.0)                                          # width 1: the plain entry's bits; wider: another picture


@pytest.mark.parametrize('B', [3, 17])
def test_indexed_and_byte_entries(B):
    """The indexed entry = gather_batch + the plain-form call; the byte entry = the float entry on the widened data.  Indices repeat."""
    H, W, N = 16, 24, 5
    xb, x, cells = case(H, W, 17, 1, 0.25)[:3]
    xb, x, cells = xb[:N], x[:N], cells[:N]
    idx = np.random.RandomState(B).randint(0, N, B).astype(np.int32)
    idx[-1] = idx[0]
    col, g = augmentation.affine_geometry(PARAM_SETS[(np.arange(B) + 1) % len(PARAM_SETS)][::-1], H, W)
    w = augmentation.affine_footprint(g)
    eng = engine()
    xd, cd = dev(x), dev(cells)
    xi, yi = eng.augment_affine_indexed(xd, cd, idx, col, g, pad=0.25, width=w)
    xu, yu = eng.augment_affine_indexed(dev(xb), cd, idx, col, g, pad=0.25, width=w)
    assert torch.equal(xu, xi) and torch.equal(yu, yi)
    xgat, _ = eng.gather_batch(xd, dev(np.zeros((N, H // 8, W // 8, 10), f32)), idx)
    xp, yp = eng.augment_affine(xgat, cd[torch.as_tensor(idx.astype(np.int64), device='cuda:0')].contiguous(), col, g, pad=0.25, width=w)
    assert torch.equal(xp, xi) and torch.equal(yp, yi)
    plain = eng.augment_affine_indexed(xd, cd, idx, col, g, pad=0.25)
    assert not torch.equal(plain[0], xi) and torch.equal(plain[1], yi)
    eng.close()


def test_fp32_and_bf16_handles_agree_bit_for_bit():
    xb, x, cells, col, g, w, xr, yr = case(16, 24, 3, 1, 0.5)
    e32, e16 = engine(precision='fp32'), engine(precision='bf16')
    a = e32.augment_affine(dev(x), dev(cells), col, g, pad=0.5, width=w)
    b = e16.augment_affine(dev(x), dev(cells), col, g, pad=0.5, width=w)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and same_bits(a[0].cpu().numpy(), xr)
    e32.close()
    e16.close()


def test_widths_of_one_are_the_plain_entry_bit_for_bit_and_another_factor_stays_within_its_bound():
    H, W, B = 40, 56, 17
    rs = np.random.RandomState(5)
    xb = rs.randint(0, 256, (B, H, W, 3)).astype(np.uint8)
    x = xb.astype(f32) / f32(255)
    cells = np.stack([rs.randint(0, H // 8 + 1, (B, 10)), rs.randint(0, W // 8 + 1, (B, 10))], axis=2).astype(np.int32)
    draw = augmentation.draw_affine(np.random.RandomState(6), B, H, W, pad=0.5, shift=0.2)      # colour, rotation and scales on both sides of 1
    assert (draw.colour[:, 2] != 1).all() and (augmentation.affine_footprint(draw.geom) > 1).any()
    eng = engine()
    one = np.ones(B)
    a = eng.augment_affine(dev(x), dev(cells), draw.colour, draw.geom, pad=0.5, width=one)
    p = eng.augment_affine(dev(x), dev(cells), draw.colour, draw.geom, pad=0.5)
    assert torch.equal(a[0], p[0]) and torch.equal(a[1], p[1])
    idx = np.arange(B, dtype=np.int32)[::-1].copy()
    for src in (dev(x), dev(xb)):
        ai = eng.augment_affine_indexed(src, dev(cells), idx, draw.colour, draw.geom, pad=0.5, width=one)
        pi = eng.augment_affine_indexed(src, dev(cells), idx, draw.colour, draw.geom, pad=0.5)
        assert torch.equal(ai[0], pi[0]) and torch.equal(ai[1], pi[1])
    # factor 1.2 under a filter of width 2: the restatement's colour step is held to 1e-6, as the plain entry's is
    col, g = augmentation.affine_geometry(np.array([[1, 32 / 255, 1.2, PI9, 0.5, 0.1, -0.1]]), 16, 24)
    x1, c1 = x[:1, :16, :24].copy(), np.minimum(cells[:1], [2, 3]).astype(np.int32)
    got = eng.augment_affine(dev(x1), dev(c1), col, g, pad=0.5, width=[2.0])[0].cpu().numpy()
    want = A.augment(x1, c1, col, g, [2.0], 0.5)[0]
    print('factor 1.2, width 2: share of differing image values %.3g, largest difference %.3g'
          % (np.mean(got.view(np.uint32) != want.view(np.uint32)), np.abs(got - want).max()))
    assert np.abs(got - want).max() <= 1e-6
    eng.close()


def test_the_checkerboard_on_the_device():
    """tests/test_affine_aa_cpu.py's aliasing case: the one-pixel checkerboard at scale 0.5 is 0.5 under the antialiased sample wherever the taps
    lie inside the source, within that test's bound, and a flat 0 there under the plain one."""
    from test_affine_aa_cpu import CHECKERBOARD_BOUND, checkerboard_case
    img, col, g = checkerboard_case()
    H, W = img.shape[:2]
    cells = np.ones((1, 10, 2), np.int32)
    eng = engine()
    aa = eng.augment_affine(dev(img[None]), dev(cells), col[None], g[None], pad=0.5, width=[2.0])[0][0].cpu().numpy()
    plain = eng.augment_affine(dev(img[None]), dev(cells), col[None], g[None], pad=0.5)[0][0].cpu().numpy()
    eng.close()
    inside = A.taps_inside(g, 2.0, H, W)
    worst_aa, worst_plain = np.abs(aa.astype(np.float64) - 0.5)[inside].max(), np.abs(plain.astype(np.float64) - 0.5)[inside].max()
    print('checkerboard at scale 0.5 on the device: antialiased within %.3g of 0.5, plain off by %.3g' % (worst_aa, worst_plain))
    assert worst_aa <= CHECKERBOARD_BOUND and worst_plain >= 0.25
    assert same_bits(aa, A.sample_image(img, col, g, 2.0, 0.5))


def test_entry_points_reject_bad_widths_and_write_nothing():
    lib = _lib.load()
    eng = engine()
    H, W, N, B = 16, 24, 5, 3
    xb, x, cells = case(H, W, 17, 1, 0.25)[:3]
    xd, ud, cd = dev(x[:N]), dev(xb[:N]), dev(cells[:N])
    col, g = augmentation.affine_geometry(PARAM_SETS[:B], H, W)
    good = augmentation.affine_footprint(g)
    xo, yo = torch.full((B, H, W, 3), 7.0, device='cuda:0'), torch.full((B, 2, 3, 10), 7.0, device='cuda:0')
    P = eng._p
    fp, dp, ip = ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int32)
    idx = np.array([0, 4, 4], np.int32)

    def call(kind, width, geom=g, hh=2):
        wa = None if width is None else np.ascontiguousarray(width, np.float64)
        wp = None if wa is None else wa.ctypes.data_as(dp)
        geom = np.ascontiguousarray(geom, np.float64)
        if kind == 'plain':
            return lib.jcm_augment_affine_aa(eng._h, P(xd[:B]), P(cd[:B]), col.ctypes.data_as(fp), geom.ctypes.data_as(dp), wp, B, H, W, hh, 3, 0.0, P(xo), P(yo))
        fn, src = (lib.jcm_augment_affine_aa_indexed_u8, ud) if kind == 'u8' else (lib.jcm_augment_affine_aa_indexed, xd)
        return fn(eng._h, P(src), P(cd), N, idx.ctypes.data_as(ip), col.ctypes.data_as(fp), geom.ctypes.data_as(dp), wp, B, H, W, hh, 3, 0.0, P(xo), P(yo))

    bad_geom = g.copy()
    bad_geom[1, 8] = np.nan
    for kind, name in (('plain', 'augment_affine_aa'), ('indexed', 'augment_affine_aa_indexed'), ('u8', 'augment_affine_aa_indexed_u8')):
        for pos, bad in ((1, 0.5), (2, 4.5), (0, np.nan), (1, np.inf), (2, -2.0)):
            w = good.copy()
            w[pos] = bad
            assert call(kind, w) == 1 and ('width[%d]' % pos) in _lib.last_error() and (name + ':') in _lib.last_error()      # 1: JCM_ERR_ARG
        assert call(kind, None) == 1 and 'null pointer' in _lib.last_error()
        assert call(kind, good, geom=bad_geom) == 1 and 'geom[1][8]' in _lib.last_error()          # the plain entries' checks, under the new names
        assert call(kind, good, hh=3) == 1 and 'H == 8 h' in _lib.last_error()
    torch.cuda.synchronize()
    assert bool((xo == 7.0).all()) and bool((yo == 7.0).all())
    for kind in ('plain', 'indexed', 'u8'):                                                        # and the same calls with good widths run
        xo.fill_(7.0)
        assert call(kind, good) == 0 and call(kind, [1.0, 4.0, 4.0 / 3.0]) == 0
        torch.cuda.synchronize()
        assert not bool((xo == 7.0).any()) and not bool((yo == 7.0).any())
    with pytest.raises(ValueError):
        eng.augment_affine(xd[:B], cd[:B], col, g, width=[1.0, 0.5, 1.0])
    with pytest.raises(ValueError):
        eng.augment_affine(xd[:B], cd[:B], col, g, width=[1.0, 1.0])
    eng.close()


# ------------------------------------------------------------------ training step
@pytest.fixture(scope='module')
def debug_case():
    p = synth.make_pd_params(debug=True, bn='trained')
    p.update(synth.make_sm_params(synth.synthetic_priors(), kind='trained'))
    return p, synth.make_images(2), synth.make_targets(2)


def test_train_step_with_an_antialiased_draw_equals_the_step_on_the_augmented_batch(debug_case):
    from joint_cnn_mrf_amd.train import Trainer
    params, x, y = debug_case
    draw = augmentation.draw_affine(np.random.RandomState(9), 2, 480, 720, pad=0.5, shift=0.2, scale=(0.5, 0.9), antialias=True)
    assert (draw.width > 1).all()
    ea, eb = engine().load_params(params), engine().load_params(params)
    ta, tb = Trainer(ea, use_sm=True, lmbd=0.001), Trainer(eb, use_sm=True, lmbd=0.001)
    xa, ya = eb.augment_affine(dev(x), eb.joint_cells(dev(y)), draw.colour, draw.geom, draw.pad, width=draw.width)
    xp, _ = eb.augment_affine(dev(x), eb.joint_cells(dev(y)), draw.colour, draw.geom, draw.pad)
    assert not torch.equal(xa, xp)
    la, _ = ta.train_step(dev(x), dev(y), augment=draw)
    lb, _ = tb.train_step(xa, ya)
    assert torch.equal(la, lb) and torch.equal(ta.grads, tb.grads)
    assert torch.equal(ta.last_batch[0], xa) and torch.equal(ta.last_batch[1], ya)
    ea.close()
    eb.close()


def test_tower_trainer_passes_the_widths_from_a_byte_data_set(debug_case):
    from joint_cnn_mrf_amd.dataset import DeviceDataset
    from joint_cnn_mrf_amd.dist import Towers
    from joint_cnn_mrf_amd.eval_run import byte_grid
    from joint_cnn_mrf_amd.main import TowerTrainer
    params, x, y = debug_case
    xb, seed, idx = byte_grid(x), 21, np.array([1, 0], np.int32)
    kw = dict(pad=0.5, scale=(0.5, 0.9), shift=0.1, antialias=True)
    towers = Towers(params, [0])
    tt = TowerTrainer(towers, params, augment_rng=np.random.RandomState(seed), augment_kind='affine', affine_kw=kw, use_sm=True, lmbd=0.001)
    tt.train_step_indexed(DeviceDataset.for_towers(towers, xb, y, image_dtype='uint8'), idx)
    torch.cuda.synchronize()
    seen = [t.clone() for t in tt.trainers[0].last_batch]
    towers.close()
    draw = augmentation.draw_affine(np.random.RandomState(seed), 2, 480, 720, **kw)
    eng = engine()
    xf = dev(xb.astype(f32) / f32(255))[torch.as_tensor(idx.astype(np.int64), device='cuda:0')].contiguous()
    want = eng.augment_affine(xf, eng.joint_cells(dev(y[idx])), draw.colour, draw.geom, draw.pad, width=draw.width)
    assert torch.equal(seen[0], want[0]) and torch.equal(seen[1], want[1])
    eng.close()


def test_cli_train_with_the_antialiased_augmentation(tmp_path):
    from cli_util import run_cli
    r = run_cli(['--train', '--synthetic', '--debug', '--augm_affine', '--augm_antialias', '--device_data', '--u8_images', '--augm_shift', '0.1', '--augm_pad', '0.5',
                 '--synthetic_size', '4', '--batch_size', '2', '--n_epochs', '1', '--gpus', '0', '--model_path', str(tmp_path / 'models_ex')], str(tmp_path), timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith('Epoch ')]
    assert [l.split()[1] for l in lines] == ['0', '1'] and 'train_mse' in lines[-1]
