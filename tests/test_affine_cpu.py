"""The host side of the affine training augmentation and its restatement tests/affine_ref.py, on hand-computed known answers: the
geometry augmentation.affine_geometry folds, the draws, the checks and the command-line rules.  No device."""
import argparse

import numpy as np
import pytest

import affine_ref as R
import joint_cnn_mrf_amd  # noqa: F401
from joint_cnn_mrf_amd import augmentation as A
from joint_cnn_mrf_amd import data
from joint_cnn_mrf_amd import main as M

f32 = np.float32
H, W, HH, HW = 16, 24, 2, 3
IDENTITY = [0, 0.0, 1.0, 0.0, 1.0, 0.0, 0.0]      # (flip, delta, factor, angle, scale, tx, ty)


def dyadic_images(B, seed=0):
    """Values k / 256 with k in 128..255: the contrast mean lies in [0.5, 1), so (v - m) + m is exact in float32 and the identity colour step returns v."""
    return (np.random.RandomState(seed).randint(128, 256, (B, H, W, 3)) / 256.0).astype(f32)


def params(**kw):
    p = dict(zip(('flip', 'delta', 'factor', 'angle', 'scale', 'tx', 'ty'), IDENTITY))
    p.update(kw)
    return np.array([[p[k] for k in ('flip', 'delta', 'factor', 'angle', 'scale', 'tx', 'ty')]], np.float64)


CELLS = np.array([[[0, 0], [1, 2], [0, 1], [1, 0], [0, 2], [1, 1], [0, 0], [1, 2], [0, 1], [1, 1]]])      # [1,10,2], all inside the 2 x 3 map


def test_identity_parameters_give_the_identity_map_and_the_image_itself():
    col, g = A.affine_geometry(params(), H, W)
    assert col.dtype == f32 and g.dtype == np.float64 and col.shape == (1, 3) and g.shape == (1, 12)
    assert np.array_equal(g[0], [1, 0, 0, 0, 1, 0, 1, 0, 0, 0, 1, 0])
    x = dyadic_images(1)
    xo, yo, moved = R.augment(x, CELLS, col, g, pad=0.5)
    assert np.array_equal(xo.view(np.uint32), x.view(np.uint32))
    assert np.array_equal(moved, CELLS) and np.array_equal(yo, data.target_heat_maps(CELLS, HH, HW))


def test_integer_shift_is_the_shifted_copy_with_pad_in_the_vacated_band():
    col, g = A.affine_geometry(params(tx=3 / W, ty=-2 / H), H, W)      # +3 px along x, -2 px along y: 3 / 24 and 2 / 16 are exact
    assert np.array_equal(g[0, :6], [1, 0, -3, 0, 1, 2]) and np.array_equal(g[0, 6:], [1, 0, 3, 0, 1, -2])
    x = dyadic_images(1, seed=1)
    for pad in (0.0, 0.5):
        xo, yo, moved = R.augment(x, CELLS, col, g, pad=pad)
        want = np.full_like(x, f32(pad))
        want[0, :H - 2, 3:] = x[0, 2:, :W - 3]                        # out[r, q] = x[r + 2, q - 3]
        assert np.array_equal(xo.view(np.uint32), want.view(np.uint32))
        assert np.array_equal(moved, CELLS)                           # 3 and 2 pixels do not leave an 8-pixel cell from its centre
        assert np.array_equal(yo, data.target_heat_maps(CELLS, HH, HW))


def test_flip_alone_mirrors_the_image_and_permutes_the_channels():
    col, g = A.affine_geometry(params(flip=1), H, W)
    assert np.array_equal(g[0], [-1, 0, W - 1, 0, 1, 0, -1, 0, W - 1, 0, 1, 0])
    x = dyadic_images(1, seed=2)
    xo, yo, moved = R.augment(x, CELLS, col, g)
    assert np.array_equal(xo.view(np.uint32), x[:, :, ::-1].view(np.uint32))
    y = data.target_heat_maps(CELLS, HH, HW)
    assert np.array_equal(yo, y[:, :, ::-1][..., list(A.HM_FLIP_PERM)])
    assert np.array_equal(moved[0], np.stack([CELLS[0, list(A.HM_FLIP_PERM), 0], HW - 1 - CELLS[0, list(A.HM_FLIP_PERM), 1]], axis=1))


@pytest.mark.parametrize('size', [(16, 24), (480, 720)])
def test_forward_map_undoes_the_inverse_map(size):
    h, w = size
    p = A.draw_affine_params(np.random.RandomState(3), 64, shift=0.3)
    _, g = A.affine_geometry(p, h, w)
    inv = np.concatenate([g[:, :6].reshape(-1, 2, 3), np.tile([[[0, 0, 1]]], (64, 1, 1))], axis=1)
    fwd = np.concatenate([g[:, 6:].reshape(-1, 2, 3), np.tile([[[0, 0, 1]]], (64, 1, 1))], axis=1)
    # the composition as a matrix, its offsets in units of the frame: the identity to 1e-12
    unit = np.diag([1.0 / w, 1.0 / h, 1.0])
    for prod in (fwd @ inv, inv @ fwd):
        comp = unit @ prod @ np.linalg.inv(unit)
        assert np.abs(comp - np.eye(3)).max() <= 1e-12
    assert p[:, 0].min() == 0 and p[:, 0].max() == 1                  # both orientations were drawn


def test_a_joint_pushed_out_of_the_frame_lands_on_the_clamped_border_cell():
    x = dyadic_images(1, seed=4)
    cells = np.array([[[0, 0], [1, 2], [0, 2], [1, 0], [1, 1], [0, 1], [1, 1], [0, 0], [1, 2], [0, 1]]])
    # +0.45 W to the right, +0.45 H down: 10.8 and 7.2 pixels
    col, g = A.affine_geometry(params(tx=0.45, ty=0.45), H, W)
    _, yo, moved = R.augment(x, cells, col, g)
    qx, qy = 8 * cells[0, :, 1] + 3.5 + 0.45 * W, 8 * cells[0, :, 0] + 3.5 + 0.45 * H
    want = np.stack([(np.minimum(qy, H) / 8).astype(int), (np.minimum(qx, W) / 8).astype(int)], axis=1)
    assert np.array_equal(moved[0], want)
    assert moved[0, 1].tolist() == [HH, HW] and moved[0, 2].tolist() == [1, HW]      # clamped to row h / column w, past the last cell
    assert np.array_equal(yo, data.target_heat_maps(moved, HH, HW))
    assert yo[0, :, :, 1].tolist() == [[0, 0, 0], [0, 0, 1 / 16]]                    # the blob's corner is all the border leaves of it
    assert yo[0, :, :, 2].tolist() == [[0, 0, 1 / 16], [0, 0, 2 / 16]]
    # to the left and up: clamped to row 0 / column 0, which are cells of the map
    col, g = A.affine_geometry(params(tx=-0.49, ty=-0.49), H, W)
    _, yo, moved = R.augment(x, cells, col, g)
    assert moved[0, 0].tolist() == [0, 0] and np.array_equal(yo, data.target_heat_maps(moved, HH, HW))
    assert yo[0, :, :, 0].tolist() == [[4 / 16, 2 / 16, 0], [2 / 16, 1 / 16, 0]]


def test_draw_affine_params_ranges_and_determinism():
    p = A.draw_affine_params(np.random.RandomState(5), 4000, scale=(0.7, 1.3), max_angle=0.2, shift=0.1)
    assert p.dtype == np.float64 and p.shape == (4000, 7)
    assert set(np.unique(p[:, 0])) == {0.0, 1.0}
    for col, lo, hi in ((1, -A.MAX_BRIGHTNESS_DELTA, A.MAX_BRIGHTNESS_DELTA), (2, A.CONTRAST_LOWER, A.CONTRAST_UPPER), (3, -0.2, 0.2), (4, 0.7, 1.3),
                        (5, -0.1, 0.1), (6, -0.1, 0.1)):
        assert lo <= p[:, col].min() < lo + 0.01 * (hi - lo) and hi - 0.01 * (hi - lo) < p[:, col].max() <= hi
    assert np.array_equal(p, A.draw_affine_params(np.random.RandomState(5), 4000, scale=(0.7, 1.3), max_angle=0.2, shift=0.1))
    rs, twin = np.random.RandomState(6), np.random.RandomState(6)
    d = A.draw_affine_params(rs, 3)                                   # the defaults: scale [0.5, 1.5], +-pi/9, no shift
    twin.random_sample((3, 7))
    assert rs.random_sample() == twin.random_sample()                 # one draw of [B, 7] and nothing else
    assert np.all(d[:, 5:] == 0) and np.all((d[:, 4] >= 0.5) & (d[:, 4] <= 1.5)) and np.all(np.abs(d[:, 3]) <= np.pi / 9)
    assert (A.AFFINE_SCALE, A.AFFINE_SHIFT, A.MAX_ROTATE_ANGLE) == ((0.5, 1.5), 0.0, np.pi / 9)
    for bad in (dict(scale=(0.0, 1.0)), dict(scale=(1.2, 1.1)), dict(shift=0.5), dict(shift=-0.1)):
        with pytest.raises(ValueError):
            A.draw_affine_params(np.random.RandomState(0), 2, **bad)
    draw = A.draw_affine(np.random.RandomState(7), 5, H, W, pad=0.25, shift=0.2)
    assert len(draw) == 5 and draw.pad == 0.25 and len(draw[1:3]) == 2 and np.array_equal(draw[1:3].geom, draw.geom[1:3])


def test_check_affine_rejections():
    col, g = A.affine_geometry(A.draw_affine_params(np.random.RandomState(8), 3), H, W)
    c2, g2 = A.check_affine(col.tolist(), g.tolist())
    assert c2.dtype == f32 and g2.dtype == np.float64 and np.array_equal(c2, col) and np.array_equal(g2, g)

    def changed(a, i, j, v):
        a = a.copy()
        a[i, j] = v
        return a
    bad = [(col[:, :2], g), (col, g[:, :11]), (col, g[:2]), (col[0], g[0]),
           (changed(col, 1, 1, np.nan), g), (col, changed(g, 2, 7, np.inf)), (changed(col, 0, 0, 0.5), g),
           (col, np.concatenate([np.zeros((3, 6)), g[:, 6:]], axis=1)),                                # a singular inverse map
           (col, changed(changed(g, 0, 6, 0.0), 0, 7, 0.0))]                                          # a singular forward map
    for c, gg in bad:
        with pytest.raises(ValueError):
            A.check_affine(c, gg)
    with pytest.raises(ValueError):
        A.AffineDraw(col, g, pad=np.nan)


REFUSALS = [
    (['--augm_affine'], M.AUGM_AFFINE_NEEDS_TRAIN),
    (['--augm_affine', '--synthetic', '--debug'], M.AUGM_AFFINE_NEEDS_TRAIN),
    (['--train', '--augm_scale', '0.8', '1.2'], M.AUGM_OPTION_NEEDS_AUGM_AFFINE),
    (['--train', '--augm_shift', '0.1'], M.AUGM_OPTION_NEEDS_AUGM_AFFINE),
    (['--augm_pad', '0.5'], M.AUGM_OPTION_NEEDS_AUGM_AFFINE),
    (['--train', '--augm_affine', '--augm_scale', '0', '1'], '--augm_scale 0 1: 0 < LO <= HI'),
    (['--train', '--augm_affine', '--augm_scale', '1.2', '1.1'], '--augm_scale 1.2 1.1: 0 < LO <= HI'),
    (['--train', '--augm_affine', '--augm_shift', '0.5'], '--augm_shift 0.5: 0 <= F < 0.5'),
    (['--train', '--augm_affine', '--augm_shift', '-0.1'], '--augm_shift -0.1: 0 <= F < 0.5'),
    (['--train', '--augm_affine', '--augm_pad', '1.5'], '--augm_pad 1.5: 0 <= V <= 1'),
    (['--train', '--augm_affine', '--augm_pad', '-0.5'], '--augm_pad -0.5: 0 <= V <= 1'),
    (['--train', '--augm_affine', '--u8_images'], M.U8_TRAIN_NEEDS_DEVICE_DATA),                       # an earlier table's rule still comes first
]


@pytest.mark.parametrize('argv,message', REFUSALS)
def test_cli_refusals(argv, message):
    keep = argparse.Namespace(**vars(M.hps))
    try:
        with pytest.raises(SystemExit) as ei:
            M.main(list(argv) + ['--gpus', '99'])
    finally:
        M.hps = keep
    assert ei.value.code == message


def test_accepted_flags_reach_the_device_check():
    """A valid combination passes every rule: on a machine without the device it ends at the --gpus check, not at a refusal."""
    keep = argparse.Namespace(**vars(M.hps))
    try:
        with pytest.raises(SystemExit) as ei:
            M.main(['--train', '--augm_affine', '--augm_scale', '0.8', '1.25', '--augm_shift', '0.1', '--augm_pad', '0.5', '--gpus', '99'])
    finally:
        M.hps = keep
    assert str(ei.value.code).startswith('--gpus [99]: device 99 does not exist')


def test_new_rules_follow_the_recorded_ones_and_defaults_are_declared_placeholders():
    assert M.FLAG_RULES[-1][1] == M.RENDER_HEAT_SM_NEEDS_USE_SM and M.SEQUENCE_RULES[-1][1] == M.SEQ_OPTION_NEEDS_SEQUENCE
    assert [m for _, m in M.AUGM_RULES[:2]] == [M.AUGM_AFFINE_NEEDS_TRAIN, M.AUGM_OPTION_NEEDS_AUGM_AFFINE] and len(M.AUGM_RULES) == 5
    text = ' '.join(M.build_parser().format_help().split())
    assert text.count('untuned placeholder') >= 4 and 'has not been measured' in text      # --seq_sigma, --seq_rho, --augm_scale, --augm_shift
