"""Rendered people without a GPU: the numpy restatement tests/synth_people_ref.py against closed forms, the scene builder
synth.people_scene / people_batch, the geometry pinned to the annotation through the restatement's image, and the new refusals of the command line."""
import argparse
import os

import numpy as np
import pytest
from numpy.testing import assert_array_equal

import synth_people_ref as R
import joint_cnn_mrf_amd  # noqa: F401
from joint_cnn_mrf_amd import data, synth
from joint_cnn_mrf_amd import main as M

HERE = os.path.dirname(os.path.abspath(__file__))
POSES = os.path.join(HERE, 'golden', 'flic_train_xy.npy')


@pytest.fixture(scope='module')
def poses():
    return np.load(POSES)


# ------------------------------------------------------------------ the restatement against closed forms
def test_nothing_drawn_is_a_constant_image():
    img = R.render(R.record(seed=5, c0=(10, 200, 77)), np.zeros((0, 16), np.int32), 9, 13)
    assert img.shape == (9, 13, 3) and img.dtype == np.uint8
    assert (img == np.array([10, 200, 77], np.uint8)).all()


def test_the_gradient_hits_both_colours_and_floors_between():
    c0, c1 = (10, 250, 100), (250, 10, 100)
    img = R.render(R.record(c0=c0, c1=c1), np.zeros((0, 16), np.int32), 7, 3)
    assert_array_equal(img[0, 0], c0)
    assert_array_equal(img[6, 2], c1)
    assert_array_equal(img[1, 1], (50, 210, 100))            # 10 + floor(240 / 6), 250 + floor(-240 / 6)
    img = R.render(R.record(c0=(0, 9, 0), c1=(10, 0, 0)), np.zeros((0, 16), np.int32), 4, 1)
    assert_array_equal(img[:, 0, 0], (0, 3, 6, 10))          # floor(10 y / 3)
    assert_array_equal(img[:, 0, 1], (9, 6, 3, 0))           # 9 + floor(-9 y / 3)
    assert_array_equal(R.render(R.record(c0=(1, 2, 3), c1=(9, 9, 9)), np.zeros((0, 16), np.int32), 1, 4)[0, 0], (1, 2, 3))      # H = 1: row 0 only


def test_an_axis_aligned_quadrilateral_covers_whole_pixels_and_halves():
    """Rows 2..4 whole (samples reach 16 y +- 6: the edge at 16 * 2 - 8 lies outside them), columns 3..5 whole and column 6 half: the right edge at
    16 * 6 runs through the pixel's centre, two of the four sample columns (-6, -2) are inside."""
    q = R.quad([(16 * 2 - 8, 16 * 3 - 8), (16 * 2 - 8, 16 * 6), (16 * 4 + 8, 16 * 6), (16 * 4 + 8, 16 * 3 - 8)], (200, 100, 40))
    img = R.render(R.record(c0=(20, 20, 20), n=1), q[None], 8, 9).astype(int)
    assert (img[2:5, 3:6] == (200, 100, 40)).all()
    assert (img[2:5, 6] == ((8 * 200 + 8 * 20 + 8) >> 4, (8 * 100 + 8 * 20 + 8) >> 4, (8 * 40 + 8 * 20 + 8) >> 4)).all()
    outside = np.ones((8, 9), bool)
    outside[2:5, 3:7] = False
    assert (img[outside] == 20).all()
    rev = R.quad([(16 * 4 + 8, 16 * 3 - 8), (16 * 4 + 8, 16 * 6), (16 * 2 - 8, 16 * 6), (16 * 2 - 8, 16 * 3 - 8)], (200, 100, 40))      # the other winding
    assert_array_equal(R.render(R.record(c0=(20, 20, 20), n=1), rev[None], 8, 9), img)


def test_a_zero_length_capsule_is_a_disc():
    r = 16 * 3
    img = R.render(R.record(n=1), R.capsule(16 * 6, 16 * 7, 16 * 6, 16 * 7, r, (255, 255, 255))[None], 13, 15)
    sy = (16 * np.arange(13)[:, None] + R.SUB[None, :]).reshape(13, 1, 4, 1) - 16 * 6
    sx = (16 * np.arange(15)[:, None] + R.SUB[None, :]).reshape(1, 15, 1, 4) - 16 * 7
    c = (sy * sy + sx * sx <= r * r).sum(axis=(2, 3))
    assert c.max() == 16 and 0 < c[6, 10] < 16       # the rim at x = 10 is cut
    assert_array_equal(img[:, :, 0], (c * 255 + 8) >> 4)


def test_overlapping_primitives_compose_in_listing_order():
    a = R.quad([(0, 0), (0, 16 * 5), (16 * 5, 16 * 5), (16 * 5, 0)], (255, 0, 0))
    b = R.capsule(16 * 2, 16 * 2, 16 * 2, 16 * 2, 16 * 2, (0, 0, 255))
    ab = R.render(R.record(n=2), np.stack([a, b]), 6, 6)
    ba = R.render(R.record(n=2), np.stack([b, a]), 6, 6)
    assert_array_equal(ab[2, 2], (0, 0, 255))
    assert_array_equal(ba[2, 2], (255, 0, 0))
    only_second = R.render(R.record(n=1, first=1), np.stack([a, b]), 6, 6)      # the record names its own primitives
    assert_array_equal(only_second, R.render(R.record(n=1), b[None], 6, 6))


def test_texture_and_octaves_stay_inside_their_amplitudes():
    img = R.render(R.record(seed=3, c0=(128, 128, 128), amp=(40, 0, 0, 0)), np.zeros((0, 16), np.int32), 40, 70).astype(int)
    assert np.abs(img - 128).max() <= 20 and img.std() > 0 and (img[..., 0] == img[..., 1]).all()
    q = R.quad([(-16, -16), (-16, 16 * 80), (16 * 50, 16 * 80), (16 * 50, -16)], (100, 100, 100), tamp=64, ts=1, tseed=9)
    tex = R.render(R.record(n=1), q[None], 40, 70).astype(int)
    assert np.abs(tex - 100).max() <= 32 and tex.std() > 0      # floor(64 * (vn - 128) / 256) lies in -32..31
    v = R.vnoise(7, 3, np.arange(64)[:, None], np.arange(64)[None, :])
    assert v.min() >= 0 and v.max() <= 255
    assert_array_equal(v[::8, ::8], (R.hash32(7, np.arange(8)[:, None], np.arange(8)[None, :]) >> np.uint64(24)).astype(np.int64))      # lattice points
    assert int(R.hash32(-1, 2, 3)) == int(R.hash32(2 ** 32 - 1, 2, 3)) and int(R.hash32(1, 2, 3)) != int(R.hash32(1, 3, 2))


def test_sensor_noise_stays_within_its_amplitude_and_varies():
    a = 5
    img = R.render(R.record(seed=11, c0=(100, 100, 100), a=a), np.zeros((0, 16), np.int32), 30, 40).astype(int)
    assert np.abs(img - 100).max() == a and len(np.unique(img)) == 2 * a + 1
    assert (img[..., 0] != img[..., 1]).any()
    dark = R.render(R.record(seed=11, c0=(1, 1, 1), a=a), np.zeros((0, 16), np.int32), 30, 40)
    assert dark.min() == 0 and dark.max() == 1 + a           # clamped below


# ------------------------------------------------------------------ the scene builder
def test_people_scene_is_a_pure_function_of_the_seed(poses):
    one = synth.people_scene(np.random.RandomState(4), poses[10], poses[20])
    two = synth.people_scene(np.random.RandomState(4), poses[10], poses[20])
    other = synth.people_scene(np.random.RandomState(5), poses[10], poses[20])
    for a, b in zip(one, two):
        assert_array_equal(a, b)
    assert not np.array_equal(one[0], other[0])
    assert one[0].dtype == np.int32 and one[0].shape == (20,) and one[1].dtype == np.int32 and one[1].shape[1] == 16
    assert one[2].dtype == np.float64 and one[2].shape == (2, 9)
    with pytest.raises(TypeError, match='unknown ranges'):
        synth.people_scene(np.random.RandomState(4), poses[10], colour=3)


def test_every_annotated_joint_is_inside_the_frame_for_every_pose(poses):
    assert poses.shape == (3987, 2, 9)
    rng = np.random.RandomState(0)
    most = 0
    for i in range(poses.shape[0]):
        rec, prims, xy = synth.people_scene(rng, poses[i], poses[(7 * i + 1) % poses.shape[0]])
        assert (xy[0] >= 0).all() and (xy[0] <= 719).all() and (xy[1] >= 0).all() and (xy[1] <= 479).all(), i
        assert rec[16] == prims.shape[0] <= 64
        most = max(most, prims.shape[0])
    assert most == 2 * 11 + 12      # two figures and the most clutter
    # an annotation that is outside the frame itself, left untransformed: moved inside by the least shift
    out = int(np.argmax((poses[:, 0] < 0).any(axis=1) | (poses[:, 0] > 719).any(axis=1) | (poses[:, 1] > 479).any(axis=1)))
    xy = synth.people_scene(np.random.RandomState(1), poses[out], tries=0)[2]
    assert synth._inside(xy, 480, 720) and not synth._inside(poses[out], 480, 720)


def test_people_batch_targets_are_the_data_sets_own(poses):
    recs, prims, xy, cells, y = synth.people_batch(np.random.RandomState(2), poses, [3, 1000, 2500])
    assert recs.shape == (3, 20) and xy.shape == (3, 2, 9) and cells.shape == (3, 10, 2) and y.shape == (3, 60, 90, 10) and y.dtype == np.float32
    assert_array_equal(cells, data.joint_cells(xy))
    assert_array_equal(y, data.target_heat_maps(cells))
    assert_array_equal(recs[:, 17], np.concatenate([[0], np.cumsum(recs[:, 16])[:-1]]))
    assert recs[:, 16].sum() == prims.shape[0]


def test_the_mirror_exchanges_left_and_right(poses):
    """With the similarity switched off a scene is the pose or its mirror image: x -> 719 - x with the joints exchanged by the table of hm_flip.h."""
    from joint_cnn_mrf_amd._lib import HM_FLIP_PERM
    assert synth.LR_PERM == HM_FLIP_PERM[:9]
    p = poses[100]
    seen = set()
    for seed in range(12):
        xy = synth.people_scene(np.random.RandomState(seed), p, scale=(1.0, 1.0), shift=0.0)[2]
        if np.allclose(xy, p, atol=1e-9):
            seen.add('plain')
        else:
            np.testing.assert_allclose(xy[0], 719 - p[0, list(HM_FLIP_PERM[:9])], atol=1e-9)
            np.testing.assert_allclose(xy[1], p[1, list(HM_FLIP_PERM[:9])], atol=1e-9)
            seen.add('mirror')
    assert seen == {'plain', 'mirror'}


def test_the_second_torso_keeps_its_distance(poses):
    rng = np.random.RandomState(6)
    for i in range(0, 3987, 40):
        rec, prims, xy = synth.people_scene(rng, poses[i], poses[(i + 13) % 3987], clutter=(0, 0), torso_margin=0.0)      # the quadrilaterals are the torsos
        assert prims.shape[0] == 22
        quads = prims[prims[:, 0] == 1]
        assert quads.shape[0] == 2      # the second person's torso first: they are behind
        centre = lambda q: np.array([q[1:9:2].mean(), q[2:9:2].mean()]) / 16.0      # noqa: E731
        d = np.hypot(*(centre(quads[0]) - centre(quads[1])))
        assert d >= synth.PEOPLE_DEFAULTS['other_dist'] * 8 - 1.0, (i, d)      # (the quadrilateral's centre is the torso centre up to the rounding)
        np.testing.assert_allclose(centre(quads[1]), (xy[:, [0, 3, 6, 7]].mean(axis=1))[::-1], atol=0.1)


def test_the_pixel_under_each_wrist_is_skin(poses):
    """Pins the geometry to the annotation: no clutter, no second person; the hands are listed last, so the wrist's own pixel shows the skin
    colour to within the texture amplitude (half of it each way) and the sensor-noise amplitude."""
    rng = np.random.RandomState(8)
    for i in (0, 500, 1500, 2500, 3900):
        rec, prims, xy = synth.people_scene(rng, poses[i], None, clutter=(0, 0))
        assert prims.shape[0] == 11
        img = R.render(rec, prims, 480, 720).astype(int)
        hand = prims[-1]
        assert hand[0] == 0 and (hand[1], hand[2]) == (hand[3], hand[4])      # a disc
        for k in (2, 5):
            px = img[int(round(xy[1, k])), int(round(xy[0, k]))]
            assert np.abs(px - hand[9:12]).max() <= hand[12] // 2 + 1 + rec[15], (i, k, px, hand[9:12])


# ------------------------------------------------------------------ the command line
def _refusal(argv):
    keep = argparse.Namespace(**vars(M.hps))
    try:
        M.main(list(argv) + ['--gpus', '99'])
    except SystemExit as e:
        return e.code
    finally:
        M.hps = keep
    return None


def test_the_new_refusals(tmp_path):
    wrong = str(tmp_path / 'wrong.npy')
    np.save(wrong, np.zeros((7, 9, 2)))
    f32 = str(tmp_path / 'f32.npy')
    np.save(f32, np.zeros((7, 2, 9), np.float32))
    assert _refusal(['--synth_people', POSES, '--synthetic']) == M.SYNTH_PEOPLE_NOT_WITH_SYNTHETIC
    assert _refusal(['--synth_people', POSES, '--predict', 'a.npy', '--predictions', 'o.json']) == M.SYNTH_PEOPLE_NOT_WITH_PREDICT
    for have in (['--train', '--device_data', '--u8_images'], ['--train', '--device_data', '--synth_people', POSES], ['--device_data', '--u8_images', '--synth_people', POSES],
                 ['--train', '--synth_people', POSES]):
        assert _refusal(['--synth_fresh'] + have) == M.SYNTH_FRESH_NEEDS_COMPANIONS, have
    assert _refusal(['--synth_dump', str(tmp_path)]) == M.SYNTH_DUMP_NEEDS_SYNTH_PEOPLE
    assert _refusal(['--synth_people', wrong]) == ('--synth_people %s: an [N,2,9] float64 array of at least five poses (data.py\'s xy) is expected; '
                                                   'the file holds float64 (7, 9, 2)' % wrong)
    assert 'the file holds float32 (7, 2, 9)' in _refusal(['--synth_people', f32])
    assert 'cannot be read' in _refusal(['--synth_people', str(tmp_path / 'none.npy')])
    # an earlier table's refusal still wins, and a good combination reaches the device check
    assert _refusal(['--synth_people', POSES, '--synthetic', '--restore']) == M.RESTORE_NEEDS_RESTORE_PATH
    ok = ['--train', '--device_data', '--u8_images', '--synth_people', POSES, '--synth_fresh', '--synth_dump', str(tmp_path)]
    assert _refusal(ok).startswith('--gpus [99]: device 99 does not exist')


def test_synthetic_alone_parses_as_before():
    a = M.build_parser().parse_args(['--synthetic'])
    assert a.synthetic and a.synth_people is None and not a.synth_fresh and a.synth_dump is None and a.synthetic_size == 56 and not a.synthetic_size_given
    assert _refusal(['--synthetic']).startswith('--gpus [99]: device 99 does not exist')
    from joint_cnn_mrf_amd import eval_run
    given = M.build_parser().parse_args(['--synthetic', '--synthetic_size', '56'])
    assert given.synthetic_size == 56 and given.synthetic_size_given
    x_train, y_train, x_test, y_test, _ = eval_run.load_data(argparse.Namespace(synthetic=True, synthetic_size=4, batch_size=2, train=False))
    assert x_train.shape[0] == 2 and x_test.shape[0] == 4
    assert_array_equal(x_test[:1], synth.make_images(1, seed=300))
    tr, te = eval_run.people_split(3987)
    assert len(tr) == 3189 and len(te) == 798 and tr[-1] + 1 == te[0] and te[-1] == 3986
