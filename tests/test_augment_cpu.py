"""Training-time augmentation without a GPU: known answers of the float32 restatement (tests/augment_ref.py), the float32
against the float64 formulation, the host-side parameter draw and check, and the C ABI entry point's presence."""
import ctypes

import numpy as np
import pytest
from hypothesis import given, settings, strategies as st

import augment_ref as A
import joint_cnn_mrf_amd  # noqa: F401
from joint_cnn_mrf_amd import _lib, augmentation

f32 = np.float32


def _rand(shape, seed):
    return np.random.RandomState(seed).random_sample(shape).astype(f32)


# ------------------------------------------------------------------ known answers of (a)
def test_zero_angle_full_box_is_the_identity():
    img = _rand((9, 13, 3), 1)
    hm = _rand((5, 7, 10), 2)
    for a in (img, hm):
        assert np.array_equal(A.rotate_f32(a, 0.0), a)
        assert np.array_equal(A.crop_resize_f32(a, 0.0, 0.0, crop_size=1.0), a)
        assert np.array_equal(A.crop_resize_f32(A.rotate_f32(a, 0.0), 0.0, 0.0, crop_size=1.0), a)


def test_flip_twice_is_the_identity():
    img = _rand((6, 11, 3), 3)
    hm = _rand((4, 9, 10), 4)
    x2, y2 = A.flip(*A.flip(img, hm))
    assert np.array_equal(x2, img) and np.array_equal(y2, hm)
    x1, y1 = A.flip(img, hm)
    assert np.array_equal(x1[:, 0], img[:, -1]) and np.array_equal(y1[:, 0, 3], hm[:, -1, 0])
    assert sorted(augmentation.HM_FLIP_PERM) == list(range(10))
    assert list(A.HM_FLIP_PERM) == list(augmentation.HM_FLIP_PERM)


def test_torso_channel_is_never_permuted():
    assert augmentation.HM_FLIP_PERM[9] == 9
    hm = _rand((5, 8, 10), 5)
    p = np.array([1, 0.01, 1.1, 0.0, 0.0, 0.0], f32)
    _, y_flip = A.augment_one_f32(_rand((5, 8, 3), 6), hm, p, crop_size=1.0)
    want = A.renorm_f32(hm[:, ::-1, 9:10])
    assert np.array_equal(y_flip[..., 9:10], want)


def test_square_rotation_by_a_right_angle_is_rot90():
    m = _rand((11, 11, 2), 7)
    np.testing.assert_allclose(A.rotate_f32(m, np.pi / 2), np.rot90(m), atol=1e-5, rtol=0)


def test_renormalised_maps_sum_to_one():
    x, y = _rand((3, 17, 23, 3), 8), _rand((3, 6, 9, 10), 9)
    _, ya = A.augment_f32(x, y, augmentation.draw_params(np.random.RandomState(0), 3))
    np.testing.assert_allclose(ya.astype(np.float64).sum(axis=(1, 2)), 1.0, atol=1e-5)
    assert (ya > 0).all()


def test_colour_steps_clip_to_the_unit_interval():
    img = _rand((8, 8, 3), 10)
    v = A.color_f32(img, 0.12, 1.2)
    assert v.min() >= 0 and v.max() <= 1 and (v == 1).any()


# ------------------------------------------------------------------ (a) against (b)
@settings(max_examples=25, deadline=None)
@given(H=st.integers(2, 24), W=st.integers(2, 24), h=st.integers(2, 9), w=st.integers(2, 9),
       flip=st.sampled_from([0.0, 1.0]), delta=st.floats(-32 / 255, 32 / 255), factor=st.floats(0.8, 1.2),
       angle=st.floats(-np.pi / 9, np.pi / 9), rh=st.floats(0, 0.05), rw=st.floats(0, 0.05), seed=st.integers(0, 2 ** 16))
def test_float32_restatement_against_float64(H, W, h, w, flip, delta, factor, angle, rh, rw, seed):
    x, y = _rand((1, H, W, 3), seed), _rand((1, h, w, 10), seed + 1)
    p = np.array([[flip, delta, factor, angle, rh, rw]], f32)
    xa, ya = A.augment_f32(x, y, p)
    xb, yb = A.augment_f64(x, y, p)
    assert np.abs(xa - xb).max() <= 1e-5
    assert (np.abs(ya - yb) / np.abs(yb).max(axis=(1, 2), keepdims=True)).max() <= 1e-4


# ------------------------------------------------------------------ parameters
def test_draw_params_columns_and_ranges():
    p = augmentation.draw_params(np.random.RandomState(3), 4096)
    assert p.dtype == np.float32 and p.shape == (4096, 6)
    u = np.random.RandomState(3).random_sample((4096, 6))
    assert np.array_equal(p[:, 0], (u[:, 0] > 0.5).astype(f32))
    np.testing.assert_allclose(p[:, 1], -32 / 255 + u[:, 1] * 64 / 255, rtol=1e-6, atol=1e-7)
    np.testing.assert_allclose(p[:, 2], 0.8 + 0.4 * u[:, 2], rtol=1e-6)
    np.testing.assert_allclose(p[:, 3], -np.pi / 9 + u[:, 3] * 2 * np.pi / 9, rtol=1e-6, atol=1e-7)
    np.testing.assert_allclose(p[:, 4:], 0.05 * u[:, 4:], rtol=1e-6)
    assert set(np.unique(p[:, 0])) == {0.0, 1.0}
    assert -32 / 255 - 1e-6 <= p[:, 1].min() and p[:, 1].max() <= 32 / 255 + 1e-6
    assert 0.8 - 1e-6 <= p[:, 2].min() and p[:, 2].max() <= 1.2 + 1e-6
    assert abs(p[:, 3]).max() <= augmentation.MAX_ROTATE_ANGLE + 1e-6
    assert p[:, 4:].min() >= 0 and p[:, 4:].max() <= 1 - augmentation.CROP_SIZE + 1e-6
    augmentation.check_params(p)


def test_draw_params_reproducible_and_sliced_from_the_global_batch():
    a = augmentation.draw_params(np.random.RandomState(11), 16)
    b = augmentation.draw_params(np.random.RandomState(11), 16)
    assert np.array_equal(a, b)
    assert not np.array_equal(a, augmentation.draw_params(np.random.RandomState(12), 16))
    # one draw for the global batch, sliced per tower: the same rows as the single-tower run
    from joint_cnn_mrf_amd.dist import shard_bounds
    rows = np.concatenate([a[lo:hi] for lo, hi in (shard_bounds(16, 2, i) for i in range(2))])
    assert np.array_equal(rows, a)


@pytest.mark.parametrize('bad', [
    np.zeros((2, 5), f32),
    np.zeros((6,), f32),
    np.zeros((0, 6), f32),
    np.array([[0, np.nan, 1, 0, 0, 0]], f32),
    np.array([[0, 0, np.inf, 0, 0, 0]], f32),
    np.array([[0.5, 0, 1, 0, 0, 0]], f32),
    np.array([[2, 0, 1, 0, 0, 0]], f32),
    np.array([[-1, 0, 1, 0, 0, 0]], f32),
])
def test_check_params_rejects(bad):
    with pytest.raises(ValueError):
        augmentation.check_params(bad)


def test_augment_test_is_the_identity():
    x, y = object(), object()
    assert augmentation.augment_test(x, y) == (x, y)


# ------------------------------------------------------------------ C ABI
def test_augment_entry_point_is_bound_and_exported():
    assert 'jcm_augment_train' in _lib.SIGNATURES
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(lib, 'jcm_augment_train')


def test_augment_entry_point_rejects_a_null_handle():
    lib = _lib.load()
    assert lib.jcm_augment_train(None, None, None, None, 1, 2, 2, 2, 2, None, None) == 1     # JCM_ERR_ARG
    assert 'null handle' in _lib.last_error()
