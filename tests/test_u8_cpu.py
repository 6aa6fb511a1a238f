"""Byte images without a GPU: the host conversion and its proof of exactness, the byte accounting of a uint8
DeviceDataset up to its refusal, the five new entry points of the C ABI, and the command line."""
import ctypes

import numpy as np
import pytest

import joint_cnn_mrf_amd  # noqa: F401
from joint_cnn_mrf_amd import _lib, dataset
from joint_cnn_mrf_amd import main as M
from joint_cnn_mrf_amd.dataset import DeviceDataset, DeviceDataTooLarge, NotByteExact, to_u8_exact

f32 = np.float32


def as_float(k):
    """THE reference of this feature: what data.load_image makes of a byte image, on the host with numpy."""
    return np.asarray(k, np.uint8).astype(f32) / f32(255)


def test_all_256_values_round_trip():
    k = np.arange(256, dtype=np.uint8)
    a = as_float(k)
    assert a.dtype == f32 and np.array_equal(np.rint(a * f32(255)), k.astype(f32))
    got = to_u8_exact(a)
    assert got.dtype == np.uint8 and np.array_equal(got, k)
    # the product with float32(1/255) is NOT the conversion: it differs for 126 of the 256 bytes
    assert int((k.astype(f32) * f32(1.0 / 255.0) != a).sum()) == 126


def test_random_byte_images_round_trip_and_bytes_pass_unchanged():
    rs = np.random.RandomState(3)
    k = rs.randint(0, 256, (3, 37, 53, 3)).astype(np.uint8)
    assert np.array_equal(to_u8_exact(as_float(k)), k)
    assert np.array_equal(to_u8_exact(as_float(k)[:, ::2, 1:]), k[:, ::2, 1:])         # a non-contiguous view
    assert to_u8_exact(k) is k
    with pytest.raises(TypeError):
        to_u8_exact(as_float(k).astype(np.float64))


@pytest.mark.parametrize('value', [0.5, 1.0 / 254.0, float('nan'), -0.25, 1.5, float('inf'), -0.0],
                         ids=['half', 'one_254th', 'nan', 'negative', 'above_one', 'inf', 'minus_zero'])
def test_values_off_the_byte_grid_are_refused_with_their_index(value):
    a = as_float(np.random.RandomState(5).randint(0, 256, (2, 5, 7, 3)))
    a[1, 3, 2, 1] = value
    a[1, 4, 0, 0] = value                          # a later one: the FIRST offending index is named
    with pytest.raises(NotByteExact) as ei:
        to_u8_exact(a)
    assert ei.value.index == (1, 3, 2, 1) and '(1, 3, 2, 1)' in str(ei.value)
    v = ei.value.value
    assert (np.isnan(v) and np.isnan(value)) or f32(v) == f32(value)
    assert isinstance(ei.value, ValueError)


def test_byte_dataset_counts_one_byte_per_image_value():
    x = np.zeros((6, 16, 24, 3), np.uint8)
    y = np.zeros((6, 2, 3, 10), f32)
    want = x.size + 4 * y.size                     # 6 912 + 1 440
    for xin in (x, as_float(x)):                   # given as bytes or as floats: the same accounting
        with pytest.raises(DeviceDataTooLarge) as ei:
            DeviceDataset(xin, y, device=0, budget_bytes=want - 1, image_dtype='uint8')
        msg = str(ei.value)
        assert str(want) in msg and str(want - 1) in msg and 'uint8' in msg
    with pytest.raises(DeviceDataTooLarge) as ei:   # the float storage of the same set: four bytes per value, today's text
        DeviceDataset(as_float(x), y, device=0, budget_bytes=want)
    assert str(4 * x.size + 4 * y.size) in str(ei.value) and 'fp32' in str(ei.value) and 'uint8' not in str(ei.value)
    with pytest.raises(ValueError):
        DeviceDataset(x, y, device=0, budget_bytes=1, image_dtype='float16')


def test_entry_points_are_bound_exported_and_reject_a_null_handle():
    lib = _lib.load()
    names = ('jcm_pd_forward_u8', 'jcm_forward_u8', 'jcm_eval_forward_u8', 'jcm_gather_batch_u8', 'jcm_augment_train_indexed_u8')
    for name in names:
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert lib.jcm_abi_version() == 1
    idx = (ctypes.c_int32 * 1)(0)
    assert lib.jcm_pd_forward_u8(None, None, 1, 8, 8, None) == 1                                         # JCM_ERR_ARG
    assert lib.jcm_forward_u8(None, None, None, 1, 8, 8, 0, None, None, None, None) == 1
    assert lib.jcm_eval_forward_u8(None, None, None, 1, 8, 8, 0, None, None, None, None, None) == 1
    assert lib.jcm_gather_batch_u8(None, None, None, 1, idx, 1, 2, 2, 2, 2, None, None) == 1
    assert lib.jcm_augment_train_indexed_u8(None, None, None, 1, idx, None, 1, 2, 2, 2, 2, None, None) == 1


def test_command_line_knows_the_flag_and_training_needs_device_data():
    p = M.build_parser()
    assert p.parse_args([]).u8_images is False
    assert p.parse_args(['--u8_images', '--train', '--device_data']).u8_images is True
    with pytest.raises(SystemExit) as ei:
        M.main(['--train', '--u8_images', '--synthetic', '--debug'])
    assert '--device_data' in str(ei.value) and '--u8_images' in str(ei.value)


def test_byte_grid_of_the_synthetic_images():
    x = np.asarray([0.0, 0.999999, 1.0, 0.5, 1.0 / 256, 255.0 / 256], f32)
    assert M.byte_grid(x).tolist() == [0, 255, 255, 128, 1, 255] and M.byte_grid(x).dtype == np.uint8
    from joint_cnn_mrf_amd import synth
    img = synth.make_images(1, seed=1)
    k = M.byte_grid(img)
    assert np.array_equal(to_u8_exact(as_float(k)), k) and np.abs(as_float(k) - img).max() <= 1.0 / 255 + 1e-6
