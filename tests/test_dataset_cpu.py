"""Device-resident data without a GPU (joint_cnn_mrf_amd/dataset.py): the epoch's index table against
evaluation.get_next_batch (same batches, same use of the random state), the chunk plan of the upload, and the two entry
points of the C ABI (bound, exported, argument checks that run before anything touches a device)."""
import ctypes

import numpy as np
import pytest

import joint_cnn_mrf_amd  # noqa: F401
from joint_cnn_mrf_amd import _lib, dataset, evaluation


@pytest.mark.parametrize('n,batch_size', [(8, 4), (10, 4), (56, 14), (57, 14), (3, 4), (1, 1), (1100, 16)])
@pytest.mark.parametrize('shuffle', [True, False])
def test_epoch_indices_are_the_batches_of_get_next_batch(n, batch_size, shuffle):
    X = np.arange(n)
    ra, rb = np.random.RandomState(17), np.random.RandomState(17)
    for _epoch in range(3):                      # the state carries over from epoch to epoch as in train_main
        want = [bx for bx, _ in evaluation.get_next_batch(X, X, batch_size, shuffle=shuffle, rng=ra)]
        got = dataset.epoch_indices(n, rb, batch_size, shuffle=shuffle)
        assert got.dtype == np.int32 and got.shape == (n // batch_size, batch_size)
        assert len(want) == got.shape[0]
        for w, g in zip(want, got):
            np.testing.assert_array_equal(w, g)   # X = arange: the batch IS its indices
        assert ra.random_sample() == rb.random_sample()
    assert not shuffle or n < 8 or not np.array_equal(got.reshape(-1), np.arange(got.size))


@pytest.mark.parametrize('n,chunk', [(12, 4), (12, 5), (12, 12), (12, 13), (12, 1), (1, 3), (1101, 64), (0, 4)])
def test_chunk_plan_covers_every_row_once(n, chunk):
    plan = dataset.plan_chunks(n, chunk)
    seen = np.zeros(n, np.int64)
    for lo, hi in plan:
        assert 0 <= lo < hi <= n and hi - lo <= chunk
        seen[lo:hi] += 1
    assert (seen == 1).all()
    assert [lo for lo, _ in plan] == sorted(lo for lo, _ in plan)
    assert len(plan) == -(-n // chunk)


def test_chunk_plan_rejects_bad_arguments():
    for n, chunk in ((4, 0), (4, -1), (-1, 4)):
        with pytest.raises(ValueError):
            dataset.plan_chunks(n, chunk)


def test_entry_points_are_bound_and_exported():
    lib = _lib.load()
    for name in ('jcm_gather_batch', 'jcm_augment_train_indexed'):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert lib.jcm_abi_version() == 1


def test_entry_points_reject_a_null_handle():
    lib = _lib.load()
    idx = (ctypes.c_int32 * 1)(0)
    assert lib.jcm_gather_batch(None, None, None, 1, idx, 1, 2, 2, 2, 2, None, None) == 1            # JCM_ERR_ARG
    assert lib.jcm_augment_train_indexed(None, None, None, 1, idx, None, 1, 2, 2, 2, 2, None, None) == 1
