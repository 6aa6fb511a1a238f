"""The argument helpers the modules of engine/ share (engine/_core.py): every refusal keeps the words of the site it replaced -- the literals
below are copied from engine.py as it stood before the split, where _seq_shift, _seq_centre and frame_flow held the table checks and
_chk_indexed and _affine_call the index checks -- and what passes comes back as those sites made it."""
import re

import numpy as np
import pytest
import torch

import joint_cnn_mrf_amd  # noqa: F401
from joint_cnn_mrf_amd.engine._core import _drop, _host_index, _host_table, _lift


def _refused(fn, args, message):
    with pytest.raises(ValueError, match='^' + re.escape(message) + '$'):
        fn(*args)


def test_host_table_refusals():
    _refused(_host_table, ('shift', np.array([[0.5, 1.0]])), 'shift must hold int32 values, got float64')
    _refused(_host_table, ('centre', np.array([0, 2 ** 31], np.int64)), 'centre must hold int32 values, got int64')
    _refused(_host_table, ('centre', np.array([-2 ** 31 - 1, 0], np.int64)), 'centre must hold int32 values, got int64')
    _refused(_host_table, ('ref', torch.zeros(2, 2, dtype=torch.int64)), 'ref must be int32, got torch.int64')
    _refused(_host_table, ('ref', [[True, False]]), 'ref must hold int32 values, got bool')


def test_host_table_passes():
    a = np.array([[-2 ** 31, 5], [7, 2 ** 31 - 1]], np.int64)
    t = _host_table('shift', a[:, ::-1])      # not contiguous
    assert t.dtype == torch.int32 and t.device.type == 'cpu' and t.is_contiguous() and np.array_equal(t.numpy(), a[:, ::-1])
    assert _host_table('ref', [[0, -1]]).tolist() == [[0, -1]]
    assert tuple(_host_table('centre', np.zeros((0, 2), np.uint8)).shape) == (0, 2)      # an empty table has no value to check
    given = torch.arange(6, dtype=torch.int32).view(3, 2).t()      # a tensor comes back as itself, layout and all
    assert _host_table('shift', given) is given


IDX_HOST = '%s: idx is a host array (it is checked on the host and travels in the kernel arguments), got a tensor on %s'
IDX_SHAPE = '%s: idx must be a non-empty 1-D integer array, got shape %s dtype %s'


def test_host_index_refusals():
    _refused(_host_index, ('gather_batch', torch.zeros(3, dtype=torch.int32, device='meta')), IDX_HOST % ('gather_batch', 'meta'))
    _refused(_host_index, ('gather_batch', np.zeros((2, 2), np.int32)), IDX_SHAPE % ('gather_batch', '(2, 2)', 'int32'))
    _refused(_host_index, ('augment_train_indexed', np.zeros(0, np.int64)), IDX_SHAPE % ('augment_train_indexed', '(0,)', 'int64'))
    _refused(_host_index, ('augment_affine_indexed', np.array([0.0, 1.0])), IDX_SHAPE % ('augment_affine_indexed', '(2,)', 'float64'))
    _refused(_host_index, ('gather_batch', torch.zeros(2, 2, dtype=torch.int64)), IDX_SHAPE % ('gather_batch', '(2, 2)', 'int64'))
    _refused(_host_index, ('augment_affine_indexed', np.array([0, 2 ** 31], np.int64)), 'augment_affine_indexed: idx does not fit int32')
    _refused(_host_index, ('gather_batch', np.array([-2 ** 31 - 1], np.int64)), 'gather_batch: idx does not fit int32')


@pytest.mark.skipif(not torch.cuda.is_available(), reason='the one case that takes a tensor on a real device; the meta tensor above takes the same branch')
def test_host_index_refuses_a_device_tensor():
    _refused(_host_index, ('gather_batch', torch.zeros(3, dtype=torch.int32, device='cuda:0')), IDX_HOST % ('gather_batch', 'cuda:0'))


def test_host_index_passes():
    for given in (np.array([3, 0, 2 ** 31 - 1], np.int64), [3, 0, 3], np.arange(8, dtype=np.int32)[::2], torch.tensor([4, 1], dtype=torch.int64),
                  np.array([7], np.uint8)):
        idx = _host_index('gather_batch', given)
        assert isinstance(idx, np.ndarray) and idx.dtype == np.int32 and idx.ndim == 1 and idx.flags['C_CONTIGUOUS']
        assert idx.tolist() == np.asarray(given).tolist()
    same = np.array([5, 6], np.int32)
    assert _host_index('gather_batch', same) is same


def test_lift_and_drop():
    t3, t4 = torch.zeros(2, 3, 4), torch.zeros(5, 2, 3, 4)
    assert tuple(_lift(t3, 4, True).shape) == (1, 2, 3, 4) and _lift(t3, 4, True).data_ptr() == t3.data_ptr()
    assert _lift(t4, 4, True) is t4      # already of the full rank: left for the caller's shape check
    assert _lift(t3, 4, False) is t3 and _lift(t4, 4, False) is t4
    assert _lift(t3, 5, True) is t3      # two short: the caller's _chk names it
    assert _lift(None, 4, True) is None and _lift([1, 2], 4, True) == [1, 2]
    out = {'a': torch.arange(6.).view(1, 2, 3), 'b': torch.arange(4, dtype=torch.int32).view(1, 4)}
    assert _drop(out, False) is out
    one = _drop(out, True)
    assert list(one) == ['a', 'b'] and tuple(one['a'].shape) == (2, 3) and tuple(one['b'].shape) == (4,)
    assert one['a'].data_ptr() == out['a'].data_ptr() and torch.equal(one['b'], out['b'][0])
