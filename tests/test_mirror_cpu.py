"""Mirrored test-time evaluation without a GPU: the numpy restatement (tests/mirror_ref.py) on hand-computed answers, the left/right channel table
(csrc/hm_flip.h, _lib.HM_FLIP_PERM) against the reference's random_flip concat and against tests/augment_ref.py, the window bookkeeping of the
16-copy order of multiscale.get_predictions(flip_test=True), and the --flip_test flag with its refusal."""
import inspect
import os
import re

import numpy as np
import pytest
from numpy.testing import assert_array_equal

import augment_ref
import mirror_ref as R
import joint_cnn_mrf_amd  # noqa: F401
from joint_cnn_mrf_amd import _lib, multiscale
from joint_cnn_mrf_amd import main as M

f32 = np.float32
RANDOM_FLIP_CONCAT = [3, 4, 5, 0, 1, 2, 7, 6, 8, 9]      # hm[:, :, 3:6], hm[:, :, 0:3], hm[:, :, 7:8], hm[:, :, 6:7], hm[:, :, 8:10] (augmentation.py:20)


# ------------------------------------------------------------------ the restatement on literals
def test_mirror_pairs_known_answer():
    x = np.arange(12, dtype=np.uint8).reshape(1, 2, 3, 2)      # rows [[0,1],[2,3],[4,5]] and [[6,7],[8,9],[10,11]]
    out = R.mirror_pairs(x)
    assert out.shape == (2, 2, 3, 2) and out.dtype == np.uint8
    assert_array_equal(out[0], x[0])
    assert out[1].tolist() == [[[4, 5], [2, 3], [0, 1]], [[10, 11], [8, 9], [6, 7]]]
    two = R.mirror_pairs(np.stack([x[0], x[0] + 100]))
    assert_array_equal(two[2], x[0] + 100)
    assert_array_equal(two[3], out[1] + 100)


def test_mirror_merge_known_answer_two_copies():
    """1 x 3 x K maps, K = 2, perm [1, 0]: out[x,k] = (a[x,k] + b[2-x,1-k]) / 2."""
    a = np.array([[[1, 2], [3, 4], [5, 6]]], f32)
    b = np.array([[[10, 20], [30, 40], [50, 60]]], f32)
    out = R.mirror_merge(np.stack([a, b]), 2, perm=[1, 0])
    assert out.dtype == f32 and out.shape == (1, 1, 3, 2)
    assert out[0, 0].tolist() == [[(1 + 60) / 2, (2 + 50) / 2], [(3 + 40) / 2, (4 + 30) / 2], [(5 + 20) / 2, (6 + 10) / 2]]


def test_mirror_merge_known_answer_flic_table():
    """K = 9 and perm None: the mirrored copy's channel 3 (right shoulder) lands on channel 0 (left shoulder), 7 on 6, 8 stays."""
    a = np.zeros((1, 3, 9), f32)
    b = np.zeros((1, 3, 9), f32)
    b[0, 0, 3] = 8      # leftmost pixel of the mirrored map, right shoulder
    b[0, 2, 7] = 4
    b[0, 1, 8] = 2
    out = R.mirror_merge(np.stack([a, b]), 2)
    want = np.zeros((1, 1, 3, 9), f32)
    want[0, 0, 2, 0] = 4      # (0 + 8) / 2 at the rightmost pixel, left shoulder
    want[0, 0, 0, 6] = 2
    want[0, 0, 1, 8] = 1
    assert_array_equal(out, want)


def test_mirror_merge_known_answer_four_copies_is_a_sequential_float64_sum():
    """G = 4 on one pixel, K = 1: float32((((1e8 + 1) + -1e8) + 1) / 4) = 0.5 -- a float32 sum would give 0.25 (1e8 + 1 rounds to 1e8)."""
    v = np.array([1e8, 1, -1e8, 1], f32).reshape(4, 1, 1, 1)
    assert R.mirror_merge(v, 4, perm=[0])[0, 0, 0, 0] == f32(0.5)
    big = np.full((2, 1, 1, 1), np.finfo(f32).max, f32)      # the sum is formed in double: no overflow on the way to the mean
    assert R.mirror_merge(big, 2, perm=[0])[0, 0, 0, 0] == np.finfo(f32).max


def test_merging_the_pairs_of_a_map_gives_a_symmetric_map():
    """mirror_merge of mirror_pairs-like input: copy 1 the mirror image (channels permuted) of copy 0 -> the result is copy 0 itself."""
    rng = np.random.RandomState(3)
    a = rng.rand(1, 4, 5, 9).astype(f32)
    mirrored = a[:, :, ::-1, :][..., R.HM_FLIP_PERM[:9]]
    assert_array_equal(R.mirror_merge(np.concatenate([a, mirrored]), 2), a)


# ------------------------------------------------------------------ the table
def _header_table(repo_root):
    text = open(os.path.join(repo_root, 'joint-cnn-mrf_amd', 'csrc', 'hm_flip.h')).read()
    m = re.search(r'kHmFlipPerm\[kHmFlipChannels\]\s*=\s*\{([^}]*)\}', text)
    assert m, 'csrc/hm_flip.h no longer defines kHmFlipPerm'
    return [int(v) for v in m.group(1).split(',')]


def test_table_is_the_reference_concat_and_an_involution(repo_root):
    table = _header_table(repo_root)
    assert table == RANDOM_FLIP_CONCAT
    assert list(_lib.HM_FLIP_PERM) == table and R.HM_FLIP_PERM == table
    assert [table[table[k]] for k in range(10)] == list(range(10))
    assert sorted(table[:9]) == list(range(9))      # cut to the nine joints it is still a permutation (the torso stays in place)
    names = list(M.joint_names)
    assert [names[k] for k in table] == ['rsho', 'relb', 'rwri', 'lsho', 'lelb', 'lwri', 'rhip', 'lhip', 'nose', 'torso']


def test_table_is_the_one_the_augmentation_restatement_uses(repo_root):
    assert augment_ref.HM_FLIP_PERM.tolist() == _header_table(repo_root)
    src = open(os.path.join(repo_root, 'joint-cnn-mrf_amd', 'csrc', 'augment.hip')).read()
    assert '#include "hm_flip.h"' in src and '__constant__ int kHmFlipPerm' not in src      # one copy of the table


# ------------------------------------------------------------------ the 16-copy order of the multi-scale wrapper
class _Recorder:
    """Stands in for the Engine: records the windows scale_hm_back asks for."""

    def window_resize(self, src, windows, oh, ow):
        self.windows = list(windows)
        return src


class _Maps:
    def __init__(self, n):
        self.shape = (n, 60, 90, 9)

    def contiguous(self):
        return self


def test_scale_hm_back_applies_one_window_to_both_members_of_a_pair():
    back = multiscale._back_windows(multiscale.PAD_ARRAY, multiscale.CROP_ARRAY, 60, 90)
    assert len(back) == 8
    rec = _Recorder()
    multiscale.scale_hm_back(rec, _Maps(16), multiscale.PAD_ARRAY, multiscale.CROP_ARRAY, 60, 90)      # as before: copy s of image i at i * 8 + s
    assert rec.windows == [(i,) + back[i % 8] for i in range(16)]
    multiscale.scale_hm_back(rec, _Maps(32), multiscale.PAD_ARRAY, multiscale.CROP_ARRAY, 60, 90, copies_per_scale=2)
    assert len(rec.windows) == 32
    for i in range(2):
        for s in range(8):
            for j in range(2):
                idx = i * 16 + 2 * s + j      # copy 2s + j of image i
                assert rec.windows[idx] == (idx,) + back[s]
    with pytest.raises(ValueError, match='multiple of 16'):
        multiscale.scale_hm_back(rec, _Maps(24), multiscale.PAD_ARRAY, multiscale.CROP_ARRAY, 60, 90, copies_per_scale=2)
    assert inspect.signature(multiscale.scale_hm_back).parameters['copies_per_scale'].default == 1


def test_some_back_windows_are_not_symmetric():
    """Why 'scale, then mirror' is the definition: the 90-wide map at 1/1.3 is cut as 10 | 69 | 11, so the window of scale s on a mirrored map
    covers other columns than the mirror image of that window."""
    back = multiscale._back_windows(multiscale.PAD_ARRAY, multiscale.CROP_ARRAY, 60, 90)
    y0, x0, h, w = back[2]      # pad 1.3
    assert (x0, w, 90 - x0 - w) == (10, 69, 11)
    asym = [s for s, (y0, x0, h, w) in enumerate(back) if 90 - x0 - w != x0]
    assert 2 in asym
    scale = multiscale._scale_windows(multiscale.PAD_ARRAY, multiscale.CROP_ARRAY, 480, 720)
    assert len(scale) == 8 and all(720 - x0 - w == x0 for (y0, x0, h, w) in scale)      # the image windows are symmetric: only the way back is not


# ------------------------------------------------------------------ the flag
def test_flag_defaults_and_signatures():
    a = M.build_parser().parse_args(['--use_sm'])
    assert a.flip_test is False
    assert M.build_parser().parse_args(['--flip_test', '--multiscale']).flip_test is True
    from joint_cnn_mrf_amd import dist, evaluation
    from joint_cnn_mrf_amd.engine import Engine
    for fn in (Engine.forward, dist.Towers.forward, evaluation.eval_curves, multiscale.get_predictions):
        assert inspect.signature(fn).parameters['flip_test'].default is False
    assert 'flip_test' not in inspect.signature(Engine.eval_forward).parameters      # its losses are defined on one copy


def test_flip_test_is_refused_with_train():
    with pytest.raises(SystemExit) as ei:
        M.main(['--train', '--flip_test', '--synthetic', '--debug'])
    assert ei.value.code == M.FLIP_TEST_IS_EVALUATION_ONLY and '--flip_test' in str(ei.value.code)
