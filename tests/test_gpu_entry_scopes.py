"""The profile scope of every entry point that launches through the shared scaffold (csrc/entry.h: timed_launch, arena_launch, and seq_launch on
top of them): with option "profile" on, one call files exactly one pair of events under the entry's name, and reading the name empties it.
bench.py and tools/ read these scopes by name, so the names below are literals, not taken from the library.  Every entry runs once at the
smallest shape it accepts; what it computes is held elsewhere (the test_gpu_* file of each kernel)."""
import numpy as np
import pytest
import torch

import joint_cnn_mrf_amd  # noqa: F401
from joint_cnn_mrf_amd import synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def eng():
    """One fp32 handle at --debug width with spatial-model parameters (torso_infer and pose_decode need them), profiling on."""
    from joint_cnn_mrf_amd.engine import Engine
    p = synth.make_pd_params(debug=True, bn='trained', conv6_gain=8.0)
    p.update(synth.make_sm_params(synth.synthetic_priors(), kind='trained'))
    e = Engine(device=0).load_params(p)
    e.set_option('profile', 1)
    yield e
    e.close()


def _f32(*shape):
    return torch.rand(*shape, device='cuda:0', dtype=torch.float32)


def _u8(*shape):
    return torch.randint(0, 256, shape, device='cuda:0', dtype=torch.uint8)


def _image():
    return np.arange(5 * 7 * 3, dtype=np.uint8).reshape(5, 7, 3)


def _torso_infer(e):
    e.torso_infer(_f32(1, 60, 90, 9))                                                          # the arena branch
    e.torso_infer(None, cells=torch.tensor([[30, 45]], device='cuda:0', dtype=torch.int32))    # the blobs at given cells


def _pose_decode(e):
    peaks = {'cells': torch.zeros(1, 9, 1, 2, device='cuda:0', dtype=torch.int32), 'count': torch.ones(1, 9, device='cuda:0', dtype=torch.int32)}
    e.pose_decode(_f32(1, 60, 90, 10), peaks)


def _seq_hm():
    return _f32(1, 2, 2, 3, 1)      # S = 1, T = 2, a 2 x 3 map, K = 1


# (scope, launches filed under it, the calls)
ENTRIES = [
    ('mirror_pairs', 1, lambda e: e.mirror_pairs(_f32(1, 2, 3, 1))),
    ('mirror_merge', 1, lambda e: e.mirror_merge(_f32(2, 2, 3, 2), group=2, perm=[1, 0])),
    ('hm_peaks', 1, lambda e: e.hm_peaks(_f32(1, 4, 5, 2), max_peaks=1)),
    ('det_curve', 1, lambda e: e.det_curve(torch.zeros(1, 2, 9, device='cuda:0', dtype=torch.int32), _f32(1, 4, 5, 10), [5.0])),
    ('fit_images', 1, lambda e: e.fit_images([_image()], out_hw=(8, 8))),
    ('fit_windows', 1, lambda e: e.fit_windows([_image()], [[0, 0, 0, 5, 7]], out_hw=(8, 8))),
    ('render_poses', 1, lambda e: e.render_poses([_image()], np.zeros((0, 8), np.int32))),
    ('synth_people', 1, lambda e: e.synth_people(np.zeros((1, 20), np.int32), np.zeros((0, 16), np.int32), 8, 8)),
    ('frame_shift', 1, lambda e: e.frame_shift(_u8(2, 16, 16, 3), (0, 0, 16, 16), search=1)),
    ('frame_flow', 1, lambda e: e.frame_flow(_u8(2, 16, 16, 3), (0, 0, 16, 16), np.array([[1], [0]], np.int32), search=1)),
    ('hm_flow_pool', 1, lambda e: e.hm_flow_pool(_f32(2, 2, 2, 1), torch.zeros(2, 2, 2, 2, 2, device='cuda:0', dtype=torch.int32), [1.0, 0.5])),
    ('torso_infer', 2, _torso_infer),
    ('pose_decode', 1, _pose_decode),
    ('conv1_fullres/act_summary', 1, lambda e: e.act_summary(_f32(1, 1, 1, 16), 'conv1_fullres', n_groups=1, pic_channel=7, n_pics=0)),
    ('seq_filter', 1, lambda e: e.seq_filter(_seq_hm(), 1.0, 0.1, radius=0)),
    ('seq_viterbi', 1, lambda e: e.seq_viterbi(_seq_hm(), 1.0, 0.1, radius=0)),
    ('seq_smooth', 1, lambda e: e.seq_smooth(_seq_hm(), 1.0, 0.1, radius=0)),
]


@pytest.mark.parametrize('scope,launches,calls', ENTRIES, ids=[s for s, _, _ in ENTRIES])
def test_one_call_files_one_pair_under_the_entrys_name(eng, scope, launches, calls):
    calls(eng)      # (no other case files under this name, so nothing is drained first)
    ms, n = eng.profile_read(scope)
    print('%s: %d launches, %.4f ms' % (scope, n, ms))
    assert n == launches, scope
    assert ms >= 0.0
    assert eng.profile_read(scope) == (0.0, 0), scope
