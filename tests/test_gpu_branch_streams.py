"""jcm_pd_forward runs the half- and quarter-resolution branches on the handle's side stream, beside the full-resolution branch (option "fft_fuse"
bit 2, default on; csrc/pd_tower.hip: SideBranches).  The kernels and their arguments are those of the one-stream order (fft_fuse = 3), so every
output is the same BITS: all comparisons here are np.array_equal between fft_fuse = 7 and fft_fuse = 3, no tolerance."""
import numpy as np
import pytest
import torch

from golden_util import full_inputs
from joint_cnn_mrf_amd import synth

pytestmark = pytest.mark.gpu

SERIAL, BESIDE = 3, 7


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32), device='cuda:0')


@pytest.fixture(scope='module')
def debug_params():
    """--debug widths at which every hand-over and the tiles are taken (tests/test_gpu_golden.py), with a spatial model."""
    p = synth.make_pd_params(debug=True, bn='trained', conv6_gain=8.0)
    p.update(synth.make_sm_params(synth.synthetic_priors(), kind='trained'))
    return p


def engine(p, fuse, **kw):
    from joint_cnn_mrf_amd.engine import Engine
    return Engine(device=0, fft_fuse=fuse, **kw).load_params(p)


def outputs(eng, x, torso):
    """model() logits, and forward(use_sm=True)'s probabilities and both coordinate sets, as numpy arrays"""
    out = {'logits': eng.model(x).cpu().numpy()}
    out.update({k: v.cpu().numpy() for k, v in eng.forward(x, torso, use_sm=True).items()})
    assert sorted(out) == ['logits', 'pd_coords', 'pd_prob', 'sm_coords', 'sm_prob']
    return out


def assert_same(got, want, what):
    for k in want:
        assert np.array_equal(got[k], want[k]), (what, k, float(np.abs(got[k].astype(np.float64) - want[k]).max()))


def test_default_has_the_bit_set():
    from joint_cnn_mrf_amd.engine import Engine
    eng = Engine(device=0)
    assert eng.get_option('fft_fuse') == BESIDE
    eng.close()


def test_model_geometry_fp32(debug_params):
    """2 images at 480 x 720: the smallest input at which every hand-over and the tiles are taken.  Three consecutive calls on one handle reuse the side
    arena and the side stream's scale words between calls; then the option goes to 3 and back to 7 on the same handle."""
    x, torso = dev(synth.make_images(2)), dev(synth.make_torso(2))
    ser = engine(debug_params, SERIAL)
    want = outputs(ser, x, torso)
    ser.close()
    assert np.abs(want['logits']).max() > 0
    eng = engine(debug_params, BESIDE)
    for i in range(3):
        assert_same(outputs(eng, x, torso), want, 'call %d' % i)
    for fuse in (SERIAL, BESIDE):
        eng.set_option('fft_fuse', fuse)
        assert_same(outputs(eng, x, torso), want, 'fft_fuse = %d on the same handle' % fuse)
    eng.close()


def test_micro_batch_loop_with_a_ragged_tail(debug_params):
    """5 images in slices of 2: every slice forks behind the previous slice's work, which is what orders the reuse of the side arena."""
    x, torso = dev(synth.make_images(5, seed=41)), dev(synth.make_torso(5, seed=42))
    got = {}
    for fuse in (SERIAL, BESIDE):
        eng = engine(debug_params, fuse, micro_batch=2)
        got[fuse] = {k: v.cpu().numpy() for k, v in eng.forward(x, torso, use_sm=True).items()}
        eng.close()
    assert_same(got[BESIDE], got[SERIAL], 'micro_batch = 2')
    assert np.abs(got[SERIAL]['pd_prob'][4]).max() > 0


@pytest.mark.parametrize('hw', [(200, 296), (240, 360)])
def test_other_geometries(debug_params, hw):
    """The resize path in front of the coarse branches, odd pooled maps, and the separate merge kernel behind the join."""
    x = dev(synth.make_images(2, seed=31, height=hw[0], width=hw[1]))
    got = {}
    for fuse in (SERIAL, BESIDE):
        eng = engine(debug_params, fuse)
        got[fuse] = [eng.model(x).cpu().numpy() for _ in range(2)]
        eng.close()
    assert np.abs(got[SERIAL][0]).max() > 0
    for g in got[BESIDE]:
        assert np.array_equal(g, got[SERIAL][0])


def test_bf16_handle():
    """The goldens' full-width parameters, 2 images at 480 x 720."""
    x2, torso2, p = full_inputs()
    p = dict(p)
    p.update(synth.make_sm_params(synth.synthetic_priors(), kind='trained'))
    x, torso = dev(x2), dev(torso2)
    got = {}
    for fuse in (SERIAL, BESIDE):
        eng = engine(p, fuse, precision='bf16')
        got[fuse] = [outputs(eng, x, torso) for _ in range(2)]
        eng.close()
    assert np.abs(got[SERIAL][0]['logits']).max() > 0
    for g in got[BESIDE]:
        assert_same(g, got[SERIAL][0], 'bf16')


def test_profiling_events_of_the_side_stream_are_readable(debug_params):
    """set_profile(True): conv4_halfres is bracketed by events on the side stream, conv4_fullres on the handle's own; each is one launch with a time."""
    x = dev(synth.make_images(2))
    eng = engine(debug_params, BESIDE)
    eng.model(x)                  # (first-use packing of the filter spectra stays out of the timed call)
    eng.set_profile(True)
    eng.model(x)
    for scope in ('conv4_halfres', 'conv4_fullres'):
        ms, n = eng.profile_read(scope)
        assert n == 1 and ms > 0, (scope, ms, n)
    eng.set_profile(False)
    eng.close()
