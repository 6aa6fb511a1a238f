"""The logits layer contracted on conv5's row spectra (option "fft_logits_rows", conv_fft_logits.hip).

conv6 behind conv5's row-transformed hand-over no longer runs as a whole frequency-domain layer: the 9 vertical taps and the input channels are
one fp16 matrix product per kx on the row spectra, with the SAME padding along y as explicit zero rows, and one inverse row pass finishes the
layer.  Both routes compute the same convolution through different arithmetic: they agree to rounding and both hold the float64 goldens."""
import numpy as np
import pytest
import torch

from golden_util import flic_priors, full_inputs, load, seeds
from joint_cnn_mrf_amd import synth
from oracle import jcm_oracle as O

pytestmark = pytest.mark.gpu


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _logits(x, p, rows, **kw):
    from joint_cnn_mrf_amd.engine import Engine
    eng = Engine(device=0, fft_logits_rows=rows, **kw).load_params(p)
    try:
        return eng.model(dev(x)).cpu().numpy()
    finally:
        eng.close()


def test_both_arms_vs_golden():
    from joint_cnn_mrf_amd.engine import Engine
    x, torso, p = full_inputs()
    p.update(synth.make_sm_params(flic_priors(), kind='trained', seed=seeds()['sm']))
    ref = load('full_pd_logits')
    scale = max(1.0, float(np.abs(ref).max()))
    got = {}
    for rows in (1, 0):
        eng = Engine(device=0, fft_logits_rows=rows).load_params(p)
        got[rows] = eng.model(dev(x)).cpu().numpy()
        r = eng.forward(dev(x), dev(torso), use_sm=True)
        eng.close()
        err = np.abs(got[rows] - ref)
        print('arm', rows, 'max err / scale', float(err.max()) / scale)
        assert err.max() <= 2e-4 * scale, (rows, float(err.max()))
        np.testing.assert_array_equal(r['pd_coords'].cpu().numpy(), load('full_pd_coords'))
        np.testing.assert_array_equal(r['sm_coords'].cpu().numpy(), load('full_sm_coords_trained'))
    d = np.abs(got[1] - got[0])
    print('arm to arm / scale', float(d.max()) / scale)
    assert d.max() <= 2e-5 * scale, float(d.max())
    assert not np.array_equal(got[1], got[0])      # the route is taken at the model's geometry (other arithmetic, other rounding)


def test_borders_vs_float64_oracle():
    """The padding along y is explicit zero rows now, and along x the 96-point transform must stay alias-free: image 0 has its content in the top and
    bottom 32 image rows (logits rows 0..3 and 56..59), image 1 in the left and right 32 columns (logits columns 0..3 and 86..89)."""
    x, _, p = full_inputs()
    x = x.copy()
    x[0] *= 0.05
    x[0, :32] = 1.0
    x[0, -32:] = 1.0
    x[1] *= 0.05
    x[1, :, :32] = 1.0
    x[1, :, -32:] = 1.0
    ref = O.model(x, p)
    scale = max(1.0, float(np.abs(ref).max()))
    got = _logits(x, p, 1)
    err = np.abs(got - ref)
    print('max err / scale', float(err.max()) / scale, 'rows', float(max(err[0, :4].max(), err[0, -4:].max())) / scale,
          'columns', float(max(err[1, :, :4].max(), err[1, :, -4:].max())) / scale)
    assert err.max() <= 2e-4 * scale, float(err.max())
    assert err[0, :4].max() <= 2e-4 * scale and err[0, -4:].max() <= 2e-4 * scale
    assert err[1, :, :4].max() <= 2e-4 * scale and err[1, :, -4:].max() <= 2e-4 * scale


def test_per_image_scale_and_batch_independence():
    """A work group is one (kx, image) under the image's own power-of-two scale: an image's result does not depend on its batch, not even next to an
    image 1e4 times brighter, and a ragged batch of 5 gives every image the bits it gets alone."""
    _, _, p = full_inputs()
    x = synth.make_images(5, seed=77)
    xb = x.copy()
    xb[2] *= 1e4
    alone = _logits(x[:1], p, 1)
    batch5 = _logits(x, p, 1)
    bright = _logits(xb, p, 1)
    assert np.array_equal(batch5[:1], alone)
    assert np.array_equal(bright[[0, 1, 3, 4]], batch5[[0, 1, 3, 4]])
    assert np.isfinite(bright).all()
    whole = _logits(xb, p, 0)
    s = max(1.0, float(np.abs(whole[2]).max()))
    print('bright image, arm to arm / scale', float(np.abs(bright[2] - whole[2]).max()) / s)
    assert np.abs(bright[2] - whole[2]).max() <= 2e-5 * s


@pytest.fixture(scope='module')
def small():
    p = synth.make_pd_params(debug=True, bn='trained', conv6_gain=8.0)      # conv6: 128 input channels = eight 16-channel chunks, one per wave
    x = synth.make_images(3, seed=41)
    return p, x, O.model(x, p)


@pytest.mark.parametrize('B', [1, 2, 3])
def test_small_channel_count(small, B):
    p, x, ref = small
    scale = max(1.0, float(np.abs(ref[:B]).max()))
    a1, a0 = _logits(x[:B], p, 1), _logits(x[:B], p, 0)
    print('B', B, 'arm 1 / 0 err', float(np.abs(a1 - ref[:B]).max()) / scale, float(np.abs(a0 - ref[:B]).max()) / scale, 'arm to arm', float(np.abs(a1 - a0).max()) / scale)
    assert np.abs(a1 - ref[:B]).max() <= 2e-4 * scale
    assert np.abs(a0 - ref[:B]).max() <= 2e-4 * scale
    assert np.abs(a1 - a0).max() <= 2e-5 * scale
    assert not np.array_equal(a1, a0)


@pytest.mark.parametrize('hw', [(240, 360), (256, 384)])
def test_other_geometries_keep_the_whole_route(hw):
    """Only a hand-over at 96-point rows is contracted: elsewhere the option changes nothing, bit for bit."""
    H, W = hw
    p = synth.make_pd_params(debug=True, bn='trained', conv6_gain=8.0)
    x = synth.make_images(2, seed=31, height=H, width=W)
    assert np.array_equal(_logits(x, p, 1), _logits(x, p, 0))


@pytest.mark.parametrize('kw', [{'precision': 'bf16'}, {'conv9_fft': 0}])
def test_other_handles_keep_their_route(kw):
    """bf16 handles (whose kernels need the full model's channel counts) and the direct fp32 chain never see the option."""
    p = full_inputs()[2] if 'precision' in kw else synth.make_pd_params(debug=True, bn='trained', conv6_gain=8.0)
    x = synth.make_images(2, seed=32)
    assert np.array_equal(_logits(x, p, 1, **kw), _logits(x, p, 0, **kw))


def test_operand_follows_the_parameters():
    """The operand is built from conv6's weights once per parameter load: other weights in the same engine give what a fresh engine gives."""
    from joint_cnn_mrf_amd.engine import Engine
    p = synth.make_pd_params(debug=True, bn='trained', conv6_gain=8.0)
    x = synth.make_images(2, seed=33)
    w2 = np.ascontiguousarray(p['conv6/weights'][::-1] * np.float32(0.5))
    eng = Engine(device=0, fft_logits_rows=1).load_params(p)
    try:
        first = eng.model(dev(x)).cpu().numpy()
        eng.update_tensor('conv6/weights', w2)
        second = eng.model(dev(x)).cpu().numpy()
    finally:
        eng.close()
    p2 = dict(p)
    p2['conv6/weights'] = w2
    assert np.array_equal(second, _logits(x, p2, 1))
    assert not np.array_equal(second, first)
