"""Training-time augmentation on the GPU (csrc/augment.hip behind jcm_augment_train) against the float32 step-by-step
restatement (tests/augment_ref.py (a); to the last bit but for powf and the float32 rounding of a double sum) and the
float64 formulation ((b), scipy's bilinear for the rotation), and its integration into Trainer / TowerTrainer."""

import numpy as np
import pytest
import torch

import augment_ref as A
import joint_cnn_mrf_amd  # noqa: F401
from joint_cnn_mrf_amd import _lib, augmentation, synth

pytestmark = pytest.mark.gpu

f32 = np.float32
PI9 = float(f32(np.pi / 9))


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), device='cuda:0')


def engine(**kw):
    from joint_cnn_mrf_amd.engine import Engine
    return Engine(device=0, **kw)


def edge_params(B, seed=5):
    """draw_params rows, the first four replaced by the edges of the parameter ranges."""
    p = augmentation.draw_params(np.random.RandomState(seed), B)
    edges = np.array([[0, 0.0, 1.0, PI9, 0.0, 0.0],
                      [1, 0.0, 1.0, -PI9, 0.05, 0.05],
                      [1, 32 / 255, 1.2, 0.0, 0.0, 0.05],
                      [0, -32 / 255, 0.8, PI9, 0.05, 0.0]], f32)
    n = min(B, len(edges))
    p[:n] = edges[:n]
    return p


def inputs(B, H, W, h, w, seed=0):
    rs = np.random.RandomState(seed)
    return rs.random_sample((B, H, W, 3)).astype(f32), rs.random_sample((B, h, w, 10)).astype(f32)


def check_against_refs(x, y, p):
    eng = engine()
    xg, yg = augmentation.augment_train(eng, dev(x), dev(y), p)
    xg, yg = xg.cpu().numpy(), yg.cpu().numpy()
    eng.close()
    xa, ya = A.augment_f32(x, y, p)
    assert np.abs(xg - xa).max() <= 1e-6
    np.testing.assert_allclose(yg, ya, rtol=1e-5, atol=1e-12)
    xb, yb = A.augment_f64(x, y, p)
    assert np.abs(xg - xb).max() <= 1e-5
    assert (np.abs(yg - yb) / np.abs(yb).max(axis=(1, 2), keepdims=True)).max() <= 1e-4
    assert xg.min() >= 0 and xg.max() <= 1
    np.testing.assert_allclose(yg.astype(np.float64).sum(axis=(1, 2)), 1.0, atol=1e-5)
    return xg, yg


def test_full_size_against_both_restatements():
    x, y = inputs(16, 480, 720, 60, 90)
    check_against_refs(x, y, edge_params(16))


def test_small_odd_geometry():
    x, y = inputs(5, 37, 53, 7, 11, seed=1)
    check_against_refs(x, y, edge_params(5, seed=6))


def test_deterministic_and_independent_per_image():
    x, y = inputs(16, 480, 720, 60, 90, seed=2)
    p = edge_params(16, seed=7)
    eng = engine()
    xd, yd, pd = dev(x), dev(y), dev(p)
    a = eng.augment_train(xd, yd, pd)
    b = eng.augment_train(xd, yd, pd)
    lo = eng.augment_train(xd[:8].contiguous(), yd[:8].contiguous(), pd[:8].contiguous())
    hi = eng.augment_train(xd[8:].contiguous(), yd[8:].contiguous(), pd[8:].contiguous())
    for k in range(2):
        assert torch.equal(a[k], b[k])
        assert torch.equal(a[k], torch.cat([lo[k], hi[k]]))
    eng.close()


def test_fp32_and_bf16_handles_agree_bit_for_bit():
    x, y = inputs(4, 480, 720, 60, 90, seed=3)
    p = edge_params(4, seed=8)
    e32, e16 = engine(precision='fp32'), engine(precision='bf16')
    a = augmentation.augment_train(e32, dev(x), dev(y), p)
    b = augmentation.augment_train(e16, dev(x), dev(y), p)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    e32.close()
    e16.close()


def test_entry_point_rejects_bad_arguments():
    lib = _lib.load()
    eng = engine()
    x, y = dev(np.zeros((2, 8, 8, 3), f32)), dev(np.zeros((2, 4, 4, 10), f32))
    pd = dev(np.zeros((2, 6), f32))
    xo, yo = torch.empty_like(x), torch.empty_like(y)
    P = eng._p
    call = lambda h, xx, yy, B, H, W, hh, hw, xout, yout: lib.jcm_augment_train(h, P(xx), P(yy), P(pd), B, H, W, hh, hw, P(xout), P(yout))
    assert call(eng._h, x, y, 2, 8, 8, 4, 4, xo, yo) == 0
    torch.cuda.synchronize()
    assert call(eng._h, x, y, 2, 8, 8, 4, 4, x, yo) == 1                       # x_out is x
    assert call(eng._h, x, y, 2, 8, 8, 4, 4, xo, y) == 1                       # y_out is y
    assert call(eng._h, x, y, 2, 8, 8, 4, 4, xo, xo) == 1                      # the outputs overlap
    assert call(eng._h, x, y, 2, 8, 1, 4, 4, xo, yo) == 1                      # W < 2
    assert call(eng._h, x, y, 0, 8, 8, 4, 4, xo, yo) == 1                      # B < 1
    assert call(eng._h, x, None, 2, 8, 8, 4, 4, xo, yo) == 1                   # null input
    e5 = engine(n_joints=5)
    assert call(e5._h, x, y, 2, 8, 8, 4, 4, xo, yo) == 1                       # heat maps of 10 channels need n_joints == 9
    assert 'n_joints' in _lib.last_error()
    with pytest.raises(ValueError):
        augmentation.augment_train(eng, x, y, np.full((2, 6), np.nan, f32))
    e5.close()
    eng.close()


# ------------------------------------------------------------------ training step
@pytest.fixture(scope='module')
def debug_case():
    p = synth.make_pd_params(debug=True, bn='trained')
    p.update(synth.make_sm_params(synth.synthetic_priors(), kind='trained'))
    B = 4
    return p, synth.make_images(B), synth.make_targets(B)


def make_trainer(params):
    from joint_cnn_mrf_amd.train import Trainer
    eng = engine().load_params(params)
    return eng, Trainer(eng, use_sm=True, lmbd=0.001)


def test_trainer_augment_equals_training_on_the_augmented_batch(debug_case):
    params, x, y = debug_case
    x, y = x[:2], y[:2]
    p = edge_params(2, seed=9)
    ea, ta = make_trainer(params)
    eb, tb = make_trainer(params)
    plain_l, plain_g = [t.clone() for t in ta.loss_and_grads(dev(x), dev(y))]
    aug_l, aug_g = [t.clone() for t in ta.loss_and_grads(dev(x), dev(y), augment=p)]
    ref_l, ref_g = tb.loss_and_grads(*augmentation.augment_train(eb, dev(x), dev(y), p))
    assert torch.equal(aug_l, ref_l) and torch.equal(aug_g, ref_g)
    assert not torch.equal(aug_l, plain_l)
    again_l, again_g = ta.loss_and_grads(dev(x), dev(y))            # augment=None: the step of before, bit for bit
    assert torch.equal(again_l, plain_l) and torch.equal(again_g, plain_g)
    ea.close()
    eb.close()


def test_tower_trainer_draws_for_the_global_batch(debug_case):
    from joint_cnn_mrf_amd.dist import Towers
    from joint_cnn_mrf_amd.main import TowerTrainer
    params, x, y = debug_case
    B, seed = x.shape[0], 21
    towers = Towers(params, [0, 0])
    tt = TowerTrainer(towers, params, augment_rng=np.random.RandomState(seed), use_sm=True, lmbd=0.001)
    tt.train_step(x, y)
    got = [tr.losses.clone() for tr in tt.trainers]
    towers.close()
    p = augmentation.draw_params(np.random.RandomState(seed), B)
    for (lo, hi), g in zip(towers.slices(B), got):
        eng, tr = make_trainer(params)
        want = tr.loss_and_grads(dev(x[lo:hi]), dev(y[lo:hi]), augment=p[lo:hi])[0]
        assert torch.equal(g, want)
        eng.close()


def test_augment_from_the_gradient_ready_callback_is_refused(debug_case):
    params, x, y = debug_case
    x, y = x[:2], y[:2]
    eng, tr = make_trainer(params)
    tr.loss_and_grads(dev(x), dev(y))
    want = tr.grads.clone()
    p = edge_params(2)
    errors, calls = [], [0]

    def hook(offset, count):
        calls[0] += 1
        if calls[0] != 2:
            return
        try:
            augmentation.augment_train(eng, dev(x), dev(y), p)
            errors.append(None)
        except RuntimeError as e:
            errors.append(str(e))
    tr.set_ready_hook(hook)
    tr.loss_and_grads(dev(x), dev(y))
    tr.set_ready_hook(None)
    assert len(errors) == 1 and errors[0] is not None and 'status %d' % 2 in errors[0] and 'gradient-ready callback' in errors[0], errors
    assert torch.equal(tr.grads, want)
    eng.close()
