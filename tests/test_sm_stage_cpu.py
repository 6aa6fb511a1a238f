"""tests/sm_stage_ref.py -- the reference of the spatial model's training stage that tests/test_gpu_sm_stage.py holds the kernels to -- checked by
itself, without a GPU, at B = 1: its dlog is the gradient through the spatial softmax, its cross-entropy gradient is TF's softmax - labels also where
a target map does not sum to one, and its gradients agree with a central difference of its own loss."""
import numpy as np
import pytest
import torch

import joint_cnn_mrf_amd  # noqa: F401
import sm_stage_ref as R
from joint_cnn_mrf_amd import synth
from oracle import train_oracle as T
from oracle.jcm_oracle import JOINT_NAMES

K = 9
GSCALE = 1.0 / K
CLIPPED = 4      # the joint whose blob sits on the map corner


@pytest.fixture(scope='module')
def params():
    return synth.make_sm_params(synth.synthetic_priors(), kind='trained')


def _logits(seed):
    return 3.0 * np.random.RandomState(seed).standard_normal((1, 5400, K))


def _targets(clip):
    y = synth.make_targets(1).astype(np.float64)
    if clip:      # the 3x3 blob centred on pixel (0, 0): its lower right 2x2 part is inside the map
        y[0, :, :, CLIPPED] = 0
        y[0, :2, :2, CLIPPED] = np.outer([2, 1], [2, 1]) / 16.0
    return y.reshape(1, 5400, K + 1)


@pytest.fixture(scope='module')
def clipped_case(params):
    """z, y with one clipped target map, the reference on softmax(z), and the same graph built here from the leaf z (kept for further backward passes)."""
    z, y = _logits(3), _targets(True)
    zt = torch.as_tensor(z).requires_grad_(True)
    prob = torch.softmax(zt, dim=1)
    ref = R.sm_stage(prob.detach().numpy(), y, params, GSCALE)
    p = T.to_torch(R.sm_params(params))
    ce, _, _ = R.forward(prob, torch.as_tensor(y), p)
    return dict(y=y, zt=zt, prob=prob, p=p, ce=ce, ref=ref)


def test_dlog_is_autograd_through_the_spatial_softmax(clipped_case):
    """Composition: the reference forms dlog = p (g - sum_px p g) from g = d/d pd_prob; autograd taken straight through softmax(z) w.r.t. z gives the
    same tensor to float64 rounding."""
    c = clipped_case
    dz, = torch.autograd.grad(c['ce'].sum() * GSCALE, [c['zt']], retain_graph=True)
    dz, dlog = dz.numpy(), c['ref']['dlog']
    assert np.abs(c['ce'].detach().numpy() - c['ref']['ce']).max() <= 1e-12 * np.abs(c['ref']['ce']).max()
    assert np.abs(dlog).max() > 0 and np.abs(dlog - dz).max() <= 1e-11 * np.abs(dz).max()


def test_clipped_target_takes_tfs_gradient(clipped_case):
    """The clipped map sums to 9/16.  The reference's bias gradients (the cheapest tensors behind the spatial model's logits: no convolution lies
    between) equal the backward pass of gscale (softmax - labels) pushed in at the logits -- TF's backprop -- for every joint; the exact derivative of
    the loss, gscale (sum(labels) softmax - labels), gives the same gradients for the whole maps and different ones for the clipped map."""
    c = clipped_case
    y = torch.as_tensor(c['y'])
    labels = y[:, :, :K].permute(0, 2, 1)
    s = labels.sum(dim=2)
    assert abs(float(s[0, CLIPPED]) - 9.0 / 16.0) < 1e-15 and all(abs(float(s[0, j]) - 1) < 1e-15 for j in range(K) if j != CLIPPED)
    # the graph down to the logits, once more: R.forward keeps them to itself
    hm10 = torch.cat([c['prob'].detach(), y[:, :, K:]], dim=2).reshape(1, R.HM_H, R.HM_W, K + 1).permute(0, 3, 1, 2)
    logits = T.spatial_model_train(hm10, c['p'], {}, K).reshape(1, K, -1)
    names = [k for k in sorted(c['p']) if k.startswith('bias_')]
    leaves = [c['p'][k] for k in names]
    sm = torch.softmax(logits, dim=2).detach()
    tf = torch.autograd.grad(logits, leaves, grad_outputs=GSCALE * (sm - labels), retain_graph=True)
    exact = torch.autograd.grad(-(labels * torch.log_softmax(logits, dim=2)).sum() * GSCALE, leaves)
    for k, a, b in zip(names, tf, exact):
        want = c['ref']['grads'][k]
        a, b = a.numpy().reshape(-1), b.numpy().reshape(-1)
        scale = np.abs(want).max()
        assert scale > 0 and np.abs(a - want).max() <= 1e-11 * scale, k
        if k.startswith('bias_%s_' % JOINT_NAMES[CLIPPED]):
            assert np.abs(b - want).max() >= 1e-2 * scale, '%s: the exact derivative should differ on the clipped map' % k
        else:
            assert np.abs(b - want).max() <= 1e-11 * scale, k


def test_central_difference_agrees_with_autograd(params):
    """One direction over ALL 164 parameter tensors and pd_prob (each tensor's part drawn N(0, 1) times the tensor's rms), targets that sum to one (there
    TF's gradient is the derivative): (L(+h) - L(-h)) / 2h against sum <grad, direction>.  Measured: inner product 0.363737, estimate 0.36373726
    at h = 1e-4 (off by 7.1e-7 of it) and 0.36373706 at h = 5e-5 (1.8e-7: the O(h^2) term; rounding of the loss, 1e-15 / h, is far below): halving
    the step moves the estimate by 5.3e-7 of the value, the asserted tolerance is 1e-5 of it for both steps."""
    y = _targets(False)
    z = _logits(4)
    prob = np.exp(z - z.max(axis=1, keepdims=True))
    prob /= prob.sum(axis=1, keepdims=True)
    ref = R.sm_stage(prob, y, params, GSCALE)
    rs = np.random.RandomState(5)
    names = sorted(ref['grads'])
    assert len(names) == 81 + 81 + 2
    d = {k: rs.standard_normal(np.asarray(params[k]).shape) * np.sqrt(np.mean(np.asarray(params[k], np.float64) ** 2)) for k in names}
    dp = rs.standard_normal(prob.shape) * np.sqrt(np.mean(prob ** 2))
    inner = sum(float((ref['grads'][k] * d[k].reshape(-1)).sum()) for k in names) + float((ref['dprob'] * dp).sum())

    def at(s):
        q = dict(params)
        q.update({k: np.asarray(params[k], np.float64) + s * d[k] for k in names})
        return R.loss(prob + s * dp, y, q, GSCALE)

    est = [(at(h) - at(-h)) / (2 * h) for h in (1e-4, 5e-5)]
    print('inner %.8g  estimates %.8g %.8g  rel %.3e %.3e  moved %.3e' % (inner, est[0], est[1], (est[0] - inner) / inner, (est[1] - inner) / inner,
                                                                      (est[1] - est[0]) / inner))
    assert abs(inner) > 0.1
    assert abs(est[1] - est[0]) < 1e-5 * abs(inner)
    assert abs(est[0] - inner) <= 1e-5 * abs(inner) and abs(est[1] - inner) <= 1e-5 * abs(inner)
