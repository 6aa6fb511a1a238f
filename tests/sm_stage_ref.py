"""Reference of the spatial model's training stage (jcm_train_sm_grads: main.py:528-531,539 and their backward pass), built on the restatement of
oracle/train_oracle.py -- spatial_model_train, _TfSoftmaxCE, _bn_train (inside spatial_model_train), update_moving -- and differentiated by autograd;
nothing of the model is restated here.

`sm_stage(..., dtype)`: torch.float64 is the reference, torch.float32 runs the SAME graph in float32.  The distance between the two modes is the
yardstick of tests/test_gpu_sm_stage.py (`bound` = train_stage_ref.bound: it comes from the reference alone, never from the kernels).
"""
import numpy as np
import torch

from oracle import train_oracle as T
from oracle.jcm_oracle import JOINT_DEPENDENCE, JOINT_NAMES, SM_DELTA
from oracle.jcm_oracle_torch import softplus5
from train_stage_ref import bound  # noqa: F401  (4 max|ref32 - ref64| + 2^-22 max|ref64| per tensor)

HM_H, HM_W = 60, 90


def is_sm_name(name):
    """The parameters the stage reads: energy_*, bias_*, bn_sm/*."""
    return name.startswith('energy_') or name.startswith('bias_') or name.startswith('bn_sm/')


def sm_params(params):
    return {k: v for k, v in params.items() if is_sm_name(k)}


def forward(prob, y, p):
    """prob [B,5400,K] torch (may carry a graph), y [B,5400,K+1] torch, p: torch parameters (train_oracle.to_torch) ->
    (ce [B,K], bn statistics {scope: (mean, unbiased var)}, T_min: the smallest argument of a pairwise log)."""
    B, HW, K = prob.shape
    hm10 = torch.cat([prob, y[:, :, K:]], dim=2).reshape(B, HM_H, HM_W, K + 1).permute(0, 3, 1, 2)      # main.py:528
    stats, convs = {}, []
    inner = T.conv_mrf_t

    def recording(prior, lik):      # the pairwise terms as spatial_model_train itself forms them, in its pair order
        out = inner(prior, lik)
        convs.append(out.detach())
        return out

    T.conv_mrf_t = recording
    try:
        logits = T.spatial_model_train(hm10, p, stats, K)
    finally:
        T.conv_mrf_t = inner
    ce = T._TfSoftmaxCE.apply(logits.reshape(B, K, -1), y[:, :, :K].permute(0, 2, 1))                   # main.py:539, per (image, joint)
    pairs = [(j, c) for j in JOINT_NAMES[:K] for c in JOINT_DEPENDENCE[j]]
    assert len(pairs) == len(convs)
    with torch.no_grad():
        t_min = min(float((r + softplus5(p['bias_%s_%s' % jc])[0, :, :, 0] + SM_DELTA).min()) for jc, r in zip(pairs, convs))
    return ce, stats, t_min


def _t(a, dtype):
    return torch.as_tensor(np.ascontiguousarray(a)).to(dtype)


def loss(pd_prob, y, params, gscale, dtype=torch.float64):
    """gscale * sum of the cross-entropies, forward only."""
    with torch.no_grad():
        p = {k: _t(v, dtype) for k, v in sm_params(params).items()}
        return float(forward(_t(pd_prob, dtype), _t(y, dtype), p)[0].sum()) * gscale


def softmax_chain(prob, g):
    """The gradient through prob = softmax over the map's pixels (axis 1): prob * (g - sum_px prob * g)."""
    return prob * (g - (prob * g).sum(dim=1, keepdim=True))


def sm_stage(pd_prob, y, params, gscale, dlog_in=None, dtype=torch.float64):
    """pd_prob [B,5400,K], y [B,5400,K+1], params (numpy dict holding the spatial-model parameters), dlog_in [B,5400,>=K] or None.
    -> dict: ce [B,K]; grads {name: flat array} of gscale * sum(ce) for every energy_* / bias_* and bn_sm gamma / beta; dprob = d / d pd_prob;
    dlog [B,5400,K] = dlog_in[..., :K] + pd_prob * (dprob - sum_px pd_prob * dprob); moving {name: array} after the call; t_min."""
    p = T.to_torch(sm_params(params), dtype)
    prob = _t(pd_prob, dtype).requires_grad_(True)
    ce, stats, t_min = forward(prob, _t(y, dtype), p)
    names = [k for k in sorted(p) if p[k].requires_grad]
    gs = torch.autograd.grad(ce.sum() * torch.tensor(gscale, dtype=dtype), [prob] + [p[k] for k in names])
    K = prob.shape[2]
    dlog = softmax_chain(prob.detach(), gs[0])
    if dlog_in is not None:
        dlog = _t(np.asarray(dlog_in)[:, :, :K], dtype) + dlog
    npd = np.float64 if dtype == torch.float64 else np.float32
    moving = T.update_moving(params, {k: (m.numpy(), v.numpy()) for k, (m, v) in stats.items()})
    return dict(ce=ce.detach().numpy(), grads={k: g.numpy().reshape(-1) for k, g in zip(names, gs[1:])}, dprob=gs[0].numpy(), dlog=dlog.numpy(),
                moving={k: v.astype(npd) for k, v in moving.items()}, t_min=t_min)
