"""The spatial model's training stage (sm_train_impl: the five kernels of csrc/sm_train.hip, the LDS transforms sm_lds_fwd_dframes / sm_lds_inv_frames,
the fused forward with its saved log arguments, bn_sm in training mode, softmax_ce / softmax_bwd around it) through its stand-alone entry point
jcm_train_sm_grads, against the float64 reference of tests/sm_stage_ref.py -- and the slice loop of its backward pass ("sm_chunk"), which no whole step
of the suite enters: every test elsewhere has B <= 32 = the default slice width.

Bound, per tensor: |got - ref64| <= 4 max|ref32 - ref64| + 2^-22 max|ref64| (train_stage_ref.bound; ref32 = the same reference in float32, never
the kernel).  Condition of the cases, asserted on the float64 reference: no pairwise log argument below 1e-2 (arguments near the 1e-6 floor are out of
scope here).  The two float64 references cost about 25 s of CPU each and are shared by every test of the module."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import joint_cnn_mrf_amd  # noqa: F401
import sm_stage_ref as R
from joint_cnn_mrf_amd import _lib, synth
from test_gpu_train import debug_case, make_trainer  # noqa: F401  (debug_case: the fixture)
from test_gpu_train_stages import NAN32, Guarded, _dev, _report, _same_bits

pytestmark = pytest.mark.gpu

K, HW = 9, 5400
MOVING = ('bn_sm/BatchNorm/moving_mean', 'bn_sm/BatchNorm/moving_variance')


@functools.lru_cache(maxsize=None)
def model_params():
    """Debug-width part detector beside the 'trained' synthetic spatial model; bn_sm's moving statistics start at ZERO, so that what the stage leaves in
    them is 0.1 x this batch's statistics (from the synthetic values near 1 the batch variance, ~1e-6, would be invisible in fp32)."""
    p = synth.make_pd_params(debug=True, bn='trained')
    p.update(synth.make_sm_params(synth.synthetic_priors(), kind='trained'))
    for k in MOVING:
        p[k] = np.zeros(10, np.float32)
    return p


@functools.lru_cache(maxsize=None)
def case(name):
    """'A': three images -- pd_prob = softmax over the map of 3 N(0,1) logits, of 12 N(0,1) (peaked) and of 0.1 N(0,1) (nearly flat) --, the targets
    of make_targets with joint 4 of image 1 moved onto the map corner (its 3x3 blob is clipped to 2x2: the map sums to 9/16), an incoming dlog that is
    seeded in channels 0..8 and NaN in channels 9..15.  'B': image 0 of A alone (one image's batch statistics).
    -> dict(prob, y, dlog_in, gscale, ref64, ref32)."""
    rs = np.random.RandomState(20)
    z = rs.standard_normal((3, HW, K)) * np.array([3.0, 12.0, 0.1])[:, None, None]
    prob = np.exp(z - z.max(axis=1, keepdims=True))
    prob = (prob / prob.sum(axis=1, keepdims=True)).astype(np.float32)
    y = synth.make_targets(3)
    y[1, :, :, 4] = 0
    y[1, :2, :2, 4] = np.outer([2, 1], [2, 1]).astype(np.float32) / 16
    y = y.reshape(3, HW, K + 1)
    dlog_in = np.full((3, HW, 16), np.nan, np.float32)
    dlog_in[:, :, :K] = (1e-3 * rs.standard_normal((3, HW, K))).astype(np.float32)
    if name == 'B':
        prob, y, dlog_in = prob[:1], y[:1], dlog_in[:1]
    B = prob.shape[0]
    gscale = float(np.float32(1.0 / (B * K)))
    p = model_params()
    c = dict(prob=prob, y=y, dlog_in=dlog_in, gscale=gscale, B=B)
    c['ref64'] = R.sm_stage(prob, y, p, gscale, dlog_in)
    c['ref32'] = R.sm_stage(prob, y, p, gscale, dlog_in, dtype=torch.float32)
    assert c['ref64']['t_min'] >= 1e-2, 'a pairwise log argument of %.3e: outside the range this module covers' % c['ref64']['t_min']
    return c


@pytest.fixture(scope='module')
def trainer():
    from joint_cnn_mrf_amd.engine import Engine
    from joint_cnn_mrf_amd.train import Trainer
    eng = Engine(device=0).load_params(model_params())
    yield Trainer(eng, use_sm=True)
    eng.close()


def stage_slices(tr):
    """[(name, offset, count)] of what the stage may write in the flat gradient buffer."""
    return [(n, o, c) for n, o, c in tr.layout if n.startswith('energy_') or n.startswith('bias_') or n in ('bn_sm/BatchNorm/gamma', 'bn_sm/BatchNorm/beta')]


def run_stage(tr, c):
    """jcm_train_sm_grads from the parameters' moving statistics into a guarded NaN ce_out, the guarded seeded dlog and a NaN gradient buffer: exactly
    the stage's slices of grads and channels 0..8 of dlog are written.  -> {name: float32 array} of every output."""
    e, p, B = tr.eng, model_params(), c['B']
    for k in MOVING:
        e.update_tensor(k, p[k], refresh=False)
    ce, dlog = Guarded((B, K)), Guarded((B, HW, 16), seed=c['dlog_in'])
    grads = torch.full((tr.n_elements,), float('nan'), dtype=torch.float32, device='cuda:0')
    pd, yd = _dev(c['prob']), _dev(c['y'])
    _lib.check(tr._lib.jcm_train_sm_grads(e._h, e._p(pd), e._p(yd), B, c['gscale'], e._p(ce.t), e._p(dlog.t), e._p(grads)), 'jcm_train_sm_grads')
    torch.cuda.synchronize()
    out = {'ce': ce.check('ce_out')}
    d = dlog.check('dlog', written=False)
    assert (d[:, :, K:].view(np.int32) == NAN32).all(), 'dlog: channels 9..15 were written'
    assert np.isfinite(d[:, :, :K]).all(), 'dlog: channels 0..8 hold non-finite values'
    out['dlog'] = d[:, :, :K].copy()
    g = grads.cpu().numpy()
    keep = np.ones(g.size, bool)
    sl = stage_slices(tr)
    assert len(sl) == 81 + 81 + 2
    for n, o, cnt in sl:
        keep[o:o + cnt] = False
        assert np.isfinite(g[o:o + cnt]).all(), '%s: unwritten or non-finite gradient entries' % n
        out[n] = g[o:o + cnt].copy()
    assert keep.sum() > 1000 and (g[keep].view(np.int32) == NAN32).all(), 'gradient elements outside the energy_* / bias_* / bn_sm slices were written'
    for k in MOVING:
        out[k] = tr.get_tensor(k, (10,))
    return out


def assert_same_bits(a, b, what):
    diff = [k for k in a if not _same_bits(a[k], b[k])]
    assert not diff, '%s: %d tensors differ, e.g. %s' % (what, len(diff), diff[:4])


@pytest.mark.parametrize('name', ['A', 'B'])
def test_sm_stage_vs_float64(trainer, name):
    """Default slice width.  ce_out, each of the 81 energy and 81 bias gradients on its own, bn_sm's gamma and beta gradients, dlog channels 0..8 (on top
    of its seed) and both moving statistics against the float64 reference, each to `bound`; the guards of run_stage; a second call from the same moving
    statistics is bit-identical.
    Achieved on an MI355X (printed by -s; the bound is NOT derived from these), worst err / max|ref64| and worst err / bound, case A | case B:
      energy_*          2.7e-6, 0.032 | 1.4e-6, 0.115        bias_*            2.9e-6, 0.036 | 2.5e-6, 0.164
      bn_sm gamma       3.3e-7, 0.002 | 2.3e-7, 0.001        bn_sm beta        3.9e-7, 0.003 | 4.1e-7, 0.001
      ce_out            3.4e-7, 0.010 | 2.3e-7, 0.011        dlog              1.3e-6, 0.008 | 1.4e-6, 0.012
      moving_mean       2.8e-7, 0.52  | 2.8e-7, 0.79         moving_variance   2.7e-7, 0.29  | 2.4e-7, 0.27
    (the moving statistics' bound is its 2^-22 max|ref| floor plus little: the float32 mode of the reference is nearly exact there)."""
    c = case(name)
    got = run_stage(trainer, c)
    assert_same_bits(got, run_stage(trainer, c), 'a second identical call')
    r64, r32 = c['ref64'], c['ref32']
    pairs = [('ce', got['ce'], r32['ce'], r64['ce']), ('dlog', got['dlog'], r32['dlog'], r64['dlog'])]
    pairs += [(n, got[n], r32['grads'][n], r64['grads'][n]) for n, _, _ in stage_slices(trainer)]
    pairs += [(k.split('/')[-1], got[k], r32['moving'][k], r64['moving'][k]) for k in MOVING]
    worst = {}
    bad = []
    for pr in pairs:
        try:
            rel = _report('sm stage ' + name, [pr])[pr[0]]
        except AssertionError as err:
            bad.append(str(err))
            continue
        ratio = float(np.abs(np.asarray(pr[1], np.float64).reshape(np.shape(pr[3])) - pr[3]).max()) / R.bound(pr[2], pr[3])
        cls = pr[0].split('_')[0] if pr[0].startswith(('energy_', 'bias_')) else pr[0]
        w = worst.get(cls, (0.0, 0.0))
        worst[cls] = (max(w[0], rel), max(w[1], ratio))
    for cls, (rel, ratio) in sorted(worst.items()):
        print('  sm stage %s worst %-26s err / max|ref| %.2e   err / bound %.3f' % (name, cls, rel, ratio))
    assert not bad, '\n'.join(bad)


def test_sm_stage_slices_are_bit_identical(trainer):
    """Case A on ONE handle with sm_chunk = 32, 1, 2, 3, 32 in turn (the slice buffers of the arena shrink, then grow): one pass; three slices of one
    image (b0 offsets, both accumulate arms twice); a full slice and a short last one (nb < Bc); Bc == B; and the first width again.  Every output of
    every run equals the first bit for bit: per-image work does not depend on the slice, and the sums over images in sm_bwd_dbias_kernel and
    sm_bwd_spec_da_kernel add image b to the stored float in the same order b = 0, 1, 2 whatever the slicing (the library is built with
    -ffp-contract=off).  The first run is held to float64 by test_sm_stage_vs_float64."""
    c = case('A')
    e = trainer.eng
    first = None
    try:
        for chunk in (32, 1, 2, 3, 32):
            e.set_option('sm_chunk', chunk)
            got = run_stage(trainer, c)
            if first is None:
                first = got
            assert_same_bits(first, got, 'sm_chunk = %d against the first run' % chunk)
    finally:
        e.set_option('sm_chunk', 32)


def test_step_with_sliced_spatial_model(debug_case):      # noqa: F811
    """The joint step of test_gpu_train.py's debug_case (debug width, two 480x720 images) with sm_chunk = 1: the losses and every tensor of
    grads_dict() equal those of a handle with the default slice width, bit for bit."""
    p, x, y = debug_case
    x, y = _dev(x), _dev(y)
    res = []
    for chunk in (None, 1):
        eng, tr = make_trainer(p, use_sm=True, lmbd=0.001)
        if chunk is not None:
            eng.set_option('sm_chunk', chunk)
        assert eng.get_option('sm_chunk') == (32 if chunk is None else chunk)
        losses, _ = tr.loss_and_grads(x, y)
        res.append(dict(tr.grads_dict(), losses=losses.cpu().numpy()))
        eng.close()
    assert np.isfinite(res[0]['losses']).all() and any(res[0][k].any() for k in res[0] if k.startswith('energy_'))
    assert_same_bits(res[0], res[1], 'the step with sm_chunk = 1 against the default')


def test_sm_stage_refusals(trainer):
    """The argument and state checks of jcm_train_sm_grads, by their messages, and that a refused call wrote nothing: ce_out, dlog and grads keep
    their NaN, bn_sm's moving statistics their values."""
    from joint_cnn_mrf_amd.engine import Engine
    from joint_cnn_mrf_amd.train import Trainer
    c = case('B')
    p = model_params()
    pd, yd = _dev(c['prob']), _dev(c['y'])

    def refused(tr_or_eng, match, pd=pd, yd=yd, B=1, null=None, wrapper=False):
        e = getattr(tr_or_eng, 'eng', tr_or_eng)
        ce, dlog = Guarded((1, K)), Guarded((1, HW, 16))
        grads = torch.full((4096,) if not hasattr(tr_or_eng, 'n_elements') else (tr_or_eng.n_elements,), float('nan'), dtype=torch.float32, device='cuda:0')
        args = dict(pd=pd, yd=yd, ce=ce.t, dlog=dlog.t, grads=grads)
        if null:
            args[null] = None
        with pytest.raises(RuntimeError, match=match):
            _lib.check(e._lib.jcm_train_sm_grads(e._h, e._p(args['pd']), e._p(args['yd']), B, ctypes.c_float(c['gscale']), e._p(args['ce']), e._p(args['dlog']),
                                                 e._p(args['grads'])), 'jcm_train_sm_grads')
        torch.cuda.synchronize()
        for what, t in (('ce_out', ce.full), ('dlog', dlog.full), ('grads', grads)):
            assert (t.cpu().numpy().view(np.int32) == NAN32).all(), '%s was written by a refused call (%s)' % (what, match)

    # ---- arguments, on the handle that would otherwise run the call
    for k in MOVING:
        trainer.eng.update_tensor(k, p[k] + np.float32(0.25), refresh=False)
    for null in ('pd', 'yd', 'ce', 'dlog', 'grads'):
        refused(trainer, 'bad train_sm_grads arguments', null=null)
    for B in (0, -3):
        refused(trainer, 'bad train_sm_grads arguments', B=B)
    # ---- from the gradient-ready callback of the same handle's running step
    errors = []

    def hook(offset, count):
        if errors:
            return
        try:
            refused(trainer, 'gradient-ready callback')
            errors.append(None)
        except BaseException as err:      # noqa: BLE001 -- reported after the step
            errors.append(err)
    trainer.set_ready_hook(hook)
    trainer.loss_and_grads(_dev(synth.make_images(1)), _dev(synth.make_targets(1)))
    trainer.set_ready_hook(None)
    assert errors == [None], errors
    for k in MOVING:
        trainer.eng.update_tensor(k, p[k] + np.float32(0.25), refresh=False)      # (the step itself moved them)
    refused(trainer, 'bad train_sm_grads arguments', B=0)
    for k in MOVING:
        assert np.array_equal(trainer.get_tensor(k, (10,)), p[k] + np.float32(0.25)), '%s moved by a refused call' % k
        trainer.eng.update_tensor(k, p[k], refresh=False)
    # ---- state: no jcm_train_begin; no spatial-model parameters; five joints
    pd_only = {k: v for k, v in p.items() if not R.is_sm_name(k)}
    eng = Engine(device=0).load_params(p)
    refused(eng, 'jcm_train_begin has not been called')
    eng.close()
    eng = Engine(device=0).load_params(pd_only)
    refused(Trainer(eng, use_sm=False), 'needs the spatial-model parameters')
    eng.close()
    p5 = synth.make_pd_params(debug=True, bn='trained', n_joints=5)
    p5.update(synth.make_sm_params(synth.synthetic_priors(), kind='trained', n_joints=5))
    eng = Engine(device=0, n_joints=5).load_params(p5)
    tr5 = Trainer(eng, use_sm=True)
    refused(tr5, 'defined for 9 joints')
    with pytest.raises(ValueError, match='pd_prob must be'):
        tr5.sm_grads(pd, yd)
    eng.close()


def test_trainer_sm_grads_is_the_entry_point(trainer):
    """Trainer.sm_grads: the same bits as the raw call (gscale given; dlog given), its shape checks, and the defaults (gscale = 1 / (B K), dlog added
    to zeros)."""
    c = case('B')
    want = run_stage(trainer, c)
    p = model_params()
    for k in MOVING:
        trainer.eng.update_tensor(k, p[k], refresh=False)
    dlog = _dev(np.nan_to_num(c['dlog_in']))
    ce, out = trainer.sm_grads(_dev(c['prob']), _dev(c['y']), gscale=c['gscale'], dlog=dlog)
    assert out is dlog and _same_bits(ce.cpu().numpy(), want['ce']) and _same_bits(dlog.cpu().numpy()[:, :, :K].copy(), want['dlog'])
    assert not dlog[:, :, K:].any()
    got = trainer.grads_dict()
    for n, _, _ in stage_slices(trainer):
        assert _same_bits(got[n], want[n]), n
    for k in MOVING:
        trainer.eng.update_tensor(k, p[k], refresh=False)
    ce2, d2 = trainer.sm_grads(_dev(c['prob']), _dev(c['y']))
    assert tuple(d2.shape) == (1, HW, 16) and _same_bits(ce2.cpu().numpy(), want['ce'])
    seedless = want['dlog'].astype(np.float64) - c['dlog_in'][:, :, :K]
    assert np.abs(d2.cpu().numpy()[:, :, :K] - seedless).max() <= 2.0 ** -22 * np.abs(want['dlog']).max()
    with pytest.raises(ValueError, match='pd_prob must be'):
        trainer.sm_grads(_dev(c['prob'][:, :100]), _dev(c['y']))
    with pytest.raises(ValueError, match='dlog must be'):
        trainer.sm_grads(_dev(c['prob']), _dev(c['y']), dlog=torch.zeros((1, HW, 9), device='cuda:0'))
    for k in MOVING:
        trainer.eng.update_tensor(k, p[k], refresh=False)
