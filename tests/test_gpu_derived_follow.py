"""Every table the library derives from the parameter store must follow a parameter change (csrc/derived.hip: refresh_derived; csrc/conv_route.hip:
fft_cache_invalidate; csrc/train_state.hip: dgrad_filters_stale): a handle whose parameters CHANGED must compute what a handle freshly loaded with
the new parameters computes.

No tolerances.  Handle A is loaded with P0 and warmed (every call of the probe sequence runs once, so every lazy table and cache entry exists), moved
to P1 by a mutation route, and compared BIT FOR BIT with a fresh handle F of the same options that was loaded with P1 as read back from A; both run
the same probe sequence (derived_follow_util.probe) in the same order.  Each case also asserts that the mutation is visible in the outputs it is
checked on, so a comparison cannot pass on tables nobody reads:
  whole-model mutations: every probe output of A differs from A's own output before the mutation in at least half of its entries;
  single-tensor mutations: every output listed for the tensor in DEPENDS differs in at least 1 % of its entries, every other output not at all;
  float64 anchor (debug width): A after the whole-model mutation against oracle.jcm_oracle.forward on P1 at test_gpu_parity's bounds, P0 and P1
  being at least 100 bounds apart on the oracle alone.

bf16 handles exist at full width only (derived.hip: "bf16 path needs Cin % 32 == 0"; the debug-width conv2 layers have 16 input channels,
test_bf16_handles_need_the_full_width pins it), so the two bf16 handles run their cases at full width, where wq1_*, wp_kxfold, the strip kernels, the
tiled conv2 and the logits-rows operand live."""
import numpy as np
import pytest
import torch

import derived_follow_util as U
from joint_cnn_mrf_amd import synth
from oracle import jcm_oracle as O
from test_gpu_parity import HM_TOL

pytestmark = pytest.mark.gpu

FP32_KINDS = ['fp32', 'chain', 'split16']
INDEX_OUTPUTS = ['fwd/pd_coords', 'fwd/sm_coords', 'torso/cell']      # arg-maxes of other outputs of the sequence: a small change need not move them


def close_all(*engines):
    for e in engines:
        e.close()


def assert_moved(before, after, least, what, skip=()):
    bad = ['%s: %.4f of the entries changed' % (k, U.changed_fraction(before[k], after[k])) for k in after
           if not U.matches(k, skip) and U.changed_fraction(before[k], after[k]) < least]
    assert not bad, '%s: the mutation does not show in\n  %s' % (what, '\n  '.join(bad))


def test_bf16_handles_need_the_full_width():
    eng = U.make_engine('bf16')
    with pytest.raises(RuntimeError, match='Cin % 32'):
        eng.load_params(U.params(0))
    eng.close()


# ---------------------------------------------------------------------------------------------------------------- float64 anchor
@pytest.fixture(scope='module')
def anchor():
    """oracle.forward on P0 and P1 (debug width, the first probe image), computed once."""
    inp = U.inputs(True, 2)
    x, torso = inp.x480[:1].cpu().numpy(), inp.torso[:1].cpu().numpy()
    return [O.forward(x, torso, U.params(w)) for w in (0, 1)]


def test_anchor_separates_the_two_parameter_sets(anchor):
    """On the float64 oracle alone: forward(P0) and forward(P1) are at least 100 bounds apart, for each bound the GPU comparison below uses --
    HM_TOL absolute on the part detector's probabilities and 2e-3 relative on the spatial model's (test_gpu_parity.test_full_tower_debug_size holds
    both maps to both bounds; the spatial model's probabilities never exceed 1.3e-3 on these parameters, so only the relative bound can separate them)."""
    r0, r1 = anchor
    d = np.abs(r0['pd_prob'] - r1['pd_prob']).max()
    print('pd_prob: oracle P0 to P1', d)
    assert d >= 100 * HM_TOL
    rel = (np.abs(r0['sm_prob'] - r1['sm_prob']) / r1['sm_prob']).max()
    print('sm_prob: oracle P0 to P1, relative', rel, 'absolute', np.abs(r0['sm_prob'] - r1['sm_prob']).max())
    assert rel >= 100 * 2e-3


# ---------------------------------------------------------------------------------------------------------------- route 1: the batch idiom
# the kernels the full-width cases are here for (jcm_conv_kernel_name(scope, 1, H, W)); the tiled conv2 and the logits-rows operand are forms of
# the conv_fft route that the name does not tell apart (conv_route.hip: run_conv_fft, FftArgs::tiles / lrows)
FFT = 'conv_fft(cgemm_split_kernel)'
FULL_ROUTES = {
    'fp32': {('conv1_fullres', 480, 720): 'conv1_mfma_pool_split_kernel', ('conv2_fullres', 120, 180): FFT, ('conv5', 60, 90): FFT, ('conv6', 60, 90): FFT},
    'bf16': {('conv1_fullres', 480, 720): 'conv1_mfma_pool_kernel', ('conv2_fullres', 120, 180): 'conv5_strip_bf16_kernel', ('conv5', 60, 90): FFT,
             ('conv6', 60, 90): 'conv_kxfold_bf16_kernel'},
}
FULL_ROUTES['bf16x2'] = FULL_ROUTES['bf16']
DEBUG_ROUTES = {
    'fp32': {('conv4_fullres', 60, 90): FFT, ('conv5', 60, 90): FFT, ('conv6', 60, 90): FFT, ('conv3_fullres', 60, 90): 'conv_igemm_f32_kernel'},
    'chain': {('conv5', 60, 90): 'conv_igemm_f32_kernel', ('conv6', 60, 90): 'conv_thin_f32_kernel'},
    'split16': {('conv5', 60, 90): 'conv_split_kernel', ('conv6', 60, 90): 'conv_thin_split16_kernel'},
}


@pytest.mark.parametrize('kind,debug', [(k, True) for k in FP32_KINDS] + [('fp32', False), ('bf16', False), ('bf16x2', False)],
                         ids=lambda v: v if isinstance(v, str) else ('debug' if v else 'full'))
def test_batch_of_updates_equals_a_fresh_handle(kind, debug, anchor):
    """jcm_update_tensor for every tensor, refresh = 0 on all but the last."""
    B = 2 if debug else 1
    p0, p1, inp = U.params(0, debug), U.params(1, debug), U.inputs(debug, B)
    A = U.make_engine(kind).load_params(p0)
    F = U.make_engine(kind)
    try:
        for (scope, H, W), name in (DEBUG_ROUTES if debug else FULL_ROUTES)[kind].items():
            assert A.conv_kernel_name(scope, B, H, W) == name, scope
        before = U.probe(A, inp)
        U.update_all(A, p1)
        back = U.get_params(A, p1)
        for k in p1:
            assert np.array_equal(U.bits(back[k]), U.bits(p1[k])), k
        after = U.probe(A, inp)
        fresh = U.probe(F.load_params(back), inp)
        assert_moved(before, after, 0.5, 'P0 -> P1')
        U.assert_same(after, fresh, '%s handle after a batch of updates against a fresh one' % kind)
        if debug:
            ref = anchor[1]
            pd, sm = (after['fwd/' + k][:1].view(np.float32) for k in ('pd_prob', 'sm_prob'))
            print('pd_prob err', np.abs(pd - ref['pd_prob']).max(), 'sm_prob err', np.abs(sm - ref['sm_prob']).max(),
                  'sm_prob rel err', (np.abs(sm - ref['sm_prob']) / ref['sm_prob']).max())
            np.testing.assert_allclose(pd, ref['pd_prob'], atol=HM_TOL, rtol=0)
            np.testing.assert_allclose(sm, ref['sm_prob'], atol=HM_TOL, rtol=0)
            np.testing.assert_allclose(sm, ref['sm_prob'], rtol=2e-3, atol=1e-9)
            for k in ('pd_coords', 'sm_coords'):
                np.testing.assert_array_equal(after['fwd/' + k][:1], ref[k])
    finally:
        close_all(A, F)


# ---------------------------------------------------------------------------------------------------------------- route 2: one tensor at a time
TOWER = ['model480', 'model240', 'fwd/pd_prob', 'fwd/sm_prob', 'fwd240/pd_prob']
SM_TOWER = ['fwd/sm_prob', 'sm']


def _conv(scope, *more):
    return TOWER + ['conv_layer/' + scope, 'pre/' + scope] + list(more)


def _bn(scope, scale=True):
    return TOWER + ['conv_layer/' + scope, 'bn/%s/shift' % scope, 'act/%s/activ' % scope, 'act/%s/pics' % scope] + (['bn/%s/scale' % scope] if scale else [])


scale15 = lambda a: a * np.float32(1.5)
add025 = lambda a: a + np.float32(0.25)
# tensor -> (the change, the probe outputs that read a table derived from it -- found by reading derived.hip, conv_route.hip, pd_tower.hip,
# act_summary.hip and torso_infer.hip).  Every other output of the sequence must not move; INDEX_OUTPUTS may do either.
DEPENDS = {
    'conv3_fullres/weights': (scale15, _conv('conv3_fullres')),                                   # a 5x5 layer: wp / wp_split, "<scope>@HxW"
    'conv4_fullres/weights': (scale15, _conv('conv4_fullres')),                                   # a wide 9x9 layer: spectra, wp (lazily), wp_split
    'conv6/weights': (scale15, _conv('conv6')),                                                   # the logits layer: "@rowsHxW", thin packings
    'conv1_fullres/weights': (scale15, _conv('conv1_fullres', 'conv1_pool/conv1_fullres')),       # w_raw, wq1_*
    'conv5/biases': (add025, _conv('conv5', 'merged/conv5')),
    # the folded scale / shift of one layer: scale = gamma / sqrt(var + eps), shift = beta - mean * scale (derived.hip: fold_bn)
    'conv4_halfres/BatchNorm/gamma': (scale15, _bn('conv4_halfres')),
    'conv4_halfres/BatchNorm/beta': (add025, _bn('conv4_halfres', scale=False)),
    'conv4_halfres/BatchNorm/moving_mean': (add025, _bn('conv4_halfres', scale=False)),
    'conv4_halfres/BatchNorm/moving_variance': (scale15, _bn('conv4_halfres')),
    # sp_energy + prior_spec_t; the torso energy reads the <j>_torso priors only (torso_infer.hip), and has no bias term
    'energy_lsho_torso': (scale15, SM_TOWER + ['torso/energy']),
    'bias_lelb_nose': (add025, SM_TOWER),
    'bn_sm/BatchNorm/moving_variance': (scale15, SM_TOWER + ['torso/energy']),
}


@pytest.fixture(scope='module', params=FP32_KINDS)
def warmed(request):
    """(kind, handle at P0 with every probe run once, its outputs)."""
    A = U.make_engine(request.param).load_params(U.params(0))
    inp = U.inputs(True, 2)
    yield request.param, A, U.probe(A, inp), inp
    A.close()


@pytest.mark.parametrize('name', list(DEPENDS))
def test_single_tensor_update_equals_a_fresh_handle(warmed, name):
    """jcm_update_tensor(refresh = 1) on one tensor: the outputs DEPENDS lists change, no other does, all equal a fresh handle; putting the tensor
    back (one more refresh) gives the first outputs again."""
    kind, A, base, inp = warmed
    change, listed = DEPENDS[name]
    assert set(listed) <= set(base), sorted(set(listed) - set(base))
    p1 = dict(U.params(0))
    p1[name] = np.ascontiguousarray(change(p1[name]), dtype=np.float32)
    F = U.make_engine(kind)
    try:
        A.update_tensor(name, p1[name], refresh=True)
        after = U.probe(A, inp)
        fresh = U.probe(F.load_params(U.get_params(A, p1)), inp)
    finally:
        A.update_tensor(name, U.params(0)[name], refresh=True)
        F.close()
    for k in after:
        frac = U.changed_fraction(base[k], after[k])
        if k in listed:
            assert frac >= 0.01, '%s does not show the change of %s (%.4f of its entries)' % (k, name, frac)
        elif k not in INDEX_OUTPUTS:
            assert frac == 0, '%s moved with %s (%.4f of its entries)' % (k, name, frac)
    U.assert_same(after, fresh, '%s handle after an update of %s against a fresh one' % (kind, name))
    U.assert_same(U.probe(A, inp), base, '%s handle with %s put back' % (kind, name))


# ---------------------------------------------------------------------------------------------------------------- routes 3 and 4: training
def _targets(B):
    return U.dev(synth.make_targets(B, seed=56))


def _stages(tr, inp):
    """The step's stages on caller tensors, after the mutation: one frequency-domain layer (on the default fp32 handle), one direct layer, a
    training-mode BatchNorm and the spatial model's stage -> {name: bits}."""
    dt = tr._act_dtype()
    out = {}
    for scope in ('conv4_fullres', 'conv3_fullres'):
        dw, dx = tr.layer_grads(scope, inp.x[scope].to(dt), inp.z[scope].to(dt))
        out['layer_grads/%s/dw' % scope], out['layer_grads/%s/dx' % scope] = U.bits(dw), U.bits(dx)
    y, p, mean, rstd = tr.bn_forward('conv3_fullres', inp.z['conv3_fullres'].to(dt), pool=True)
    for k, v in (('y', y), ('pool', p), ('mean', mean), ('rstd', rstd)):
        out['bn_forward/' + k] = U.bits(v)
    B = inp.B
    ce, dlog = tr.sm_grads(inp.prob.view(B, 5400, 9), _targets(B).view(B, 5400, 10))
    out['sm_grads/ce'], out['sm_grads/dlog'], out['sm_grads/grads'] = U.bits(ce), U.bits(dlog), U.bits(tr.grads)
    return out


def _same_route_without_training_state(A, Fi, inp):
    """Which probe outputs a handle with training state computes on the route an inference-only handle takes: a layer whose kernel name is the same
    on both and is not the frequency-domain route (conv_route.hip: run_conv_fft sets FftScale::common = 1 on a handle with training state, one scale
    per tensor, and refuses the logits-rows operand there); the tower when that holds for every layer; everything that is no convolution."""
    B, maps = inp.B, dict(U.layer_maps(), conv1_fullres=(480, 720), conv1_halfres=(240, 360), conv1_quarterres=(120, 180))
    ok = {s[0]: A.conv_kernel_name(s[0], B, *maps[s[0]]) == Fi.conv_kernel_name(s[0], B, *maps[s[0]]) and not A.conv_kernel_name(s[0], B, *maps[s[0]]).startswith('conv_fft')
          for s in inp.scopes}
    whole = all(ok.values()) and all(A.conv_kernel_name(s, B, h, w) == Fi.conv_kernel_name(s, B, h, w) and not A.conv_kernel_name(s, B, h, w).startswith('conv_fft')
                                     for s, (h, w) in U.layer_maps(240, 368).items())

    def same(name):
        head, _, rest = name.partition('/')
        if head in ('conv_layer', 'pre', 'merged', 'conv1_pool', 'conv2_pool'):
            return ok[rest]
        if head in ('model480', 'model240', 'fwd', 'fwd240'):
            return whole
        return True
    return same


@pytest.mark.parametrize('kind,debug,optimizer', [(k, True, o) for k in FP32_KINDS for o in ('adam', 'momentum')] + [('bf16', False, 'adam')],
                         ids=lambda v: v if isinstance(v, str) else ('debug' if v else 'full'))
def test_training_steps_equal_a_fresh_handle(kind, debug, optimizer):
    """Two loss_and_grads + apply steps on A; F gets A's parameters, optimizer slots and n_iters.  Inference after the second apply (route 4), the third
    loss_and_grads (the data-gradient filters, the window spectra and the "dgrad:" spectra are rebuilt in it), the third apply and the stages."""
    from joint_cnn_mrf_amd.train import Trainer
    B = 2 if debug else 1
    p0, inp = U.params(0, debug), U.inputs(debug, B)
    x, y = inp.x480, _targets(B)
    kw = dict(optimizer=optimizer, lr=0.001, lmbd=0.001, use_sm=True)
    A, Ft, Fi = (U.make_engine(kind) for _ in range(3))
    try:
        trA = Trainer(A.load_params(p0), **kw)
        before = U.probe(A, inp)
        for _ in range(2):
            trA.loss_and_grads(x, y)
            trA.apply()
        p2 = U.get_params(A, p0)
        m, v, n = U.get_state(trA)
        assert n == 2
        after = U.probe(A, inp)
        assert_moved(before, after, 0.5, 'two %s updates' % optimizer, skip=INDEX_OUTPUTS)
        trF = Trainer(Ft.load_params(p2), **kw)
        U.set_state(trF, m, v, n)
        U.assert_same(after, U.probe(Ft, inp), '%s handle after two updates against a fresh handle with training state' % kind)
        fi = U.probe(Fi.load_params(p2), inp)
        same = _same_route_without_training_state(A, Fi, inp)
        assert sum(same(k) for k in after) >= (len(after) if kind in ('chain', 'split16') else 20)
        U.assert_same(after, fi, '%s handle after two updates against a fresh inference-only handle' % kind, only=same)
        got = []
        for tr in (trA, trF):
            losses, grads = tr.loss_and_grads(x, y)
            step = {'losses': U.bits(losses), 'grads': U.bits(grads)}
            tr.apply()
            step.update({'param/' + k: U.bits(t) for k, t in U.get_params(tr.eng, p0).items()})
            ms, vs, ns = U.get_state(tr)
            step.update({'slot0': U.bits(ms), 'slot1': U.bits(vs), 'n_iters': np.array([ns])})
            step.update(_stages(tr, inp))
            got.append(step)
        assert got[0]['n_iters'][0] == 3 and np.isfinite(got[0]['losses'].view(np.float32)).all()
        assert U.changed_fraction(got[0]['grads'], np.zeros_like(got[0]['grads'])) >= 0.5
        U.assert_same(got[0], got[1], '%s handle, third step and stages, against a fresh handle' % kind)
    finally:
        close_all(A, Ft, Fi)


@pytest.mark.parametrize('kind', FP32_KINDS)
def test_inference_between_loss_and_grads_and_apply(kind):
    """jcm_train_loss_grads advances the moving statistics in the parameter store, but the folded BatchNorm tables are rebuilt by jcm_train_apply /
    jcm_update_tensor(refresh != 0) only: inference after a lone loss_and_grads is bit-identical to inference before it, differs from a fresh handle
    with the stored parameters, and equals that handle after a refresh (include/jcm.h: jcm_train_loss_grads)."""
    from joint_cnn_mrf_amd.train import Trainer
    p0, inp = U.params(0), U.inputs(True, 2)
    kw = dict(optimizer='adam', lr=0.001, lmbd=0.001, use_sm=True)
    A, G = U.make_engine(kind), U.make_engine(kind)
    try:
        trA = Trainer(A.load_params(p0), **kw)
        before = U.probe(A, inp)
        trA.loss_and_grads(inp.x480, _targets(2))
        U.assert_same(U.probe(A, inp), before, '%s handle before and after a lone loss_and_grads' % kind)
        stored = U.get_params(A, p0)
        moved = [k for k in p0 if not np.array_equal(stored[k], p0[k])]
        assert moved and all(k.endswith(('moving_mean', 'moving_variance')) for k in moved), moved
        Trainer(G.load_params(stored), **kw)
        fresh = U.probe(G, inp)
        assert_moved(before, fresh, 0.5, 'the advanced moving statistics', skip=INDEX_OUTPUTS + ['pre/*', 'conv_layer/conv6'])      # (conv + bias reads no BatchNorm)
        A.update_tensor(moved[0], stored[moved[0]], refresh=True)      # the same bits: only the refresh
        U.assert_same(U.probe(A, inp), fresh, '%s handle after the refresh against a fresh handle' % kind)
    finally:
        close_all(A, G)
