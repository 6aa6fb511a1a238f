"""The per-layer activation summaries on the GPU (csrc/act_summary.hip, jcm_conv_layer_pre, summary.activation_summaries, --tb_activations;
DESIGN.md 4.8): the kernel against the numpy restatement of tests/act_summary_ref.py, the pre-activations of every layer against the
float64 oracle, the whole chain against the fused forward, and the command line through the independent event-file decoder."""
import ctypes
import io
import os
import sys
import zlib

import numpy as np
import pytest
import torch

from cli_util import run_cli
import joint_cnn_mrf_amd  # noqa: F401
from joint_cnn_mrf_amd import _lib, synth
from oracle import jcm_oracle as O

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import act_summary_ref as A  # noqa: E402
import tb_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -24          # unit roundoff of float32


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32), device='cuda:0')


def logit_tol(ref):
    return 2e-4 * max(1.0, float(np.abs(ref).max()))


def lib_limits():
    n = _lib.load().jcm_hist_bucket_limits(None, 0)
    buf = (ctypes.c_double * n)()
    assert _lib.load().jcm_hist_bucket_limits(buf, n) == n == A.N_BUCKETS
    return np.array(buf, np.float64)


# ------------------------------------------------------------------ the kernel against the restatement
# scope -> Cout; the *bn layers carry BatchNorm tensors the test draws itself, lin9 has none (activ = z, as for conv6)
KLAYERS = {'bn16': 16, 'bn128': 128, 'bn9': 9, 'lin9': 9}


def _kernel_params():
    rng = np.random.RandomState(77)
    p = {}
    for name, c in KLAYERS.items():
        p[name + '/weights'] = (rng.standard_normal((5, 5, 16, c)) * 0.05).astype(np.float32)
        p[name + '/biases'] = rng.standard_normal(c).astype(np.float32)
        if name.startswith('bn'):
            p[name + '/BatchNorm/gamma'] = (rng.uniform(0.3, 2.0, c) * rng.choice([-1.0, 1.0], c)).astype(np.float32)
            p[name + '/BatchNorm/beta'] = rng.standard_normal(c).astype(np.float32)
            p[name + '/BatchNorm/moving_mean'] = rng.standard_normal(c).astype(np.float32)
            p[name + '/BatchNorm/moving_variance'] = rng.uniform(0.05, 3.0, c).astype(np.float32)
    return p


@pytest.fixture(scope='module')
def kernel_setup():
    from joint_cnn_mrf_amd.engine import Engine
    p = _kernel_params()
    eng = Engine(device=0).load_params(p)
    yield eng, p
    eng.close()


def hand_made(shape, seed, lim):
    """Normal values of several magnitudes; NaN, +-Inf, exact zeros, +-1e-12, bucket limits themselves and their float32 neighbours sprinkled
    over every image; channel 3 negative everywhere.  Channel 7 (the pictures) gets its share of all of them."""
    rng = np.random.RandomState(seed)
    z = (rng.standard_normal(shape) * rng.choice([1e-3, 0.1, 1.0, 30.0], shape)).astype(np.float32)
    mid = lim.size // 2
    edges = [np.float32(lim[mid + 1 + k]) for k in (0, 1, 7, 150, 290, 291, 400, 600)]
    special = [np.nan, np.inf, -np.inf, 0.0, -0.0, 1e-12, -1e-12]
    for e in edges:
        special += [e, -e, np.nextafter(e, np.float32(0)), np.nextafter(e, np.float32(np.inf))]
    special = np.array(special, np.float32)
    flat = z.reshape(-1)
    where = rng.choice(flat.size, size=min(flat.size // 9, 40 * special.size), replace=False)
    flat[where] = special[np.arange(where.size) % special.size]
    z[..., 3] = -np.abs(rng.standard_normal(shape[:-1])).astype(np.float32) - np.float32(0.01)
    z[:, 0, :special.size, 7] = special[:z.shape[2]]
    return z


def check_against_restatement(eng, z, name, n_groups, n_pics, lim):
    r = eng.act_summary(dev(z), name, n_groups=n_groups, pic_channel=7, n_pics=n_pics)
    r2 = eng.act_summary(dev(z), name, n_groups=n_groups, pic_channel=7, n_pics=n_pics)
    ref = A.stats(z, n_groups, lim)
    st, cn = r['stats'], r['counts']
    assert st.shape == (n_groups, 4) and cn.shape == (n_groups, 3 + A.N_BUCKETS)
    for g, w in enumerate(ref):
        print('%s %s group %d: num %d n_pos %d nonfinite %d  |sum - fsum| %.3g (bound %.3g)  |sumsq - fsum| %.3g (bound %.3g)' % (
            name, z.shape, g, cn[g, 0], cn[g, 1], cn[g, 2], abs(st[g, 2] - w['sum']), w['sum_bound'], abs(st[g, 3] - w['sum_squares']), w['sum_squares_bound']))
        assert (cn[g, 0], cn[g, 1], cn[g, 2]) == (w['num'], w['n_pos'], w['n_nonfinite']), (name, g)
        assert w['n_nonfinite'] > 0 and w['num'] + w['n_nonfinite'] == w['size']
        assert np.array_equal(cn[g, 3:], w['buckets']), (name, g, np.nonzero(cn[g, 3:] != w['buckets']))
        assert st[g, 0] == w['min'] and st[g, 1] == w['max'], (name, g)
        assert abs(st[g, 2] - w['sum']) <= w['sum_bound'], (name, g)
        assert abs(st[g, 3] - w['sum_squares']) <= w['sum_squares_bound'], (name, g)
    used = A.groups(z.shape[0], n_groups)[-1][1]
    activ, pics = r['activ'].cpu().numpy(), r['pics'].cpu().numpy()
    assert st.tobytes() == r2['stats'].tobytes() and cn.tobytes() == r2['counts'].tobytes()
    assert activ[:used].tobytes() == r2['activ'].cpu().numpy()[:used].tobytes() and pics.tobytes() == r2['pics'].cpu().numpy().tobytes()
    assert pics.shape == (n_groups, n_pics) + z.shape[1:3]
    assert pics.tobytes() == np.ascontiguousarray(A.pictures(activ, n_groups, 7, n_pics)).tobytes()      # the slice of activ, bit for bit
    return activ[:used], z[:used]


@pytest.mark.parametrize('name,shape,n_groups,n_pics', [('bn16', (3, 7, 11, 16), 1, 3), ('bn128', (2, 15, 23, 128), 1, 2), ('bn9', (5, 30, 45, 9), 2, 2),
                                                        ('bn16', (4, 60, 90, 16), 2, 2), ('lin9', (5, 30, 45, 9), 2, 1)])
def test_kernel_against_restatement(kernel_setup, name, shape, n_groups, n_pics):
    """Statistics equal to the restatement (counts, buckets, min, max) and within the bound of any double summation order (sums), two calls
    bitwise identical; the activation against the formula with the fold read back from the library (jcm_bn_folded), which itself lies
    within the roundings of its four float32 steps of the float64 fold."""
    eng, p = kernel_setup
    lim = lib_limits()
    assert np.array_equal(lim, A.limits())
    z = hand_made(shape, zlib.crc32(repr((name, shape)).encode()), lim)
    activ, zu = check_against_restatement(eng, z, name, n_groups, n_pics, lim)
    if name == 'lin9':
        assert activ.tobytes() == zu.tobytes()                 # no BatchNorm: the activation is z
        return
    C = shape[3]
    sc, sh = eng.bn_folded(name, C)
    bn = [p['%s/BatchNorm/%s' % (name, k)] for k in ('gamma', 'beta', 'moving_mean', 'moving_variance')]
    sc64, sh64 = A.fold64(*bn)
    msc = np.abs(bn[2].astype(np.float64) * sc64)
    d_sc, d_sh = np.abs(sc.astype(np.float64) - sc64), np.abs(sh.astype(np.float64) - sh64)
    print('%s fold: library vs float64 fold rounded once: scale differs in %d of %d channels, max %.2f ulp; shift in %d, max %.2f ulp' % (
        name, (sc != sc64).sum(), C, (d_sc / np.spacing(np.abs(sc64))).max(), (sh != sh64).sum(), (d_sh / np.spacing(np.abs(sh64))).max()))
    # the library rounds v + eps, sqrt, 1 / . and gamma * . to float32 (3.5 U on the scale, sqrt halves the first), then mean * scale and beta - .
    assert (d_sc <= 5 * U * np.abs(sc64)).all()
    assert (d_sh <= 6 * U * msc + 2 * U * np.abs(sh64)).all()
    neg = zu <= 0
    assert neg[..., 3].all() and np.array_equal(activ[neg], np.broadcast_to(sh, zu.shape)[neg])      # one value per channel: the shift
    want = A.activation(zu, sc, sh)
    nan = np.isnan(zu)
    assert nan.any() and np.isnan(activ[nan]).all() and np.isnan(want[nan]).all()
    rest = ~neg & ~nan
    with np.errstate(invalid='ignore'):
        ok = (activ[rest] == want[rest]) | (np.abs(activ[rest].astype(np.float64) - want[rest]) <= np.spacing(np.abs(want[rest])))
    print('%s activ: %d of %d positive positions differ from the two-rounding formula (allowed: 1 ulp)' % (name, (activ[rest] != want[rest]).sum(), rest.sum()))
    assert ok.all()


def test_error_paths(kernel_setup):
    eng, _ = kernel_setup
    z = dev(np.zeros((4, 6, 5, 16), np.float32))
    for kw, msg in ((dict(n_groups=5), 'do not fill'), (dict(pic_channel=16), 'pic_channel'), (dict(n_groups=2, n_pics=3), 'n_pics'),
                    (dict(n_groups=0), 'n_groups'), (dict(pic_channel=-1), 'pic_channel')):
        with pytest.raises(RuntimeError, match=msg):
            eng.act_summary(z, 'bn16', **kw)
    with pytest.raises(RuntimeError, match='no conv layer'):
        eng.act_summary(z, 'conv7')
    with pytest.raises(RuntimeError, match='output channels'):
        eng.act_summary(z, 'bn128')
    x = dev(np.zeros((1, 8, 8, 16), np.float32))
    with pytest.raises(RuntimeError, match='no conv layer'):
        eng.conv_layer_pre(x, 'conv7', 1, 16)
    with pytest.raises(ValueError, match='stride'):
        eng.conv_layer_pre(x, 'bn16', 3, 16)
    with pytest.raises(RuntimeError, match='stride'):
        _lib.check(eng._lib.jcm_conv_layer_pre(eng._h, b'bn16', 3, eng._p(x), 1, 8, 8, eng._p(x)), 'jcm_conv_layer_pre')
    with pytest.raises(RuntimeError, match='stride-2 kernel'):
        eng.conv_layer_pre(x, 'bn16', 2, 16)
    with pytest.raises(RuntimeError, match='bad conv_layer_pre'):
        _lib.check(eng._lib.jcm_conv_layer_pre(eng._h, b'bn16', 1, eng._p(x), 1, 0, 8, eng._p(x)), 'jcm_conv_layer_pre')
    with pytest.raises(RuntimeError, match='no BatchNorm'):
        eng.bn_folded('lin9', 9)
    st = eng.act_summary(z, 'bn16')                       # the handle keeps working
    assert st['counts'][0, 0] == z.numel() and st['counts'][0, 1] == 0


# ------------------------------------------------------------------ the layers against the oracle
@pytest.fixture(scope='module')
def debug_setup():
    from joint_cnn_mrf_amd.engine import Engine
    p = synth.make_pd_params(debug=True, bn='trained', conv6_gain=8.0)
    eng = Engine(device=0).load_params(p)
    yield eng, p
    eng.close()


LAYERS = [('conv1_fullres', 5, 2, 1), ('conv1_halfres', 5, 2, 2), ('conv1_quarterres', 5, 2, 4),
          ('conv2_fullres', 5, 1, (120, 180)), ('conv3_fullres', 5, 1, (60, 90)), ('conv4_fullres', 9, 1, (60, 90)),
          ('conv3_halfres', 5, 1, (30, 45)), ('conv4_halfres', 9, 1, (30, 45)), ('conv4_quarterres', 9, 1, (15, 23)),
          ('conv5', 9, 1, (60, 90)), ('conv6', 9, 1, (60, 90))]


def layer_input(p, scope, stride, geo):
    if stride == 2:
        return synth.make_images(2, seed=3)[:, ::geo, ::geo]
    cin = p[scope + '/weights'].shape[2]
    return np.random.RandomState(zlib.crc32(scope.encode()) % 1000).standard_normal((2, geo[0], geo[1], cin)).astype(np.float32)


def check_layer(eng, p, scope, size, stride, x):
    cout = p[scope + '/weights'].shape[3]
    last = scope == 'conv6'
    ref_z = O.conv_layer(x, p, size, stride, scope, last_layer=True)
    z = eng.conv_layer_pre(dev(x), scope, stride, cout)
    got_z = z.cpu().numpy()
    assert got_z.shape == ref_z.shape
    err = float(np.abs(got_z - ref_z).max())
    print('%s %s: |z - oracle| max %.3g (tol %.3g)' % (scope, eng.conv_kernel_name(scope, *x.shape[:3]), err, logit_tol(ref_z)))
    assert err <= logit_tol(ref_z)
    r = eng.act_summary(z, scope, n_pics=2)
    activ = r['activ'].cpu().numpy()
    direct = eng.conv_layer(dev(x), scope, stride, last_layer=last, n_out=cout).cpu().numpy()
    print('%s: act_summary activ %s Engine.conv_layer bit for bit (%d of %d elements differ, max |d| %.3g)' % (
        scope, 'equals' if np.array_equal(activ, direct) else 'differs from', (activ != direct).sum(), activ.size, np.abs(activ - direct).max()))
    if last:
        assert activ.tobytes() == got_z.tobytes()
        return
    ref_a = O.bn_infer(np.maximum(ref_z, 0), p, scope)
    atol, rtol = (2e-5, 1e-5) if stride == 2 else (1e-4, 1e-4)
    np.testing.assert_allclose(activ, ref_a, atol=atol, rtol=rtol)
    assert r['counts'][0, 0] == got_z.size and r['counts'][0, 1] == int((got_z > 0).sum())


@pytest.mark.parametrize('scope,size,stride,geo', LAYERS)
def test_layers_against_oracle(debug_setup, scope, size, stride, geo):
    eng, p = debug_setup
    check_layer(eng, p, scope, size, stride, layer_input(p, scope, stride, geo))


def test_both_routes_of_one_layer(debug_setup):
    """conv4_halfres (64 input channels) on an odd map: the default engine takes the frequency-domain route, an engine with conv9_fft off the
    direct MFMA kernel; the pre-activation of either holds the same bound."""
    from joint_cnn_mrf_amd.engine import Engine
    eng, p = debug_setup
    x = np.random.RandomState(45).standard_normal((3, 33, 47, 64)).astype(np.float32)
    assert 'conv_fft' in eng.conv_kernel_name('conv4_halfres', 3, 33, 47)
    check_layer(eng, p, 'conv4_halfres', 9, 1, x)
    eng2 = Engine(device=0, conv9_fft=False).load_params(p)
    assert eng2.conv_kernel_name('conv4_halfres', 3, 33, 47) == 'conv_igemm_f32_kernel'
    check_layer(eng2, p, 'conv4_halfres', 9, 1, x)
    eng2.close()


def test_refusals_stay(debug_setup):
    from joint_cnn_mrf_amd.engine import Engine
    eng, _ = debug_setup
    x = dev(np.zeros((1, 30, 45, 16), np.float32))
    with pytest.raises(RuntimeError, match='last_layer'):
        eng.conv_layer(x, 'conv2_fullres', 1, last_layer=True, n_out=32)
    # a bf16 handle needs Cin % 32 == 0 in every stride-1 layer (the debug-width conv2 layers have 16): one 32-channel layer of its own
    rng = np.random.RandomState(5)
    q = {'wide/weights': (rng.standard_normal((5, 5, 32, 32)) * 0.05).astype(np.float32), 'wide/biases': rng.standard_normal(32).astype(np.float32)}
    for k in ('gamma', 'beta', 'moving_mean', 'moving_variance'):
        q['wide/BatchNorm/' + k] = rng.uniform(0.5, 1.5, 32).astype(np.float32)
    bf = Engine(device=0, precision='bf16').load_params(q)
    xb = dev(np.zeros((1, 30, 45, 32), np.float32))
    with pytest.raises(RuntimeError, match='bf16'):
        bf.conv_layer_pre(xb, 'wide', 1, 32)
    bf.close()


# ------------------------------------------------------------------ the whole chain
def test_whole_chain(debug_setup):
    from joint_cnn_mrf_amd import summary as S
    eng, p = debug_setup
    x = synth.make_images(4, seed=21)
    ref = O.model(x, p)
    taps = {'conv6': None}
    vals = S.activation_summaries(eng, dev(x), n_towers=2, taps=taps)
    z6 = taps['conv6'].cpu().numpy()
    fused = eng.model(dev(x)).cpu().numpy()
    print('chain: |conv6 pre-activation - oracle| %.3g, |. - fused model| %.3g (tol %.3g)' % (np.abs(z6 - ref).max(), np.abs(z6 - fused).max(), logit_tol(ref)))
    np.testing.assert_allclose(z6, ref, atol=logit_tol(ref), rtol=0)
    np.testing.assert_allclose(z6, fused, atol=logit_tol(ref), rtol=0)
    vals = [R.parse_value(v.result() if hasattr(v, 'result') else v) for v in vals]
    assert [v['tag'] for v in vals] == A.tags(2, 2) and len(vals) == 2 * 14 * (6 + 2)
    by = {v['tag']: v for v in vals}
    widths = {s: p[s + '/weights'].shape[3] for s in A.SCOPES}
    for i in range(2):
        for s in A.SCOPES:
            res = {'fullres': 1, 'halfres': 2, 'quarterres': 4}.get(s.split('_')[-1], 1)
            h, w = (240 // res, 360 // res) if s.startswith('conv1') else (120 // res, 180 // res) if s.startswith('conv2') else (60 // res, -(-90 // res))
            pre = 'tower_%d/pre_activ_%s/' % (i, s)
            assert by[pre + 'histogram']['histo']['num'] == 2 * h * w * widths[s] == sum(by[pre + 'histogram']['histo']['bucket']), (s, h, w)
            assert 0.0 <= by[pre + 'n_pos']['simple_value'] <= 1.0
            assert by[pre + 'min']['simple_value'] <= by[pre + 'mean']['simple_value'] <= by[pre + 'max']['simple_value']
            im = by['tower_%d/f_activ_%s/image/1' % (i, s)]['image']
            assert (im['height'], im['width'], im['colorspace']) == (h, w, 1)


# ------------------------------------------------------------------ the command line
def _run(args, cwd, ok=True, timeout=900):
    r = run_cli(args, cwd, timeout=timeout)
    assert (r.returncode == 0) == ok, r.stdout[-2000:] + r.stderr[-2000:]
    return r


def _events(d):
    files = [f for f in os.listdir(d) if f.startswith('events.out.tfevents.')]
    assert len(files) == 1, files
    by_step = {}
    for e in R.read_events(os.path.join(d, files[0]), check_crc=True)[1:]:
        for v in e['values']:
            by_step.setdefault(e['step'], {})[v['tag']] = v
    return by_step


def _check_activation_tags(tags):
    from PIL import Image
    for i in range(2):
        t = 'tower_%d/' % i
        assert 0.0 <= tags[t + 'pre_activ_conv1_fullres/n_pos']['simple_value'] <= 1.0
        assert tags[t + 'pre_activ_conv5/histogram']['histo']['num'] == 2 * 60 * 90 * 128
        for s, hw in (('conv1_fullres', (240, 360)), ('conv6', (60, 90))):
            v = tags[t + 'f_activ_%s/image/1' % s]['image']
            im = np.asarray(Image.open(io.BytesIO(v['png'])))
            assert (v['height'], v['width']) == hw and im.shape == hw and im.dtype == np.uint8, (s, im.shape)      # gray
    assert not any(k.startswith('tower_') and k.endswith('/image/2') for k in tags)
    assert [k for k in tags if k.startswith('tower_')] == A.tags(2, 2)


def test_cli_train_writes_activation_summaries(tmp_path):
    common = ['--train', '--debug', '--use_sm', '--synthetic', '--synthetic_size', '8', '--batch_size', '4', '--gpus', '0', '0', '--n_epochs', '1',
              '--model_path', str(tmp_path / 'models_ex')]
    D = tmp_path / 'tb'
    _run(common + ['--tb_dir', str(D), '--tb_activations'], str(tmp_path))
    (run,) = os.listdir(str(D))
    for split in ('train', 'test'):
        ev = _events(str(D / run / split))
        assert sorted(ev) == [0, 1]
        for step in (0, 1):
            _check_activation_tags(ev[step])
            assert 'input/image/0' in ev[step] and 'grads/conv5/weights' in ev[step]      # behind the tags that were there before
    D2 = tmp_path / 'tb_plain'
    _run(common + ['--tb_dir', str(D2)], str(tmp_path))
    (run,) = os.listdir(str(D2))
    for split in ('train', 'test'):
        for tags in _events(str(D2 / run / split)).values():
            assert not any(k.startswith('tower_') for k in tags)


def test_cli_eval_and_refusals(tmp_path):
    D = tmp_path / 'tb'
    common = ['--debug', '--use_sm', '--synthetic', '--synthetic_size', '4', '--batch_size', '4', '--gpus', '0', '0']
    _run(common + ['--tb_dir', str(D), '--tb_activations'], str(tmp_path))
    (run,) = os.listdir(str(D))
    for split in ('train', 'test'):
        ev = _events(str(D / run / split))
        assert sorted(ev) == [0]
        _check_activation_tags(ev[0])
    r = _run(common + ['--tb_activations'], str(tmp_path), ok=False)
    assert '--tb_dir' in r.stderr
    r = _run(common + ['--tb_dir', str(tmp_path / 'no'), '--tb_activations', '--precision', 'bf16'], str(tmp_path), ok=False)
    assert 'fp32' in r.stderr and not os.path.exists(str(tmp_path / 'no'))
