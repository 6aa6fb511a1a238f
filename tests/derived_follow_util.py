"""Helpers of tests/test_gpu_derived_follow.py: the handles, the parameter sets, the probe sequence and the bitwise comparisons.

A probe sequence is an ORDERED dict {output name: numpy integer array holding the output's bits}.  Two handles that hold the same parameters
and run the same sequence in the same order must return the same dict, bit for bit; state that legitimately depends on the order of calls
(the scale word a "dgrad:" pseudo-layer borrows from its forward spectra, conv_route.hip: fft_forward_wscale) is then equal on both sides."""
import ctypes
import fnmatch
import functools

import numpy as np
import torch

import joint_cnn_mrf_amd  # noqa: F401
from joint_cnn_mrf_amd import _lib, synth

# keyword arguments of Engine per handle kind (the issue's list)
HANDLES = {
    'fp32': {},
    'chain': {'conv9_fft': False},
    'split16': {'f32_conv': 'split16', 'split_min_wgs': 0},
    'bf16': {'precision': 'bf16'},
    'bf16x2': {'precision': 'bf16', 'fft_single': False},
}


def make_engine(kind):
    from joint_cnn_mrf_amd.engine import Engine
    return Engine(device=0, **HANDLES[kind])


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), device='cuda:0')


def bits(t):
    """The bits of a tensor or array as a numpy integer array of the same shape."""
    if isinstance(t, torch.Tensor):
        if t.dtype == torch.bfloat16:
            return t.view(torch.int16).cpu().numpy()
        t = t.cpu().numpy()
    a = np.ascontiguousarray(t)
    if a.dtype.kind == 'f':
        return a.view({4: np.int32, 8: np.int64}[a.dtype.itemsize])
    return a


@functools.lru_cache(maxsize=None)
def params(which, debug=True):
    """P0 (which = 0) and P1 (which = 1): two seeds of make_pd_params + make_sm_params.  The prior histograms take another seed as well (the
    'trained' energies are a function of the priors alone), and P1's biases are not the zeros every seed starts from."""
    s = 100 * which
    p = synth.make_pd_params(debug=debug, seed=7 + s, bn='trained', conv6_gain=8.0)
    p.update(synth.make_sm_params(synth.synthetic_priors(seed=5 + s), kind='trained', seed=11 + s))
    if which:
        rs = np.random.RandomState(1000 + s)
        for k in p:
            if k.endswith('/biases'):
                p[k] = (0.1 * rs.standard_normal(p[k].shape)).astype(np.float32)
    return {k: np.ascontiguousarray(v, dtype=np.float32) for k, v in p.items()}


def get_tensor(eng, name, like):
    out = np.empty(np.asarray(like).size, np.float32)
    _lib.check(eng._lib.jcm_get_tensor(eng._h, name.encode(), ctypes.c_void_p(out.ctypes.data), out.size), 'jcm_get_tensor(%s)' % name)
    return out.reshape(np.asarray(like).shape)


def get_params(eng, like):
    return {k: get_tensor(eng, k, v) for k, v in like.items()}


def update_all(eng, p):
    """The documented batch idiom: refresh = 0 on every tensor but the last."""
    names = list(p)
    for i, k in enumerate(names):
        eng.update_tensor(k, p[k], refresh=(i == len(names) - 1))


def get_state(tr):
    """(slot 0, slot 1, n_iters) of a Trainer's optimizer."""
    out, n = [], ctypes.c_int64()
    for slot in (0, 1):
        buf = np.empty(tr.n_elements, np.float32)
        _lib.check(tr._lib.jcm_train_get_state(tr.eng._h, slot, ctypes.c_void_p(buf.ctypes.data), buf.size, ctypes.byref(n)), 'jcm_train_get_state')
        out.append(buf)
    return out[0], out[1], n.value


def set_state(tr, m, v, n_iters):
    for slot, buf in ((0, m), (1, v)):
        _lib.check(tr._lib.jcm_train_set_state(tr.eng._h, slot, ctypes.c_void_p(buf.ctypes.data), buf.size, int(n_iters)), 'jcm_train_set_state')


# ---------------------------------------------------------------------------------------------------------------- probe inputs
def layer_maps(H=480, W=720):
    """{stride-1 scope: (h, w) of its input map} for an H x W image (main.py:44-72)."""
    c = lambda n: -(-n // 2)
    out = {}
    for sub, res in ((1, 'fullres'), (2, 'halfres'), (4, 'quarterres')):
        h1, w1 = c(c(-(-H // sub))), c(c(-(-W // sub)))      # conv1 (stride 2) + pool1
        out['conv2_' + res] = (h1, w1)
        out['conv3_' + res] = out['conv4_' + res] = (c(h1), c(w1))
    out['conv5'] = out['conv6'] = out['conv4_fullres']
    return out


class Inputs:
    """The fixed inputs of one probe sequence: B images at 480x720 and at 240x368, a torso map, and per layer a seeded input, pre-activation
    and heat map of the layer's own shape.  Device tensors, made once per (width, B)."""

    def __init__(self, debug, B):
        self.debug, self.B = debug, B
        self.scopes = synth.conv_scopes(debug)
        self.x480 = dev(synth.make_images(B, seed=51))
        self.x240 = dev(synth.make_images(B, seed=53, height=240, width=368))
        self.torso = dev(synth.make_torso(B, seed=52))
        rs = np.random.RandomState(54)
        maps = layer_maps()
        self.x, self.z = {}, {}
        for scope, k, stride, cin, cout, last in self.scopes:
            if stride != 1:
                continue
            h, w = maps[scope]
            self.x[scope] = dev(rs.standard_normal((B, h, w, cin)).astype(np.float32))
            if not last:
                self.z[scope] = dev(rs.standard_normal((B, h, w, cout)).astype(np.float32))
        c4 = self.x['conv5'].shape[3]
        self.merge = [dev(rs.standard_normal((B, h, w, c4)).astype(np.float32)) for h, w in ((60, 90), (30, 45), (15, 23))]
        self.p1 = {res: dev(rs.standard_normal((B,) + maps['conv2_' + res] + (self.x['conv2_' + res].shape[3],)).astype(np.float32)).to(torch.bfloat16)
                   for res in synth.RESOLUTIONS}
        e = np.exp(3.0 * rs.standard_normal((B, 5400, 9)))
        prob = (e / e.sum(axis=1, keepdims=True)).reshape(B, 60, 90, 9).astype(np.float32)
        self.prob = dev(prob)
        self.hm10 = dev(np.concatenate([prob, synth.make_torso(B, seed=55)], axis=3))


@functools.lru_cache(maxsize=None)
def inputs(debug, B):
    return Inputs(debug, B)


# ---------------------------------------------------------------------------------------------------------------- the probe sequence
def probe(eng, inp, second_size=True):
    """Every inference entry point that reads a parameter-derived table, in a fixed order -> {name: bits}.

    model / forward: the tower (every packed weight or filter-spectra form the handle's route takes, the folded BatchNorm, the spatial model's
    tables); conv_layer / conv_layer_pre / conv_layer_merged: each stride-1 layer by itself ("<scope>@HxW" spectra, wp / wp_split / wp_bf16 /
    wp_kxfold); conv1_pool / conv2_pool: wq1_* and the strip kernels' wp_bf16; spatial_model: sp_energy / sp_bias / prior_spec_t / bn_sm's fold;
    jcm_bn_folded: the folded table itself; act_summary: the fold applied to a given pre-activation; torso_infer: sp_energy and bn_sm's fold
    (torso_infer.hip: torso_infer_direct(prob, B, c->sp_energy, c->bn_sm_scale, c->bn_sm_shift, ..))."""
    bf = eng.precision == 'bf16'
    out = {}
    out['model480'] = bits(eng.model(inp.x480))
    r = eng.forward(inp.x480, inp.torso, use_sm=True)
    for k in ('pd_prob', 'sm_prob', 'pd_coords', 'sm_coords'):
        out['fwd/' + k] = bits(r[k])
    if second_size:
        out['model240'] = bits(eng.model(inp.x240))
        out['fwd240/pd_prob'] = bits(eng.forward(inp.x240, None, use_sm=False)['pd_prob'])
    for scope, k, stride, cin, cout, last in inp.scopes:
        if stride == 1:
            out['conv_layer/' + scope] = bits(eng.conv_layer(inp.x[scope], scope, 1, last_layer=last, n_out=cout))
            if not bf:
                out['pre/' + scope] = bits(eng.conv_layer_pre(inp.x[scope], scope, 1, cout))
        else:
            sub = {'fullres': 1, 'halfres': 2, 'quarterres': 4}[scope.split('_')[1]]
            out['conv1_pool/' + scope] = bits(eng.conv1_pool(inp.x480, scope, sub))
            if not bf:
                xs = inp.x480[:, ::sub, ::sub].contiguous()
                out['conv_layer/' + scope] = bits(eng.conv_layer(xs, scope, 2, n_out=cout))
                out['pre/' + scope] = bits(eng.conv_layer_pre(xs, scope, 2, cout))
    out['merged/conv5'] = bits(eng.conv_layer_merged(*inp.merge, 'conv5', inp.z['conv5'].shape[3]))
    if bf:
        for res in synth.RESOLUTIONS:
            out['conv2_pool/conv2_' + res] = bits(eng.conv2_pool(inp.p1[res], 'conv2_' + res))
    out['sm'] = bits(eng.spatial_model(inp.hm10))
    for scope, z in inp.z.items():
        sc, sh = eng.bn_folded(scope, z.shape[3])
        out['bn/%s/scale' % scope], out['bn/%s/shift' % scope] = bits(sc), bits(sh)
        a = eng.act_summary(z, scope, n_pics=1)
        out['act/%s/activ' % scope], out['act/%s/pics' % scope] = bits(a['activ']), bits(a['pics'])
    for scope, k, stride, cin, cout, last in inp.scopes:
        if stride == 2:
            sc, sh = eng.bn_folded(scope, cout)
            out['bn/%s/scale' % scope], out['bn/%s/shift' % scope] = bits(sc), bits(sh)
    t = eng.torso_infer(inp.prob, want_energy=True)
    out['torso/energy'], out['torso/cell'] = bits(t['energy']), bits(t['cell'])
    torch.cuda.synchronize()
    return out


def assert_same(a, f, what, only=None):
    """Two probe results, bit for bit."""
    assert list(a) == list(f), 'the two sequences differ'
    bad = []
    for k in a:
        if only is not None and not only(k):
            continue
        if a[k].shape != f[k].shape or not np.array_equal(a[k], f[k]):
            n = int((a[k] != f[k]).sum()) if a[k].shape == f[k].shape else -1
            bad.append('%s: %d of %d entries differ' % (k, n, a[k].size))
    assert not bad, '%s:\n  %s' % (what, '\n  '.join(bad))


def changed_fraction(a, b):
    return float((a != b).mean())


def matches(name, patterns):
    return any(fnmatch.fnmatchcase(name, p) for p in patterns)
