"""The handle's options (jcm_set_option / jcm_get_option; csrc/options.h): every key of the table in include/jcm.h round-trips with the documented
default and range, the three keys that shape the parameters are refused after jcm_finalize, the environment supplies defaults at jcm_create only, and
an option belongs to its handle -- nothing process-wide is left."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import joint_cnn_mrf_amd  # noqa: F401
from joint_cnn_mrf_amd import _lib
from oracle import jcm_oracle as O

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, ERR_ARG, ERR_STATE = 0, 1, 2
INT_MAX = 2 ** 31 - 1


def documented_options():
    """The rows of the option table in include/jcm.h: key -> dict(default, kind, lo, hi, before, env).  kind: 'bool' (any non-zero value is stored
    as 1), 'range' (lo..hi; no hi = INT_MAX), 'either' (lo|hi)."""
    text = open(os.path.join(ROOT, 'include', 'jcm.h')).read()
    rows = {}
    for m in re.finditer(r'^ \*   "(\w+)"\s+(-?\d+)\s+(\S+)\s+(any|before)\s+(\S+)\s+\S', text, flags=re.M):
        key, default, rng, when, env = m.groups()
        if rng == 'bool':
            kind, lo, hi = 'bool', 0, 1
        elif '|' in rng:
            kind, (lo, hi) = 'either', map(int, rng.split('|'))
        else:
            kind = 'range'
            lo, hi = rng.split('..')
            lo, hi = int(lo), int(hi) if hi else INT_MAX
        rows[key] = dict(default=int(default), kind=kind, lo=lo, hi=hi, before=when == 'before', env=None if env == '-' else env)
    return rows


def raw_set(eng, key, value):
    return eng._lib.jcm_set_option(eng._h, key.encode(), int(value))


def raw_get(eng, key):
    v = ctypes.c_int64(-12345)
    return eng._lib.jcm_get_option(eng._h, key.encode(), ctypes.byref(v)), v.value


def test_header_table_lists_every_option():
    """The table is complete: the keys documented are the 19 of before this table existed plus fft_reg and fft_cache_gb, and the environment
    defaults are the four that survive."""
    rows = documented_options()
    assert sorted(rows) == sorted(['precision', 'n_joints', 'f32_conv', 'split_min_wgs', 'profile', 'conv9_fft', 'call_order', 'fft_single', 'fft_t16',
                                   'fft_rows_mfma', 'fft_windows', 'fft_fuse', 'fft_tiles', 'fft_logits_rows', 'fft_reg', 'fft_cache_gb', 'bf16_hpool',
                                   'sm_algo', 'sm_chunk', 'micro_batch', 'debug_skip'])
    assert {k: r['env'] for k, r in rows.items() if r['env']} == {'fft_tiles': 'JCM_FFT_TILES', 'fft_logits_rows': 'JCM_FFT_LOGITS_ROWS',
                                                                   'fft_reg': 'JCM_FFT_REG', 'fft_cache_gb': 'JCM_FFT_CACHE_GB'}
    assert [k for k, r in rows.items() if r['before']] == ['precision', 'n_joints', 'f32_conv']


def test_round_trip_of_every_key():
    """Fresh handle without parameters: the documented default; both ends of the range round-trip; a value outside the range is JCM_ERR_ARG and
    leaves the stored value alone; an unknown key is JCM_ERR_ARG for set and get.  A boolean key has no value outside its range (jcm.h: any non-zero
    value is stored as 1), so for those the test holds that instead."""
    from joint_cnn_mrf_amd.engine import Engine
    env_named = [r['env'] for r in documented_options().values() if r['env']]
    assert not any(v in os.environ for v in env_named), 'the defaults are tested without the environment overrides'
    eng = Engine(device=0)
    for key, r in documented_options().items():
        assert raw_get(eng, key) == (OK, r['default']), key
        assert eng.get_option(key) == r['default']
        for end in (r['hi'], r['lo']):
            assert raw_set(eng, key, end) == OK, (key, end)
            assert raw_get(eng, key) == (OK, end), (key, end)
        if r['kind'] == 'bool':
            assert raw_set(eng, key, 5) == OK and raw_get(eng, key) == (OK, 1), key
            assert raw_set(eng, key, -1) == OK and raw_get(eng, key) == (OK, 1), key
        else:
            outside = [r['lo'] - 1] + ([r['hi'] + 1] if r['hi'] < INT_MAX else []) + ([r['lo'] + 1] if r['kind'] == 'either' else [])
            for bad in outside:
                assert raw_set(eng, key, bad) == ERR_ARG, (key, bad)
                assert key in _lib.last_error()
                assert raw_get(eng, key) == (OK, r['lo']), (key, bad)
        assert raw_set(eng, key, r['default']) == OK
    assert raw_set(eng, 'no_such_option', 1) == ERR_ARG and 'no_such_option' in _lib.last_error()
    assert raw_get(eng, 'no_such_option') == (ERR_ARG, -12345)
    with pytest.raises(RuntimeError, match='jcm_get_option'):
        eng.get_option('no_such_option')
    eng.close()


def test_finalize_gate():
    """After jcm_finalize (debug-width synthetic parameters) precision, f32_conv and n_joints are JCM_ERR_STATE and keep their values; every other key is
    still accepted."""
    from joint_cnn_mrf_amd import synth
    from joint_cnn_mrf_amd.engine import Engine
    eng = Engine(device=0).load_params(synth.make_pd_params(debug=True, bn='trained'))
    rows = documented_options()
    for key, r in rows.items():
        other = r['hi'] if r['default'] != r['hi'] else r['lo']
        if key in ('precision', 'f32_conv', 'n_joints'):
            assert raw_set(eng, key, other) == ERR_STATE, key
            assert 'jcm_finalize' in _lib.last_error()
            assert raw_get(eng, key) == (OK, r['default']), key
        else:
            assert raw_set(eng, key, other) == OK, key
            assert raw_get(eng, key) == (OK, other), key
    eng.close()


_CHILD = """
import json
import joint_cnn_mrf_amd
from joint_cnn_mrf_amd.engine import Engine
eng = Engine(device=0)
keys = ('fft_reg', 'fft_tiles', 'fft_logits_rows', 'fft_cache_gb')
first = [eng.get_option(k) for k in keys]
eng.set_option('fft_tiles', 1)
print('RESULT ' + json.dumps([first, eng.get_option('fft_tiles'), [Engine(device=0).get_option(k) for k in keys]]))
"""


def _child(extra_env):
    import json
    env = {k: v for k, v in os.environ.items() if k not in ('JCM_FFT_REG', 'JCM_FFT_TILES', 'JCM_FFT_LOGITS_ROWS', 'JCM_FFT_CACHE_GB')}
    env.update(extra_env, PYTHONPATH=os.pathsep.join([ROOT] + sys.path))
    r = subprocess.run([sys.executable, '-c', _CHILD], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and 'RESULT ' in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    return json.loads(r.stdout.split('RESULT ', 1)[1])


def test_environment_seeds_the_defaults():
    """A fresh process with the four variables set: a new handle shows them, an explicit set_option wins over the environment, and a second handle is
    seeded again.  A process without them shows the documented defaults."""
    first, tiles_after_set, second = _child({'JCM_FFT_REG': '0', 'JCM_FFT_TILES': '0', 'JCM_FFT_LOGITS_ROWS': '0', 'JCM_FFT_CACHE_GB': '3'})
    assert first == [0, 0, 0, 3]
    assert tiles_after_set == 1
    assert second == [0, 0, 0, 3]
    first, tiles_after_set, second = _child({})
    rows = documented_options()
    assert first == second == [rows[k]['default'] for k in ('fft_reg', 'fft_tiles', 'fft_logits_rows', 'fft_cache_gb')] == [1, 1, 1, 64]
    assert tiles_after_set == 1


def test_fft_reg_belongs_to_the_handle():
    """Two fp32 engines in one process, one with fft_reg = 0, run one 9x9 layer (64 -> 64 channels, 2 images of 20 x 28: the 24 x 32 transform, the
    smallest whose inverse row pass exists both as a register kernel -- cfft_rows_inv_reg takes 32-point rows of fp32 outputs -- and as an LDS kernel).
    Both are within the bound of this route in test_gpu_random_shapes.py, 2e-5 of the float64 reference's max; a third engine with the default
    reproduces the first bit for bit, so the second engine's option did not leak into the process."""
    from joint_cnn_mrf_amd.engine import Engine
    from test_gpu_random_shapes import layer_params
    rs = np.random.RandomState(77)
    p = layer_params(rs, 64, 64, 9)
    x = rs.standard_normal((2, 20, 28, 64)).astype(np.float32)
    ref = O.conv_layer(x.astype(np.float64), p, 9, 1, 'c')
    xd = torch.as_tensor(x, device='cuda:0')
    got = []
    for reg in (None, 0, None):
        eng = Engine(device=0).load_params(p)
        if reg is not None:
            eng.set_option('fft_reg', reg)
        assert eng.get_option('fft_reg') == (1 if reg is None else reg)
        assert eng.conv_kernel_name('c', 2, 20, 28).startswith('conv_fft')
        got.append(eng.conv_layer(xd, 'c', 1, n_out=64).cpu().numpy())
        eng.close()
    for g in got:
        err = np.abs(g - ref).max() / np.abs(ref).max()
        print('fft_reg layer error: %.3e' % err)
        assert err <= 2e-5
    assert np.array_equal(got[0], got[2])


def _tower_engine(precision, debug=True, **kw):
    """A part-detector engine and one 64 x 96 image.  debug: the debug widths (16/32/64/128/128 filters), where conv4_*, conv5 and conv6 have
    Cin % 64 == 0 and run in the frequency domain, so a forward fills the filter-spectra cache with entries of three map sizes."""
    from joint_cnn_mrf_amd import synth
    from joint_cnn_mrf_amd.engine import Engine
    eng = Engine(device=0, precision=precision, **kw).load_params(synth.make_pd_params(debug=debug))
    return eng, torch.as_tensor(synth.make_images(1, seed=31, height=64, width=96), device='cuda:0')


def test_filter_spectra_cache_eviction_repacks_the_same_spectra():
    """fft_cache_gb = 0: a key that is not cached drops all others (stream synchronise, free, clear) before it is packed.
    On the engine that has run a forward with the default bound every key of this image is cached, so the bound of 0 set afterwards evicts nothing:
    its two further forwards only hold that the option leaves cached spectra alone.  The eviction is crossed on a SECOND engine that gets the bound
    before its first forward: the branches' layers have different map sizes, so every forward there drops, synchronises and re-packs several times
    (after the first forward only the last key is held).  All five results are the logits under the default bound, bit for bit."""
    eng, x = _tower_engine('fp32')
    assert eng.conv_kernel_name('conv5', 1, 8, 12).startswith('conv_fft')
    want = eng.model(x).clone()
    eng.set_option('fft_cache_gb', 0)
    for _ in range(2):
        assert torch.equal(eng.model(x), want)
    eng.close()
    tight, _ = _tower_engine('fp32')
    tight.set_option('fft_cache_gb', 0)
    for _ in range(2):
        assert torch.equal(tight.model(x), want)
    tight.close()


def test_fft_single_change_drops_the_filter_spectra():
    """bf16 handle: the cached spectra are packed for one operand form.  set_option('fft_single', 0) behind a forward drops them, and the next forward
    equals that of a fresh engine created with fft_single = False, bit for bit; back at 1 the first result comes again.  (The full-width tower: a
    bf16 handle refuses the debug widths at jcm_finalize, "bf16 path needs Cin % 32 == 0" -- conv2 has Cin = 16 there.  Same image, same assertions.)"""
    eng, x = _tower_engine('bf16', debug=False)
    assert eng.conv_kernel_name('conv5', 1, 8, 12).startswith('conv_fft')
    first = eng.model(x).clone()
    eng.set_option('fft_single', 0)
    two_parts = eng.model(x).clone()
    fresh, _ = _tower_engine('bf16', debug=False, fft_single=False)
    assert torch.equal(two_parts, fresh.model(x))
    fresh.close()
    eng.set_option('fft_single', 1)
    assert torch.equal(eng.model(x), first)
    eng.close()
