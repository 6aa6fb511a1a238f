"""Mirrored test-time evaluation on the GPU: jcm_mirror_pairs and jcm_mirror_merge (csrc/mirror.hip) bit for bit against torch.flip
and the numpy restatement (tests/mirror_ref.py, pinned by tests/test_mirror_cpu.py) -- the first copies, the second is a float64 sum in a fixed order,
so there is no tolerance anywhere -- then forward(flip_test=True), the towers, the multi-scale wrapper and the command line, each against the
composition of the calls that existed before."""
import ctypes
import functools
import json
import os

import numpy as np
import pytest
import torch
from numpy.testing import assert_array_equal

import mirror_ref as R
from cli_util import run_cli
import joint_cnn_mrf_amd  # noqa: F401
from joint_cnn_mrf_amd import multiscale as MS
from joint_cnn_mrf_amd import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
FLT_MAX = float(np.finfo(f32).max)
PERM9 = R.HM_FLIP_PERM[:9]


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), device='cuda:0')


def _bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and bool((_bits(a) == _bits(b)).all())


def _pairs(x, dim=2):
    """The 2B interleaved batch made with what existed before: x[b], then torch.flip of it."""
    return torch.stack([x, torch.flip(x, dims=[dim])], dim=1).reshape((2 * x.shape[0],) + tuple(x.shape[1:])).contiguous()


def _params(debug=True):
    p = synth.make_pd_params(debug=debug, bn='trained', conv6_gain=8.0)
    p.update(synth.make_sm_params(synth.synthetic_priors(), kind='trained'))
    return p


@pytest.fixture(scope='module')
def eng():
    """A bare fp32 handle: the two kernels need no parameters."""
    from joint_cnn_mrf_amd.engine import Engine
    e = Engine(device=0)
    yield e
    e.close()


@pytest.fixture(scope='module')
def tower():
    """fp32 handle at --debug width with parameters, 2 byte images, the floats they stand for and their targets."""
    from joint_cnn_mrf_amd.engine import Engine
    e = Engine(device=0).load_params(_params())
    k = np.random.RandomState(5).randint(0, 256, (2, 480, 720, 3)).astype(np.uint8)
    yield e, k, k.astype(f32) / f32(255), synth.make_targets(2, seed=42)
    e.close()


# ------------------------------------------------------------------ mirror_pairs
def _values(shape, dtype, seed):
    """Every bit pattern is fair game for a copy: random words (NaNs, infinities and denormals among the floats) or random bytes."""
    rng = np.random.RandomState(seed)
    if dtype == 'uint8':
        return torch.as_tensor(rng.randint(0, 256, shape).astype(np.uint8), device='cuda:0')
    return torch.as_tensor(rng.randint(-2 ** 31, 2 ** 31, shape, dtype=np.int64).astype(np.int32), device='cuda:0').view(torch.float32)


# the last two: several tiles of an even number of 360-byte rows (16-byte chunks), and the full-size image whose tiles are 3 (float) / 15 (bytes) rows
@pytest.mark.parametrize('shape', [(3, 5, 7, 3), (2, 4, 1, 1), (1, 6, 8, 1), (2, 200, 90, 1), (2, 480, 720, 3)], ids=lambda s: 'x'.join(map(str, s)))
@pytest.mark.parametrize('dtype', ['float32', 'uint8'])
def test_mirror_pairs_is_flip_interleaved_with_the_input(eng, shape, dtype):
    x = _values(shape, dtype, seed=sum(shape))
    got = eng.mirror_pairs(x)
    torch.cuda.synchronize()
    assert got.dtype == x.dtype and tuple(got.shape) == (2 * shape[0],) + shape[1:]
    assert _same_bits(got, _pairs(x))
    if x.numel() < 10000:
        host = x.cpu().numpy()
        ref = R.mirror_pairs(host.view(np.int32) if dtype == 'float32' else host)
        assert_array_equal(got.cpu().numpy().view(ref.dtype), ref)


@pytest.mark.parametrize('dtype', ['float32', 'uint8'])
def test_mirror_pairs_from_a_pointer_off_the_16_byte_grid(eng, dtype):
    """(1,6,8,1) moves as 16-byte chunks from an aligned pointer; one value further on it moves value by value."""
    flat = _values((6 * 8 + 1,), dtype, seed=9)
    x = flat[1:].view(1, 6, 8, 1)
    assert x.is_contiguous() and x.data_ptr() % 16 != 0
    got = eng.mirror_pairs(x)
    torch.cuda.synchronize()
    assert _same_bits(got, _pairs(x))


# ------------------------------------------------------------------ mirror_merge
def _maps(N, HH, WW, K, seed):
    """float32 [N,HH,WW,K]: signed values of every magnitude, with exact zeros, denormals and values near FLT_MAX / 16 mixed in."""
    rng = np.random.RandomState(seed)
    v = (rng.standard_normal((N, HH, WW, K)) * 10.0 ** rng.uniform(-6, 6, (N, HH, WW, K))).astype(f32)
    kind = rng.randint(0, 10, v.shape)
    v[kind == 0] = 0
    v[kind == 1] = (rng.randint(1, 2 ** 23, v.shape).astype(np.uint32).view(f32) * np.where(rng.rand(*v.shape) < 0.5, f32(-1), f32(1)))[kind == 1]      # denormals
    v[kind == 2] = (f32(FLT_MAX / 16) * rng.uniform(0.9, 1.0, v.shape).astype(f32) * np.where(rng.rand(*v.shape) < 0.3, f32(-1), f32(1)))[kind == 2]
    v.reshape(-1)[:3] = [0, np.uint32(12345).view(f32), f32(FLT_MAX / 16) * f32(0.99)]      # ... in every array, however small
    assert (v == 0).any() and ((np.abs(v) < np.finfo(f32).tiny) & (v != 0)).any() and (np.abs(v) > FLT_MAX / 20).any()
    return v


MERGE_MAPS = {'60x90': (60, 90), '7x11': (7, 11), 'one_column': (6, 1)}
MERGE_TABLES = {'K9_flic': (9, None), 'K4_perm': (4, [1, 2, 3, 0])}      # the explicit table is no involution: perm and its inverse differ


@functools.lru_cache(maxsize=None)
def _merge_case(G, n, size, table):
    HH, WW = MERGE_MAPS[size]
    K, perm = MERGE_TABLES[table]
    hm = _maps(n * G, HH, WW, K, seed=G * 100 + n * 10 + HH)
    return hm, perm, R.mirror_merge(hm, G, perm)


@pytest.mark.parametrize('table', sorted(MERGE_TABLES))
@pytest.mark.parametrize('size', sorted(MERGE_MAPS))
@pytest.mark.parametrize('n', [1, 3])
@pytest.mark.parametrize('G', [2, 16])
def test_mirror_merge_equals_the_restatement(eng, G, n, size, table):
    hm, perm, want = _merge_case(G, n, size, table)
    got = eng.mirror_merge(_dev(hm), group=G, perm=perm)
    torch.cuda.synchronize()
    got = got.cpu().numpy()
    assert got.dtype == f32 and got.shape == want.shape
    assert_array_equal(got.view(np.uint32), want.view(np.uint32))
    assert np.isfinite(got).all()


def test_mirror_merge_off_the_16_byte_grid(eng):
    """60x90x9 maps move as float4 from an aligned pointer; from one float further on, one at a time -- the same bits."""
    hm, perm, want = _merge_case(2, 1, '60x90', 'K9_flic')
    flat = torch.empty(hm.size + 1, dtype=torch.float32, device='cuda:0')
    x = flat[1:].view(hm.shape)
    x.copy_(_dev(hm))
    assert x.data_ptr() % 16 != 0
    got = eng.mirror_merge(x)
    torch.cuda.synchronize()
    assert_array_equal(got.cpu().numpy().view(np.uint32), want.view(np.uint32))


def test_swapping_the_members_of_every_pair_mirrors_the_merge(eng):
    """G = 2, the FLIC table (an involution): merge(b, a) is merge(a, b) mirrored with the channels exchanged, bit for bit (a two-term sum
    does not depend on its order)."""
    hm = _dev(_merge_case(2, 3, '7x11', 'K9_flic')[0])
    swapped = hm.view(3, 2, 7, 11, 9).flip(1).reshape(6, 7, 11, 9).contiguous()
    a, b = eng.mirror_merge(hm), eng.mirror_merge(swapped)
    torch.cuda.synchronize()
    assert _same_bits(b, torch.flip(a, dims=[2])[..., PERM9].contiguous())


def test_argument_contract(eng):
    hm = torch.zeros(6, 7, 11, 9, device='cuda:0')
    for group in (3, 1, 0, -2):      # odd, or no pair at all
        with pytest.raises(ValueError, match='even'):
            eng.mirror_merge(hm, group=group)
    with pytest.raises(ValueError, match='whole number of groups'):
        eng.mirror_merge(hm, group=4)
    for perm in ([0, 1, 2, 3, 4, 5, 6, 7, 7], [0, 1, 2], list(range(1, 10)), [0.5] * 9):
        with pytest.raises(ValueError, match='permutation'):
            eng.mirror_merge(hm, perm=perm)
    with pytest.raises(ValueError, match='give perm'):      # the FLIC table cut to 7 channels maps the hips out of range
        eng.mirror_merge(torch.zeros(2, 3, 3, 7, device='cuda:0'))
    for bad in (hm.double(), hm.to(torch.uint8), hm.half()):
        with pytest.raises(ValueError, match='float32'):
            eng.mirror_merge(bad)
    with pytest.raises(ValueError, match='4 dims'):
        eng.mirror_merge(hm[0])
    for bad in (hm.double(), hm.to(torch.int32), hm.half()):
        with pytest.raises(ValueError, match='float32 or uint8'):
            eng.mirror_pairs(bad)
    for bad in (hm[0], hm.unsqueeze(0)):
        with pytest.raises(ValueError, match='4 dims'):
            eng.mirror_pairs(bad)
    # the entry points themselves: a status and a message, nothing launched
    from joint_cnn_mrf_amd import _lib
    p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
    out = torch.full((3, 7, 11, 9), 7.0, device='cuda:0')
    i32 = lambda v: (ctypes.c_int32 * len(v))(*v)
    for args, msg in (((p(hm), 2, 3, 7, 11, 9, None, p(out)), 'G is even'),
                      ((p(hm), 3, 2, 7, 11, 0, None, p(out)), 'K >= 1'),
                      ((p(hm), 3, 2, 7, 11, 9, i32([0, 1, 2, 3, 4, 5, 6, 8, 8]), p(out)), 'not a permutation'),
                      ((p(hm), 3, 2, 7, 11, 9, i32([0, 1, 2, 3, 4, 5, 6, 7, 9]), p(out)), 'not a permutation'),
                      ((p(hm), 1, 2, 7, 11, 12, None, p(out)), 'needs a perm'),
                      ((None, 3, 2, 7, 11, 9, None, p(out)), 'null pointer'),
                      ((p(hm), 3, 2, 7, 11, 9, None, None), 'null pointer')):
        assert eng._lib.jcm_mirror_merge(eng._h, *args) != 0
        assert msg in _lib.last_error(), (msg, _lib.last_error())
    for args, msg in (((None, 0, 3, 7, 11, 9, p(out)), 'null pointer'), ((p(hm), 0, 3, 7, 11, 9, None), 'null pointer'),
                      ((p(hm), 0, 3, 7, 11, 0, p(out)), 'C >= 1'), ((p(hm), 0, 1, 1, 70000, 1, p(out)), '65536')):
        assert eng._lib.jcm_mirror_pairs(eng._h, *args) != 0
        assert msg in _lib.last_error(), (msg, _lib.last_error())
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())      # no refused call wrote anything


# ------------------------------------------------------------------ forward(flip_test=True)
def _check_forward(e, k, y, use_sm=True):
    """forward(flip_test=True) on the byte images k and on the floats they stand for against torch.flip + forward on the 2B batch + the restatement."""
    xb, xf, t = _dev(k), _dev(k.astype(f32) / f32(255)), _dev(y[..., 9:])
    tt = t if use_sm else None
    r2 = e.forward(_pairs(xf), _pairs(t) if use_sm else None, use_sm=use_sm)      # what existed before
    got = e.forward(xf, tt, use_sm=use_sm, flip_test=True)
    got8 = e.forward(xb, tt, use_sm=use_sm, flip_test=True)
    lean = e.forward(xf, tt, use_sm=use_sm, flip_test=True, want_prob=False)
    torch.cuda.synchronize()
    keys = ('pd', 'sm') if use_sm else ('pd',)
    assert list(got) == [key + f for key in keys for f in ('_coords', '_prob')] and list(got8) == list(got)
    assert list(lean) == [key + '_coords' for key in keys]
    for key in keys:
        want = R.mirror_merge(r2[key + '_prob'].cpu().numpy(), 2, PERM9)
        assert tuple(got[key + '_prob'].shape) == (k.shape[0], 60, 90, 9)
        assert_array_equal(got[key + '_prob'].cpu().numpy().view(np.uint32), want.view(np.uint32), err_msg=key)
        coords = e.argmax_coords(_dev(want))
        assert got[key + '_coords'].dtype == torch.int32 and torch.equal(got[key + '_coords'], coords), key
        assert torch.equal(got[key + '_coords'], e.argmax_coords(got[key + '_prob'])), key
        flat = want.reshape(want.shape[0], -1, 9).argmax(axis=1)      # first occurrence, as the kernel
        assert_array_equal(got[key + '_coords'].cpu().numpy(), np.stack([flat // 90, flat % 90], axis=1))
        assert torch.equal(lean[key + '_coords'], got[key + '_coords']), key
    for name in got:      # the byte forward: the same bits as for the float image
        assert _same_bits(got8[name], got[name]), name
    return got


def _check_self_mirrored(e, k, y):
    """An image that is its own mirror image, with a symmetric torso map: the merged maps are their own mirror image with the channels exchanged."""
    half, thalf = _dev(k[:, :, :360].astype(f32) / f32(255)), _dev(y[:, :, :45, 9:])
    x, t = torch.cat([half, torch.flip(half, dims=[2])], dim=2).contiguous(), torch.cat([thalf, torch.flip(thalf, dims=[2])], dim=2).contiguous()
    assert torch.equal(x, torch.flip(x, dims=[2])) and torch.equal(t, torch.flip(t, dims=[2]))
    r = e.forward(x, t, use_sm=True, flip_test=True)
    torch.cuda.synchronize()
    for key in ('pd_prob', 'sm_prob'):
        assert _same_bits(r[key], torch.flip(r[key], dims=[2])[..., PERM9].contiguous()), key


def test_forward_flip_test_debug_size(tower):
    e, k, xf, y = tower
    _check_forward(e, k, y)
    _check_forward(e, k, y, use_sm=False)
    _check_self_mirrored(e, k, y)
    x, t = _dev(xf), _dev(y[..., 9:])
    plain, off = e.forward(x, t), e.forward(x, t, flip_test=False)
    torch.cuda.synchronize()
    assert list(off) == list(plain)
    for name in plain:
        assert _same_bits(off[name], plain[name]), name
    with pytest.raises(ValueError, match='torso'):
        e.forward(x, None, use_sm=True, flip_test=True)


@pytest.mark.parametrize('precision', ['fp32', 'bf16'])
def test_forward_flip_test_full_size(precision):
    from joint_cnn_mrf_amd.engine import Engine
    e = Engine(device=0, precision=precision).load_params(_params(debug=False))
    k = np.random.RandomState(6).randint(0, 256, (1, 480, 720, 3)).astype(np.uint8)
    y = synth.make_targets(1, seed=43)
    _check_forward(e, k, y)
    _check_self_mirrored(e, k, y)
    e.close()


def test_peaks_and_decode_work_on_the_merged_maps(tower):
    e, k, xf, y = tower
    x, t = _dev(xf), _dev(y[..., 9:])
    r = e.forward(x, t, use_sm=True, peaks=4, decode=True, flip_test=True)
    lean = e.forward(x, t, use_sm=True, peaks=4, decode=True, flip_test=True, want_prob=False)
    plain = e.forward(x, t, use_sm=True, flip_test=True)
    torch.cuda.synchronize()
    assert sorted(r) == sorted(list(plain) + ['pd_peaks', 'sm_peaks', 'pose'])
    assert sorted(lean) == ['pd_coords', 'pd_peaks', 'pose', 'sm_coords', 'sm_peaks']
    for name in plain:
        assert _same_bits(r[name], plain[name]), name
    for key in ('pd', 'sm'):
        want = e.hm_peaks(r[key + '_prob'], max_peaks=4)
        for f in want:
            assert _same_bits(r[key + '_peaks'][f], want[f]) and _same_bits(lean[key + '_peaks'][f], want[f]), (key, f)
        assert tuple(want['cells'].shape) == (2, 9, 4, 2)
    pose = e.pose_decode(torch.cat([r['pd_prob'], t], dim=3), r['pd_peaks'])      # the merged maps and the UNMIRRORED torso map
    torch.cuda.synchronize()
    for f in pose:
        assert _same_bits(r['pose'][f], pose[f]) and _same_bits(lean['pose'][f], pose[f]), f
    assert bool((r['pose']['index'] >= 0).all())


def test_towers_mirror_their_own_slices(tower):
    """Two in-process towers on the one device, one image each, against one engine on both images."""
    from joint_cnn_mrf_amd.dist import Towers
    e, k, xf, y = tower
    tw = Towers(_params(), [0, 0])
    try:
        got = tw.forward(xf, y[:, :, :, 9:], use_sm=True, want_prob=True, flip_test=True)
        got8 = tw.forward(k, y[:, :, :, 9:], use_sm=True, want_prob=True, flip_test=True)
        want = e.forward(_dev(xf), _dev(y[..., 9:]), use_sm=True, flip_test=True)
        torch.cuda.synchronize()
        assert sorted(got) == sorted(want)
        for name in want:
            assert _same_bits(got[name], want[name]) and _same_bits(got8[name], want[name]), name
    finally:
        tw.close()


# ------------------------------------------------------------------ the multi-scale wrapper
def _compose_multiscale(e, X, Y, per_forward):
    """get_predictions(flip_test=True) step by step from what existed before and the restatement -> (pd, sm) merged maps [N,60,90,9] (host)."""
    back = MS._back_windows(MS.PAD_ARRAY, MS.CROP_ARRAY, 60, 90)
    out = {'pd': [], 'sm': []}
    for i0 in range(0, X.shape[0], per_forward):
        x, y = _dev(X[i0:i0 + per_forward]), _dev(Y[i0:i0 + per_forward])
        xs = _pairs(MS.get_different_scales(e, x, MS.PAD_ARRAY, MS.CROP_ARRAY, 480, 720))              # scale first, then mirror: 16 per image
        torso = _pairs(y[:, :, :, 9:].repeat_interleave(8, dim=0).contiguous())
        r = e.forward(xs, torso, use_sm=True)
        windows = [(i,) + back[(i // 2) % 8] for i in range(xs.shape[0])]                              # copy 2s + j takes the window of scale s
        for key in out:
            scaled = e.window_resize(r[key + '_prob'], windows, 60, 90)
            torch.cuda.synchronize()
            out[key].append(R.mirror_merge(scaled.cpu().numpy(), 16, PERM9))
    return np.concatenate(out['pd']), np.concatenate(out['sm'])


@pytest.mark.parametrize('per_forward', [1, 2])
def test_get_predictions_flip_test(tower, per_forward):
    e, k, X, Y = tower
    pd, sm, pk_pd, pk_sm = MS.get_predictions(e, X, Y, use_sm=True, images_per_forward=per_forward, peaks=2, flip_test=True)
    torch.cuda.synchronize()
    assert pd.shape == (2, 9, 2) and sm.shape == (2, 9, 2)
    composed = _compose_multiscale(e, X, Y, per_forward)
    for coords, pk, want in zip((pd, sm), (pk_pd, pk_sm), composed):
        flat = want.reshape(2, -1, 9).argmax(axis=1)                                                   # [N,K], first occurrence
        assert_array_equal(coords, np.stack([flat // 90, flat % 90], axis=0).transpose(0, 2, 1))        # [2,K,N]
        ref = e.hm_peaks(_dev(want), max_peaks=2)      # the averaged maps themselves: the peaks' scores are their bits at the peaks' cells
        for f in ref:
            assert _same_bits(pk[f], ref[f]), f
    if per_forward == 2:      # and the library's own steps on the way give those maps, every bit
        x, y = _dev(X), _dev(Y)
        xs = e.mirror_pairs(MS.get_different_scales(e, x, MS.PAD_ARRAY, MS.CROP_ARRAY, 480, 720))
        torso = e.mirror_pairs(y[:, :, :, 9:].repeat_interleave(8, dim=0).contiguous())
        r = e.forward(xs, torso, use_sm=True)
        for key, want in zip(('pd', 'sm'), composed):
            got = e.mirror_merge(MS.scale_hm_back(e, r[key + '_prob'], MS.PAD_ARRAY, MS.CROP_ARRAY, 60, 90, copies_per_scale=2), group=16)
            torch.cuda.synchronize()
            assert_array_equal(got.cpu().numpy().view(np.uint32), want.view(np.uint32), err_msg=key)
    plain = MS.get_predictions(e, X, Y, use_sm=True, images_per_forward=per_forward)
    off = MS.get_predictions(e, X, Y, use_sm=True, images_per_forward=per_forward, flip_test=False)
    assert_array_equal(off[0], plain[0])
    assert_array_equal(off[1], plain[1])


# ------------------------------------------------------------------ the command line
CLI_CASES = {
    'single_scale': (['--batch_size', '2', '--synthetic_size', '4', '--peaks', '2', '--decode_pose'], 4),
    'multiscale': (['--multiscale', '--batch_size', '2', '--synthetic_size', '2', '--peaks', '2'], 2),
    'byte_images': (['--u8_images', '--batch_size', '2', '--synthetic_size', '4'], 4),
}


@pytest.mark.parametrize('case', sorted(CLI_CASES))
def test_cli_flip_test(tmp_path, case):
    import scipy.io
    extra, n = CLI_CASES[case]
    mat, curve = str(tmp_path / 'P.mat'), str(tmp_path / 'C.json')
    r = run_cli(['--debug', '--synthetic', '--use_sm', '--gpus', '0', '--flip_test', '--predictions', mat, '--det_curve', curve] + extra, str(tmp_path))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line['flip_test'] is True and line['n_images'] == n and line['multiscale'] == (case == 'multiscale')
    m = scipy.io.loadmat(mat)
    assert m['flic_pred_pd'].shape == (2, 9, n) and m['flic_pred_sm'].shape == (2, 9, n)
    assert json.load(open(curve))['n_images'] == n
    if '--peaks' in extra:
        assert m['flic_peaks_pd'].shape == (n, 9, 2, 3) and m['flic_peaks_sm'].shape == (n, 9, 2, 3)
        assert_array_equal(np.round(m['flic_peaks_sm'][:, :, 0, :2] / 8).astype(m['flic_pred_sm'].dtype).transpose(2, 1, 0), m['flic_pred_sm'])
    if '--decode_pose' in extra:
        assert m['flic_pred_pose'].shape == (2, 9, n) and 'pose_changed' in line
    if case == 'byte_images':
        assert line['image_dtype'] == 'uint8' and line['bytes_uploaded'] == n * (480 * 720 * 3 + 60 * 90 * 4)


def test_cli_refuses_flip_test_with_train(tmp_path):
    r = run_cli(['--train', '--flip_test', '--debug', '--synthetic', '--gpus', '0'], str(tmp_path))
    assert r.returncode != 0 and '--flip_test' in r.stderr
