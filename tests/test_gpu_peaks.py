"""Heat-map peaks on the GPU: jcm_hm_peaks (csrc/peaks.hip) against the numpy restatement (tests/peaks_ref.py, pinned by
tests/test_peaks_cpu.py) with assert_array_equal on all four outputs -- the kernel compares and copies, it does no arithmetic, so there is
no tolerance -- then forward(peaks=), the multi-scale wrapper and the command line."""
import json
import os

import numpy as np
import pytest
import torch
from numpy.testing import assert_array_equal

import peaks_ref as R
from cli_util import run_cli
import joint_cnn_mrf_amd  # noqa: F401
from joint_cnn_mrf_amd import multiscale, synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ('cells', 'offsets', 'scores', 'count')


@pytest.fixture(scope='module')
def eng():
    """A bare fp32 handle: the peaks kernel needs no parameters."""
    from joint_cnn_mrf_amd.engine import Engine
    e = Engine(device=0)
    yield e
    e.close()


@pytest.fixture(scope='module')
def tower():
    """fp32 handle at --debug width with parameters, and 2 images with their targets."""
    from joint_cnn_mrf_amd.engine import Engine
    p = synth.make_pd_params(debug=True, bn='trained', conv6_gain=8.0)
    p.update(synth.make_sm_params(synth.synthetic_priors(), kind='trained'))
    e = Engine(device=0).load_params(p)
    yield e, synth.make_images(2, seed=41), synth.make_targets(2, seed=42)
    e.close()


@pytest.fixture(scope='module')
def noise():
    """[3,60,90,9]: the logits 3 * N(0,1) and their spatial softmax."""
    logits = (3 * np.random.RandomState(1234).standard_normal((3, 60, 90, 9))).astype(np.float32)
    return logits, R.softmax_maps(logits)


def _dev(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), device='cuda:0', dtype=dtype)


def _host(r):
    torch.cuda.synchronize()
    return {k: r[k].cpu().numpy() for k in KEYS}


def _check(eng, hm, P, threshold=0.0, cand=None):
    """hm_peaks of the host array hm against the restatement, all four outputs bit for bit; peak 0 against the library's own arg-max."""
    t = _dev(hm)
    kw = {} if threshold == 0.0 else {'threshold': threshold}
    got = _host(eng.hm_peaks(t, max_peaks=P, **kw))
    want = R.hm_peaks(hm, P, threshold, cand=cand)
    assert sorted(got) == sorted(KEYS)
    for k in KEYS:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, k
        if got[k].dtype == np.float32:
            assert_array_equal(got[k].view(np.uint32), want[k].view(np.uint32), err_msg=k)      # the bits: -0.0 is not 0.0, the scores are the input's
        else:
            assert_array_equal(got[k], want[k], err_msg=k)
    am = eng.argmax_coords(t).cpu().numpy().transpose(0, 2, 1)      # [B,K,2]
    has = got['count'] > 0
    assert_array_equal(got['cells'][:, :, 0][has], am[has])
    return got


def test_noise_maps_fill_every_slot(eng, noise):
    got = _check(eng, noise[1], 8)
    assert (got['count'] == 8).all()                          # hundreds of local maxima per map: the test cannot pass on empty output
    assert (got['cells'] >= 0).all() and (np.diff(got['scores'], axis=2) <= 0).all()
    assert (np.abs(got['offsets']) == 0.25).any() and set(np.unique(got['offsets'])) <= {-0.25, 0.0, 0.25}


def test_four_levels_ties_and_plateaus(eng, noise):
    """np.round(x * 3) / 3 gives four levels for x in [0,1].  Nearly every probability of a 5400-pixel map is below 1/6, so the quantised
    probabilities are one plateau of zeros with a few pixels of 1/3 or 2/3 in it: few peaks above the default threshold, and the first pixel
    of the plateau as well under a negative one.  The logits squashed to (0,1) give all four levels with ties and plateaus everywhere."""
    logits, prob = noise
    flat = (np.round(prob * 3) / 3).astype(np.float32)
    assert 0 < (flat > 0).sum() < 100
    assert (_check(eng, flat, 8)['count'] < 8).all()
    assert (_check(eng, flat, 8, threshold=-1.0)['count'] >= 1).all()
    x = (1 / (1 + np.exp(-logits / 3))).astype(np.float32)
    q = (np.round(x * 3) / 3).astype(np.float32)
    assert len(np.unique(q)) == 4
    got = _check(eng, q, 8)
    assert (got['count'] == 8).all()
    assert (got['scores'][:, :, 0] == got['scores'][:, :, 1]).all()      # ties: the order within them is by index
    idx = got['cells'][..., 0].astype(np.int64) * 90 + got['cells'][..., 1]
    tied = np.diff(got['scores'], axis=2) == 0
    assert (np.diff(idx, axis=2)[tied] > 0).all()


def test_underflowed_softmax_regions_of_exact_zeros(eng, noise):
    prob40 = R.softmax_maps(40 * noise[0])
    assert (prob40 == 0).mean() > 0.5
    got = _check(eng, prob40, 8)
    assert (got['count'] >= 1).all() and (got['count'] < 8).any()      # a few isolated survivors per map: filler slots appear
    got = _check(eng, prob40, 8, threshold=-np.inf)          # now the first pixel of every zero plateau counts too
    assert (got['scores'] == 0).any()


def test_threshold_above_every_value_gives_filler(eng, noise):
    got = _check(eng, noise[1], 4, threshold=2.0)
    assert (got['count'] == 0).all() and (got['cells'] == -1).all() and (got['offsets'] == 0).all() and (got['scores'] == 0).all()


def _geometry_input(B, H, W, K):
    """Image 0: softmax of noise; image 1: four levels with ties and plateaus (the values k/3); a further image: sparse spikes on zeros."""
    rs = np.random.RandomState(1000 * H + 10 * W + K)
    hm = np.empty((B, H, W, K), np.float32)
    hm[0] = R.softmax_maps(3 * rs.standard_normal((1, H, W, K)))[0]
    if B > 1:
        hm[1] = rs.randint(0, 4, (H, W, K)).astype(np.float32) / np.float32(3)
    for b in range(2, B):
        hm[b] = (rs.random_sample((H, W, K)) < 0.2) * rs.random_sample((H, W, K))
    return hm


# (B, HH, WW): single pixels, single rows and columns (an axis that is always clipped), 2x2 (every pixel a corner), 7x11 (odd, one partial
# sweep of the threads), 61x91 (odd, not a multiple of 4, more pixels than threads), 120x180 (the size limit: one map per work group).
# K = 1, 9, 10: one map; the model's count (three groups of 3 at 60x90); a count that leaves a last group of one map.  With K = 9 or 10 the
# odd sizes are no multiple of 4 floats per image: the general path of the loads.
GEOMETRIES = [(3, 1, 1), (3, 1, 5), (3, 5, 1), (3, 2, 2), (3, 7, 11), (2, 61, 91), (2, 120, 180)]


@pytest.mark.parametrize('K', [1, 9, 10])
@pytest.mark.parametrize('geom', GEOMETRIES, ids=lambda g: '%dx%dx%d' % (g[1], g[2], g[0]))
def test_awkward_geometries(eng, geom, K):
    B, H, W = geom
    hm = _geometry_input(B, H, W, K)
    cand = R.all_local_maxima(hm)                             # once per input; the three P share it
    for P in (1, 3, 8):
        got = _check(eng, hm, P, cand=cand)
        assert (got['count'] > 0).any()


def test_unaligned_input_takes_the_general_path(eng, noise):
    """A view that starts 4 bytes into an allocation: 16-byte loads are not possible, the result is the same."""
    hm = noise[1][:1]
    flat = torch.zeros(hm.size + 1, device='cuda:0')
    flat[1:] = _dev(hm).reshape(-1)
    v = flat[1:].view(hm.shape)
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    got = _host(eng.hm_peaks(v, max_peaks=8))
    want = R.hm_peaks(hm, 8)
    for k in KEYS:
        assert_array_equal(got[k], want[k], err_msg=k)


def test_refusals_touch_no_output(eng):
    import ctypes
    big = torch.zeros(1, 121, 180, 2, device='cuda:0')
    with pytest.raises(RuntimeError, match=r'jcm_hm_peaks failed.*21600'):
        eng.hm_peaks(big, max_peaks=4)
    ok = torch.zeros(1, 6, 7, 2, device='cuda:0')
    for P in (0, 9, -1):
        with pytest.raises(RuntimeError, match=r'jcm_hm_peaks failed.*1 <= P <= 8'):
            eng.hm_peaks(ok, max_peaks=P)
    with pytest.raises(ValueError, match='hm is on cpu'):
        eng.hm_peaks(torch.zeros(1, 6, 7, 2), max_peaks=4)
    # the C entry itself, on tensors with a known filling
    cells = torch.full((1, 2, 4, 2), 7, dtype=torch.int32, device='cuda:0')
    offsets = torch.full((1, 2, 4, 2), 7.0, device='cuda:0')
    scores = torch.full((1, 2, 4), 7.0, device='cuda:0')
    count = torch.full((1, 2), 7, dtype=torch.int32, device='cuda:0')
    torch.cuda.synchronize()
    p = eng._p
    rc = eng._lib.jcm_hm_peaks(eng._h, p(big), 1, 121, 180, 2, 4, ctypes.c_float(0.0), p(cells), p(offsets), p(scores), p(count))
    assert rc != 0
    torch.cuda.synchronize()
    for t in (cells, offsets, scores, count):
        assert int((t != 7).sum()) == 0
    # offsets may be NULL: the other three are written as usual
    hm = _geometry_input(2, 7, 11, 2)
    cells = torch.empty(2, 2, 4, 2, dtype=torch.int32, device='cuda:0')
    scores = torch.empty(2, 2, 4, device='cuda:0')
    count = torch.empty(2, 2, dtype=torch.int32, device='cuda:0')
    t = _dev(hm)
    torch.cuda.synchronize()
    rc = eng._lib.jcm_hm_peaks(eng._h, p(t), 2, 7, 11, 2, 4, ctypes.c_float(0.0), p(cells), p(None), p(scores), p(count))
    assert rc == 0
    torch.cuda.synchronize()
    want = R.hm_peaks(hm, 4)
    assert_array_equal(cells.cpu().numpy(), want['cells'])
    assert_array_equal(scores.cpu().numpy(), want['scores'])
    assert_array_equal(count.cpu().numpy(), want['count'])


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and bool((a.view(torch.int32) == b.view(torch.int32)).all())


@pytest.mark.parametrize('entry', ['forward', 'eval_forward'])
def test_forward_with_peaks(tower, entry):
    e, X, Y = tower
    x, y = _dev(X), _dev(Y)

    def call(**kw):
        r = e.forward(x, y[:, :, :, 9:].contiguous(), use_sm=True, **kw) if entry == 'forward' else e.eval_forward(x, y, use_sm=True, **kw)
        torch.cuda.synchronize()
        return r
    for want_prob in (True, False):
        plain = call(want_prob=want_prob)
        with_pk = call(want_prob=want_prob, peaks=4)
        assert sorted(with_pk) == sorted(list(plain) + ['pd_peaks', 'sm_peaks'])
        for k in plain:
            assert _same_bits(plain[k], with_pk[k]), k
        if want_prob:
            probs = with_pk
        for key in ('pd', 'sm'):
            want = _host(e.hm_peaks(probs[key + '_prob'], max_peaks=4))      # (want_prob=False: the probabilities of the first pass, the same bits)
            got = _host(with_pk[key + '_peaks'])
            for f in KEYS:
                assert_array_equal(got[f], want[f], err_msg=key + f)
            assert got['cells'].shape == (2, 9, 4, 2) and (got['count'] >= 1).all()
            assert_array_equal(got['cells'][:, :, 0].transpose(0, 2, 1), with_pk[key + '_coords'].cpu().numpy())
            ref = R.hm_peaks(probs[key + '_prob'].cpu().numpy(), 4)
            for f in KEYS:
                assert_array_equal(got[f], ref[f], err_msg=key + f)
    no_sm = e.forward(x, None, use_sm=False, peaks=2)
    assert 'pd_peaks' in no_sm and 'sm_peaks' not in no_sm


def test_towers_concatenate_peaks(tower):
    """Two in-process towers on the one device, one image each: the peaks of the batch in tower order."""
    from joint_cnn_mrf_amd.dist import Towers
    e, X, Y = tower
    p = synth.make_pd_params(debug=True, bn='trained', conv6_gain=8.0)
    p.update(synth.make_sm_params(synth.synthetic_priors(), kind='trained'))
    tw = Towers(p, [0, 0])
    try:
        plain = tw.forward(X, Y[:, :, :, 9:], use_sm=True, want_prob=True)
        r = tw.forward(X, Y[:, :, :, 9:], use_sm=True, want_prob=True, peaks=3)
        torch.cuda.synchronize()
        assert sorted(r) == sorted(list(plain) + ['pd_peaks', 'sm_peaks'])
        for k in plain:
            assert _same_bits(plain[k], r[k]), k
        for key in ('pd', 'sm'):
            got, want = _host(r[key + '_peaks']), _host(e.hm_peaks(r[key + '_prob'], max_peaks=3))
            for f in KEYS:
                assert got[f].shape[0] == 2
                assert_array_equal(got[f], want[f], err_msg=key + f)
    finally:
        tw.close()


def test_multiscale_with_peaks(tower):
    e, X, Y = tower
    pd, sm = multiscale.get_predictions(e, X, Y, use_sm=True, images_per_forward=2)
    r = multiscale.get_predictions(e, X, Y, use_sm=True, images_per_forward=2, peaks=2)
    assert len(r) == 4
    assert_array_equal(r[0], pd)
    assert_array_equal(r[1], sm)
    for coords, pk in ((pd, r[2]), (sm, r[3])):
        got = _host(pk)
        assert got['cells'].shape == (2, 9, 2, 2) and got['offsets'].shape == (2, 9, 2, 2) and got['scores'].shape == (2, 9, 2) and got['count'].shape == (2, 9)
        assert (got['count'] >= 1).all()
        assert_array_equal(got['cells'][:, :, 0].transpose(2, 1, 0), coords)      # [N,K,2] -> [2,K,N]
    one = multiscale.get_predictions(e, X, Y, use_sm=True, images_per_forward=1, peaks=2)      # collected over two image groups
    assert one[2]['cells'].shape == (2, 9, 2, 2)
    assert_array_equal(one[2]['cells'][:, :, 0].cpu().numpy().transpose(2, 1, 0), one[0])


def _run_ok(args, cwd):
    r = run_cli(args, cwd)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return r.stdout


def test_cli_writes_the_peaks_of_its_predictions(tmp_path):
    import scipy.io
    args = ['--debug', '--synthetic', '--use_sm', '--batch_size', '4', '--synthetic_size', '8', '--gpus', '0']
    with_pk, without = str(tmp_path / 'P.mat'), str(tmp_path / 'Q.mat')
    out = _run_ok(args + ['--predictions', with_pk, '--peaks', '3'], str(tmp_path))
    m = scipy.io.loadmat(with_pk)
    line = json.loads(out.strip().splitlines()[-1])
    assert line['peaks'] == 3 and line['n_images'] == 8
    for key in ('pd', 'sm'):
        pk, pred = m['flic_peaks_' + key], m['flic_pred_' + key]
        assert pk.shape == (8, 9, 3, 3) and pk.dtype == np.float32 and pred.shape == (2, 9, 8)
        assert_array_equal(np.round(pk[:, :, 0, :2] / 8).astype(pred.dtype).transpose(2, 1, 0), pred)
        assert (pk[:, :, 0, 2] > 0).all()
        filler = pk[..., 2] == 0
        assert (pk[filler][:, :2] == -1).all()
    out = _run_ok(args + ['--predictions', without], str(tmp_path))
    q = scipy.io.loadmat(without)
    assert 'flic_peaks_pd' not in q and 'flic_peaks_sm' not in q
    assert 'peaks' not in json.loads(out.strip().splitlines()[-1])
    for key in ('flic_pred_pd', 'flic_pred_sm'):
        assert_array_equal(q[key], m[key])
