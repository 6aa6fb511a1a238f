"""Pose decoding on the GPU: jcm_pose_decode (csrc/pose_decode.hip) against the two numpy restatements of tests/pose_ref.py (pinned by
tests/test_pose_cpu.py).  The tables are held to float64 within pose_ref.TABLE_BOUND; the search is held bit for bit to the fixed-order fp32
sum over the GPU's own tables; then the planted two-person scene, the end-to-end answer against float64 wherever the float64 margin decides
it, forward(decode=), the argument contract and the command line."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch
from numpy.testing import assert_array_equal

import pose_ref as R
from cli_util import run_cli
import joint_cnn_mrf_amd  # noqa: F401
from joint_cnn_mrf_amd import main as M
from joint_cnn_mrf_amd import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = ('index', 'coords', 'score', 'score0')
CORNERS = [(0, 0), (59, 89), (0, 89), (59, 0)]


def _pd_params():
    return synth.make_pd_params(debug=True, bn='trained', conv6_gain=8.0)


@pytest.fixture(scope='module')
def engines():
    """fp32 handles at --debug width, one per kind of spatial-model parameters, the planted scene's among them -> {kind: (engine, sm params)}."""
    from joint_cnn_mrf_amd.engine import Engine
    sm = {kind: synth.make_sm_params(synth.synthetic_priors(), kind=kind) for kind in ('init', 'trained')}
    sm['scene'] = R.scene()[1]
    made = {}
    for kind, p in sm.items():
        made[kind] = (Engine(device=0).load_params(dict(_pd_params(), **p)), p)
    yield made
    for e, _ in made.values():
        e.close()


def _dev(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), device='cuda:0', dtype=dtype)


def _host(r):
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in r.items()}


def _peaks(cells, count):
    return {'cells': _dev(cells, torch.int32), 'count': _dev(count, torch.int32)}


def corner_cells(B, P):
    """Candidates at the four map corners, dealt so that opposite corners meet in every pair of joints: the prior index reaches [0,0],
    [118,178], [0,178] and [118,0]."""
    cells = np.array([[[CORNERS[(j + p + b) % 4] for p in range(P)] for j in range(9)] for b in range(B)], np.int32)
    d = cells[:, :, None, :, None, :] - cells[:, None, :, None, :, :]      # [B,j,c,pj,pc,2]
    reached = {(59 + int(y), 89 + int(x)) for y, x in d.reshape(-1, 2)}
    assert reached >= {(0, 0), (118, 178), (0, 178), (118, 0)}
    return cells, np.full((B, 9), P, np.int32)


def _table_inputs(eng, P):
    """-> [(name, hm10, cells, count)]: noise maps with the peaks of hm_peaks, and with candidates at the corners."""
    hm10 = R.noise_hm10(3, 500 + P)
    pk = _host(eng.hm_peaks(_dev(hm10[..., :9]), max_peaks=P))
    assert (pk['count'] == P).all()
    return [('peaks', hm10, pk['cells'], pk['count']), ('corners', hm10) + corner_cells(3, P)]


@pytest.mark.parametrize('kind', ['init', 'trained'])
@pytest.mark.parametrize('P', [1, 2, 4])
def test_tables(engines, kind, P):
    """V and M against tables64.  Measured on the MI355X over the twelve inputs of this test (2 kinds x 3 P x peaks / corners): the largest
    |GPU - float64| is 6.638e-07 (M, 'init', P = 4, corners; V: 4.647e-07), recorded as pose_ref.TABLE_MEASURED = 6.64e-7; the bound is
    4 x that, pose_ref.TABLE_BOUND = 2.656e-6, and must stay within the project's heat-map tolerance of 1e-4."""
    eng, params = engines[kind]
    assert R.TABLE_BOUND <= 1e-4
    for name, hm10, cells, count in _table_inputs(eng, P):
        got = _host(eng.pose_decode(_dev(hm10), _peaks(cells, count), want_tables=True))
        V, Mt = R.tables64(hm10, params, cells, count)
        assert got['V'].shape == (3, 9, P) and got['M'].shape == (3, 36, P, P) and got['V'].dtype == np.float32
        dv, dm = float(np.abs(got['V'] - V).max()), float(np.abs(got['M'] - Mt).max())
        print('tables %s P=%d %s: max |dV| %.3e, max |dM| %.3e (|V| <= %.2f, |M| <= %.2f)' % (kind, P, name, dv, dm, np.abs(V).max(), np.abs(Mt).max()))
        assert max(dv, dm) <= R.TABLE_BOUND, (kind, P, name, dv, dm)


def _check_search(eng, hm10, cells, count):
    """The four outputs bit for bit against search32 on the GPU's own tables; the coordinates are the chosen cells."""
    got = _host(eng.pose_decode(_dev(hm10), _peaks(cells, count), want_tables=True))
    want = R.search32(got['V'], got['M'], count, cells)
    for k in OUT:
        assert got[k].dtype == want[k].dtype, k
        assert_array_equal(got[k].view(np.int32), want[k].view(np.int32), err_msg=k)
    plain = _host(eng.pose_decode(_dev(hm10), _peaks(cells, count)))      # without the tables: the same answer through the workspace
    assert sorted(plain) == sorted(OUT)
    for k in OUT:
        assert_array_equal(plain[k].view(np.int32), got[k].view(np.int32), err_msg=k)
    return got, want


@pytest.mark.parametrize('B', [1, 3])
@pytest.mark.parametrize('P', [2, 3, 4])
def test_search_on_noise(engines, B, P):
    eng, _ = engines['trained']
    hm10 = R.noise_hm10(B, 40 + P)
    cells, count = R.random_cells(B, P, 50 + B)
    got, _ = _check_search(eng, hm10, cells, count)
    assert (got['score'] >= got['score0']).all() and (got['index'] >= 0).all()


def _four_level(B, seed):
    """Maps of four levels under constant priors and biases: every table entry takes one of a few values, so scores tie exactly in droves."""
    rs = np.random.RandomState(seed)
    return rs.choice(np.array([0.0, 0.25, 0.5, 1.0], np.float32), (B, 60, 90, 10)).astype(np.float32)


def test_search_ties_go_to_the_smallest_pose():
    from joint_cnn_mrf_amd.engine import Engine
    flat = {key: np.full((120, 180), 0.5) for key in synth.pair_keys()}
    eng = Engine(device=0).load_params(dict(_pd_params(), **synth.make_sm_params(flat, 'init')))
    try:
        hm10 = _four_level(3, 7)
        cells, count = R.random_cells(3, 4, 8)
        got, want = _check_search(eng, hm10, cells, count)
        for b in range(3):      # the ties are there: several poses reach the best score
            S = R.all_scores(got['V'][b], got['M'][b])
            assert int((S == got['score'][b]).sum()) > 1
        same = np.zeros_like(hm10)      # one level everywhere: every pose ties, the answer is pose 0
        got, _ = _check_search(eng, same, cells, count)
        assert (got['index'] == 0).all() and (got['score'] == got['score0']).all()
    finally:
        eng.close()


def test_search_with_mixed_counts(engines):
    """Counts between 0 and P: slots at or beyond count are skipped (they hold cells -1 as hm_peaks leaves them); a 0 leaves the image without a pose."""
    eng, _ = engines['trained']
    B, P = 3, 4
    hm10 = R.noise_hm10(B, 61)
    cells, _ = R.random_cells(B, P, 62)
    count = np.array([[4, 1, 3, 2, 4, 1, 2, 3, 4], [2, 2, 0, 4, 4, 4, 1, 1, 3], [1, 4, 4, 4, 2, 3, 4, 4, 1]], np.int32)
    cells[np.arange(P)[None, None, :] >= count[:, :, None]] = -1
    got, _ = _check_search(eng, hm10, cells, count)
    assert (got['index'] < count).all()
    assert (got['index'][1] == -1).all() and (got['coords'][1] == -1).all() and got['score'][1] == -np.inf and got['score0'][1] == -np.inf
    assert (got['index'][[0, 2]] >= 0).all()
    dead = np.arange(P)[None, None, :] >= count[:, :, None]
    assert (got['V'][dead] == 0).all()


def test_search_with_one_candidate(engines):
    eng, _ = engines['init']
    hm10 = R.noise_hm10(3, 71)
    cells, count = R.random_cells(3, 1, 72)
    got, _ = _check_search(eng, hm10, cells, count)
    assert (got['index'] == 0).all()
    assert_array_equal(got['score'].view(np.int32), got['score0'].view(np.int32))
    assert_array_equal(got['coords'], cells[:, :, 0].transpose(0, 2, 1))


def test_search_across_work_groups(engines):
    """33 images: the partial winners of one image lie in 16 work groups, those of the batch in 528."""
    eng, _ = engines['trained']
    hm10 = R.noise_hm10(33, 81)
    cells, count = R.random_cells(33, 4, 82)
    got, _ = _check_search(eng, hm10, cells, count)
    assert len({tuple(i) for i in got['index']}) > 16      # the answers differ from image to image


def test_planted_scene(engines):
    """Two people, B's wrists louder: the peak-0 pose mixes them, the decoded pose is all A."""
    eng, _ = engines['scene']
    hm10, _, a, b = R.scene()
    pk = eng.hm_peaks(_dev(hm10[..., :9]), max_peaks=2)
    got = _host(eng.pose_decode(_dev(hm10), pk))
    cells = pk['cells'].cpu().numpy()
    mixed = np.where(np.isin(np.arange(9), R.WRISTS)[:, None], b, a)
    assert_array_equal(cells[0, :, 0], mixed)
    assert_array_equal(got['coords'][0].T, a)
    assert_array_equal(got['index'][0], np.isin(np.arange(9), R.WRISTS).astype(np.int32))
    assert got['score'][0] > got['score0'][0]


def test_end_to_end_against_float64(engines):
    """32 random images, P = 3 (the inputs of test_pose_cpu.py::test_end_to_end_seed_leaves_few_images_out): wherever the float64 top-two
    margin exceeds 90 x the table bound -- 90 terms per score -- the GPU's pose is the float64 pose; at most 10 % of the images fall under that rule."""
    eng, params = engines['trained']
    hm10, cells, count = R.end_to_end_inputs()
    got = _host(eng.pose_decode(_dev(hm10), _peaks(cells, count)))
    want = R.search32(*R.tables64(hm10, params, cells, count), count, cells)
    decided = want['margin'] > 90 * R.TABLE_BOUND
    print('end to end: %d of %d images decided, smallest margin %.3e' % (decided.sum(), len(decided), want['margin'].min()))
    assert (~decided).sum() <= 0.1 * len(decided)
    assert_array_equal(got['index'][decided], want['index'][decided])
    assert_array_equal(got['coords'][decided], want['coords'][decided])
    assert np.abs(got['score'][decided] - want['score'][decided]).max() <= 90 * R.TABLE_BOUND


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and bool((a.view(torch.int32) == b.view(torch.int32)).all())


@pytest.mark.parametrize('entry', ['forward', 'eval_forward', 'towers'])
def test_forward_with_decode(engines, entry):
    from joint_cnn_mrf_amd.dist import Towers
    e, sm = engines['trained']
    X, Y = synth.make_images(2, seed=41), synth.make_targets(2, seed=42)
    x, y = _dev(X), _dev(Y)
    torso = y[:, :, :, 9:].contiguous()
    tw = Towers(dict(_pd_params(), **sm), [0, 0]) if entry == 'towers' else None

    def call(**kw):
        if entry == 'forward':
            r = e.forward(x, torso, use_sm=True, **kw)
        elif entry == 'eval_forward':
            r = e.eval_forward(x, y, use_sm=True, **kw)
        else:
            r = tw.forward(X, Y[:, :, :, 9:], use_sm=True, want_prob=True, **kw)
        torch.cuda.synchronize()
        return r
    try:
        plain = call(peaks=3)
        r = call(peaks=3, decode=True)
        assert sorted(r) == sorted(list(plain) + ['pose'])
        for k in plain:
            if isinstance(plain[k], dict):
                assert all(_same_bits(plain[k][f], r[k][f]) for f in plain[k]), k
            else:
                assert _same_bits(plain[k], r[k]), k
        want = e.pose_decode(torch.cat([r['pd_prob'], torso], dim=3), r['pd_peaks'])
        torch.cuda.synchronize()
        assert sorted(r['pose']) == sorted(OUT)
        for k in OUT:
            assert _same_bits(r['pose'][k], want[k]), k
        assert r['pose']['index'].shape == (2, 9) and bool((r['pose']['index'] >= 0).all())
        if entry != 'towers':
            quiet = call(peaks=3, decode=True, want_prob=False)      # the probabilities in a scratch tensor: the same pose
            assert 'pd_prob' not in quiet and all(_same_bits(quiet['pose'][k], want[k]) for k in OUT)
            for kw in (dict(peaks=0), dict(peaks=5), dict(peaks=3, use_sm=False)):
                with pytest.raises(ValueError, match='decode=True needs use_sm=True and 1 <= peaks <= 4'):
                    e.forward(x, torso, decode=True, **kw) if entry == 'forward' else e.eval_forward(x, y, decode=True, **kw)
    finally:
        if tw is not None:
            tw.close()


def test_argument_contract(engines):
    from joint_cnn_mrf_amd.engine import Engine
    eng, _ = engines['init']
    p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)
    hm10 = _dev(R.noise_hm10(1, 91))
    mark_i, mark_f = -77, -77.0

    def call(handle, P, lib=eng._lib):
        n = max(P, 1)
        cells, count = R.random_cells(1, n, 92)
        outs = [torch.full((1, 9), mark_i, dtype=torch.int32, device='cuda:0'), torch.full((1, 2, 9), mark_i, dtype=torch.int32, device='cuda:0'),
                torch.full((1,), mark_f, device='cuda:0'), torch.full((1,), mark_f, device='cuda:0'),
                torch.full((1, 9, n), mark_f, device='cuda:0'), torch.full((1, 36, n, n), mark_f, device='cuda:0')]
        c, k = _dev(cells, torch.int32), _dev(count, torch.int32)
        torch.cuda.synchronize()
        rc = lib.jcm_pose_decode(handle, p(hm10), 1, p(c), p(k), P, *[p(o) for o in outs])
        torch.cuda.synchronize()
        return rc, all(bool((o == (mark_i if o.dtype == torch.int32 else mark_f)).all()) for o in outs)
    assert call(eng._h, 0) == (1, True)      # JCM_ERR_ARG
    assert call(eng._h, 5) == (1, True)
    rc, untouched = call(eng._h, 4)
    assert rc == 0 and not untouched
    with pytest.raises(RuntimeError, match=r'jcm_pose_decode failed.*1 <= P <= 4'):
        eng.pose_decode(hm10, _peaks(*R.random_cells(1, 5, 93)))
    with pytest.raises(ValueError, match='pose_decode expects'):
        eng.pose_decode(hm10[..., :9].contiguous(), _peaks(*R.random_cells(1, 2, 93)))
    bare = Engine(device=0).load_params(_pd_params())      # finalised, no spatial model
    try:
        assert call(bare._h, 2) == (2, True)      # JCM_ERR_STATE
    finally:
        bare.close()
    fresh = Engine(device=0)      # not finalised
    try:
        assert call(fresh._h, 2) == (2, True)
    finally:
        fresh.close()


def test_cli_decodes_the_poses_of_its_predictions(tmp_path):
    import scipy.io
    args = ['--debug', '--synthetic', '--use_sm', '--batch_size', '4', '--synthetic_size', '8', '--gpus', '0']
    mat = str(tmp_path / 'P.mat')
    r = run_cli(args + ['--predictions', mat, '--peaks', '3', '--decode_pose'], str(tmp_path))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    m = scipy.io.loadmat(mat)
    lines = r.stdout.strip().splitlines()
    line = json.loads(lines[-1])
    assert line['peaks'] == 3 and line['n_images'] == 8 and 0.0 <= line['pose_changed'] <= 1.0
    dr = [ln for ln in lines if ln.startswith('test_dr_pose: ')]
    assert len(dr) == 1 and 0.0 <= float(dr[0].split()[1]) <= 100.0
    pose, score, pk = m['flic_pred_pose'], m['flic_pose_score'], m['flic_peaks_pd']
    assert pose.shape == m['flic_pred_pd'].shape == (2, 9, 8) and pose.dtype == m['flic_pred_pd'].dtype
    assert score.shape == (8, 2) and score.dtype == np.float32 and (score[:, 0] >= score[:, 1]).all()
    # every decoded cell is one of the image's peaks of that joint, and pose_changed counts the images that left peak 0
    cells = np.round(pk[..., :2] / 8).astype(np.int64)      # [N,K,P,2]
    hit = (cells == pose.transpose(2, 1, 0)[:, :, None, :]).all(axis=3)
    assert hit.any(axis=2).all()
    changed = (pose != m['flic_pred_pd']).any(axis=(0, 1))
    assert line['pose_changed'] == float(changed.mean())
    assert_array_equal(score[~changed, 0], score[~changed, 1])


def test_cli_refusals(tmp_path):
    mat = str(tmp_path / 'p.mat')
    base = ['--debug', '--synthetic', '--gpus', '0', '--decode_pose']
    ok = ['--use_sm', '--predictions', mat, '--peaks', '2']
    cases = [(base + ok + ['--train'], M.DECODE_POSE_IS_EVALUATION_ONLY),
             (base + ['--predictions', mat, '--peaks', '2'], M.DECODE_POSE_NEEDS_USE_SM),
             (base + ['--use_sm', '--peaks', '2'], M.DECODE_POSE_NEEDS_PREDICTIONS),
             (base + ['--use_sm', '--predictions', mat], M.DECODE_POSE_NEEDS_PEAKS),
             (base + ['--use_sm', '--predictions', mat, '--peaks', '5'], M.DECODE_POSE_NEEDS_PEAKS),
             (base + ok + ['--u8_images'], M.DECODE_POSE_NOT_WITH_U8_IMAGES),
             (base + ok + ['--multiscale'], M.DECODE_POSE_NOT_WITH_MULTISCALE)]
    for argv, text in cases:
        hps = M.hps
        try:
            with pytest.raises(SystemExit) as ei:
                M.main(argv)
        finally:
            M.hps = hps
        assert ei.value.code == text, argv
    assert not os.path.exists(mat)
