"""Pose decoding without a GPU: the numpy restatements of tests/pose_ref.py on hand-computed answers -- the search on toy tables, the tie
rule, short and empty candidate lists; the prior index against oracle.conv_mrf_pre; the planted two-person scene; the seed of the GPU
end-to-end test -- then evaluation.pose_to_pixels on a literal and the --decode_pose flag with its refusals."""
import numpy as np
import pytest

import peaks_ref
import pose_ref as R
import joint_cnn_mrf_amd  # noqa: F401
from joint_cnn_mrf_amd import evaluation, synth
from joint_cnn_mrf_amd.evaluation import pose_to_pixels  # noqa: F401  (the feature under test: without it nothing here is meaningful)
from joint_cnn_mrf_amd import main as M
from oracle import jcm_oracle as O


def _toy(k, P, dtype=np.float32):
    return np.zeros((k, P), dtype), np.zeros((k * (k - 1) // 2, P, P), dtype)


def test_pairs_are_lexicographic():
    assert R.pairs(4) == [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)]
    assert len(R.pairs()) == 36 and R.pairs()[8] == (1, 2) and R.pairs()[35] == (7, 8)


def test_search_on_toy_tables():
    """Three joints, two candidates.  Alone, every joint prefers candidate 0 (V = 1 against 0, score0 = 3); the pair term of joints 0 and 2
    pays 5 for (1, 1): the best pose is (1, 0, 1) with 0 + 1 + 0 + 5 = 6, the runner-up (1, 1, 1) with 5."""
    V, Mt = _toy(3, 2)
    V[:, 0] = 1
    Mt[1, 1, 1] = 5                                    # pair (0, 2)
    idx, score, score0, margin = R.search_one(V, Mt, [2, 2, 2])
    assert idx.tolist() == [1, 0, 1] and idx.dtype == np.int32 and score == 6 and score0 == 3 and margin == 1
    assert score.dtype == np.float32
    S = R.all_scores(V, Mt)
    assert S.shape == (2, 2, 2) and S[0, 0, 0] == 3 and S[1, 1, 1] == 5 and S[0, 1, 0] == 2
    r = R.search32(V[None], Mt[None], np.array([[2, 2, 2]]), cells=np.arange(12).reshape(1, 3, 2, 2))
    assert r['index'].tolist() == [[1, 0, 1]] and r['coords'].tolist() == [[[2, 4, 10], [3, 5, 11]]] and r['score'].dtype == np.float32


def test_search_sums_in_the_fixed_order():
    """fp32: (((V1 + M01) + ..): 1e8 + 1 is 1e8, so the order decides.  inc_1 = V[1] + M[0,1] = -1e8 + 1e8 = 0, S_1 = V[0] + 0 = 1; any
    other order of the three numbers loses the 1."""
    V, Mt = _toy(2, 1)
    V[0, 0], V[1, 0], Mt[0, 0, 0] = 1, -1e8, 1e8
    assert R.search_one(V, Mt, [1, 1])[1] == 1
    assert np.float32(1) + np.float32(-1e8) + np.float32(1e8) == 0      # what left-to-right over (V0, V1, M) would give


def test_a_tie_goes_to_the_lexicographically_smallest_pose():
    V, Mt = _toy(3, 3)
    idx, score, score0, margin = R.search_one(V, Mt, [3, 3, 3])           # all 27 poses tie
    assert idx.tolist() == [0, 0, 0] and score == 0 and score0 == 0 and margin == 0
    V[0, 2] = V[1, 1] = V[2, 0] = 1                                       # (2,1,0) is the only best pose
    assert R.search_one(V, Mt, [3, 3, 3])[0].tolist() == [2, 1, 0]
    V[0, 1] = 1                                                           # (1,1,0) ties with it: p_0 is the most significant
    assert R.search_one(V, Mt, [3, 3, 3])[0].tolist() == [1, 1, 0]
    V[1, 0] = 1                                                           # ... and (1,0,0) before (1,1,0)
    idx, score, _, margin = R.search_one(V, Mt, [3, 3, 3])
    assert idx.tolist() == [1, 0, 0] and score == 3 and margin == 0


def test_a_count_below_p_hides_the_slots_behind_it():
    V, Mt = _toy(3, 3)
    V[0] = [0, 1, 9]
    V[1] = [0, 0, 9]
    Mt[0, 1, 2] = 50                                                      # pair (0, 1), candidates (1, 2): hidden with count[1] = 2
    idx, score, score0, margin = R.search_one(V, Mt, [2, 2, 1])
    assert idx.tolist() == [1, 0, 0] and score == 1 and score0 == 0 and margin == 0      # (1,1,0) scores 1 too
    assert R.search_one(V, Mt, [3, 3, 1])[0].tolist() == [1, 2, 0]
    assert R.search_one(V, Mt, [1, 1, 1])[3] == np.inf                    # one pose: no runner-up


def test_a_count_of_zero_leaves_no_pose():
    V, Mt = _toy(3, 2)
    idx, score, score0, margin = R.search_one(V, Mt, [2, 0, 2])
    assert idx.tolist() == [-1, -1, -1] and score == -np.inf and score0 == -np.inf and np.isnan(margin)
    r = R.search32(np.stack([V, V]), np.stack([Mt, Mt]), np.array([[2, 0, 2], [2, 1, 2]]), cells=np.ones((2, 3, 2, 2), np.int32))
    assert r['index'].tolist() == [[-1, -1, -1], [0, 0, 0]] and (r['coords'][0] == -1).all() and (r['coords'][1] == 1).all()


def _spot_params(spot=(59 + 3, 89 - 5)):
    """Raw parameters whose softplus'd prior is ~1 at `spot` and ~0 elsewhere, for every pair; biases far below; identity bn."""
    e = np.full((120, 180), -10.0)
    e[spot] = 1.0
    p = synth.make_sm_params({key: e for key in synth.pair_keys()}, 'init')
    for key in synth.pair_keys():
        p['bias_' + key] = np.full((1, 60, 90, 1), -10.0, np.float32)
    return p


def test_the_prior_index():
    """The pair term is large exactly where cell_j - cell_c = (3, -5), and the prior value it reads is what conv_mrf_pre gives for a one-hot
    likelihood at cell_c, read at cell_j."""
    p = _spot_params()
    hm10 = np.full((1, 60, 90, 10), 0.5, np.float32)
    hm10[0, 30, 40, 9] = 1.0                                              # torso cell (30, 40)
    cells = np.zeros((1, 9, 2, 2), np.int32)
    cells[0, :, 0] = (20, 50)
    cells[0, :, 1] = (23, 45)                                             # candidate 1 - candidate 0 = (3, -5)
    cells[0, 8, 1] = (33, 35)                                             # nose: torso + (3, -5)
    count = np.full((1, 9), 2, np.int32)
    V, Mt = R.tables64(hm10, p, cells, count)
    bn = 1 / np.sqrt(1 + O.BN_EPS)                                        # the 'identity' BatchNorm still divides by sqrt(1 + eps)
    u, ut = O.softplus5(0.5 * bn), O.softplus5(1.0 * bn)
    rows = [i for i, (a, c) in enumerate(R.pairs()) if c != 8]            # the pairs without the nose, whose candidate 1 is elsewhere
    on, off = np.log(O.softplus5(1.0) * u + O.softplus5(-10.0) + 1e-6), np.log(O.softplus5(-10.0) * u + O.softplus5(-10.0) + 1e-6)
    assert on > -1 and off < -13
    # M[a,b,pa,pb] = T[a,b,pa,pb] + T[b,a,pb,pa]: T[a,b,1,0] is on the spot (a at candidate 1, b at candidate 0), T[b,a,1,0] likewise
    np.testing.assert_allclose(Mt[0, rows, 1, 0], on + off, rtol=1e-12)
    np.testing.assert_allclose(Mt[0, rows, 0, 1], off + on, rtol=1e-12)
    np.testing.assert_allclose(Mt[0, rows, 0, 0], 2 * off, rtol=1e-12)
    np.testing.assert_allclose(Mt[0, rows, 1, 1], 2 * off, rtol=1e-12)
    # V: only the nose's candidate 1 sits at torso + (3, -5)
    unary = np.log(u + 1e-6)
    t_on = np.log(O.softplus5(1.0) * ut + O.softplus5(-10.0) + 1e-6)
    t_off = np.log(O.softplus5(-10.0) * ut + O.softplus5(-10.0) + 1e-6)
    np.testing.assert_allclose(V[0, 8, 1], unary + t_on, rtol=1e-12)
    np.testing.assert_allclose(np.delete(V[0].reshape(-1), 17), unary + t_off, rtol=1e-12)
    # against the oracle's convolution
    A = O.softplus5(np.asarray(p['energy_lsho_lelb'], np.float64))
    for cell_c, cell_j in (((20, 50), (23, 45)), ((23, 45), (20, 50)), ((0, 0), (59, 89)), ((59, 89), (0, 0)), ((0, 89), (59, 0)), ((7, 11), (7, 11))):
        onehot = np.zeros((1, 60, 90, 1))
        onehot[0, cell_c[0], cell_c[1], 0] = 1.0
        pre = O.conv_mrf_pre(A, onehot)
        assert pre.shape == (1, 61, 91, 1)
        assert pre[0, cell_j[0], cell_j[1], 0] == R.prior_at(A[0, :, :, 0], cell_j, cell_c)
    assert R.prior_at(A[0, :, :, 0], (23, 45), (20, 50)) == O.softplus5(1.0)


def test_planted_scene():
    """Two people; B's wrists are louder, so the nine arg-maxes mix the two, and the decoded pose is all A.  Blob ratio 0.8 and bump width
    1.5 cells (pose_ref.SCENE_LOW / SCENE_SIGMA) give the all-A pose a float64 margin of 21.446 over the runner-up: far from a tie, so a GPU
    run that decodes another pose cannot blame rounding."""
    hm10, params, a, b = R.scene()
    pk = peaks_ref.hm_peaks(hm10[..., :9], 2)
    assert (pk['count'] == 2).all()
    wrist = np.isin(np.arange(9), R.WRISTS)
    np.testing.assert_array_equal(pk['cells'][0, :, 0], np.where(wrist[:, None], b, a))      # the peak-0 pose mixes the two
    np.testing.assert_array_equal(pk['cells'][0, :, 1], np.where(wrist[:, None], a, b))
    V, Mt = R.tables64(hm10, params, pk['cells'], pk['count'])
    r = R.search32(V, Mt, pk['count'], pk['cells'])
    np.testing.assert_array_equal(r['index'][0], wrist.astype(np.int32))
    np.testing.assert_array_equal(r['coords'][0].T, a)
    assert r['score'][0] > r['score0'][0]
    assert r['margin'][0] >= 1e-2
    assert abs(r['margin'][0] - 21.446) < 1e-3
    r32 = R.search32(V.astype(np.float32), Mt.astype(np.float32), pk['count'])
    np.testing.assert_array_equal(r32['index'], r['index'])


def test_end_to_end_seed_leaves_few_images_out():
    """The inputs of test_gpu_pose.py::test_end_to_end_against_float64: at most 10 % of the 32 images have a float64 top-two margin within
    90 x the table bound."""
    hm10, cells, count = R.end_to_end_inputs()
    assert hm10.shape == (32, 60, 90, 10) and cells.shape == (32, 9, 3, 2)
    params = synth.make_sm_params(synth.synthetic_priors(), kind='trained')
    r = R.search32(*R.tables64(hm10, params, cells, count), count)
    assert R.TABLE_BOUND <= 1e-4 and R.TABLE_BOUND == 4 * R.TABLE_MEASURED
    assert (r['margin'] <= 90 * R.TABLE_BOUND).sum() <= 3


def test_pose_to_pixels_on_a_literal():
    pose = {'index': np.array([[1, 0], [-1, -1]], np.int32), 'coords': np.array([[[3, 4], [5, 6]], [[-1, -1], [-1, -1]]], np.int32),
            'score': np.array([1.5, -np.inf], np.float32)}
    peaks = {'offsets': np.array([[[[0, 0], [0.25, -0.25]], [[0, 0.25], [0, 0]]]] * 2, np.float32)}
    px = evaluation.pose_to_pixels(pose, peaks)
    assert px.dtype == np.float32 and px.shape == (2, 2, 3)
    assert px[0].tolist() == [[26.0, 38.0, 1.5], [32.0, 50.0, 1.5]]      # (3 + 0.25) * 8, (5 - 0.25) * 8; 4 * 8, (6 + 0.25) * 8
    assert px[1].tolist() == [[-1.0, -1.0, -np.inf]] * 2
    assert evaluation.pose_to_pixels(pose, {}, stride=4)[0].tolist() == [[12.0, 20.0, 1.5], [16.0, 24.0, 1.5]]


def test_parser_knows_decode_pose_and_its_refusals(tmp_path):
    assert M.build_parser().parse_args(['--decode_pose']).decode_pose and not M.build_parser().parse_args([]).decode_pose
    mat = str(tmp_path / 'p.mat')

    def refused(argv):
        hps = M.hps
        try:
            with pytest.raises(SystemExit) as ei:
                M.main(['--synthetic', '--debug', '--decode_pose'] + argv)
        finally:
            M.hps = hps
        return ei.value.code
    ok = ['--use_sm', '--predictions', mat, '--peaks', '2']
    assert refused(ok + ['--train']) == M.DECODE_POSE_IS_EVALUATION_ONLY
    assert refused(['--predictions', mat, '--peaks', '2']) == M.DECODE_POSE_NEEDS_USE_SM
    assert refused(['--use_sm', '--peaks', '2']) == M.DECODE_POSE_NEEDS_PREDICTIONS
    assert refused(['--use_sm', '--predictions', mat]) == M.DECODE_POSE_NEEDS_PEAKS
    assert refused(['--use_sm', '--predictions', mat, '--peaks', '5']) == M.DECODE_POSE_NEEDS_PEAKS
    assert refused(ok + ['--u8_images']) == M.DECODE_POSE_NOT_WITH_U8_IMAGES
    assert refused(ok + ['--multiscale']) == M.DECODE_POSE_NOT_WITH_MULTISCALE
    for text, words in ((M.DECODE_POSE_IS_EVALUATION_ONLY, ('--train',)), (M.DECODE_POSE_NEEDS_USE_SM, ('--use_sm',)),
                        (M.DECODE_POSE_NEEDS_PREDICTIONS, ('--predictions',)), (M.DECODE_POSE_NEEDS_PEAKS, ('--peaks', '<= 4')),
                        (M.DECODE_POSE_NOT_WITH_U8_IMAGES, ('--u8_images',)), (M.DECODE_POSE_NOT_WITH_MULTISCALE, ('--multiscale',))):
        assert '--decode_pose' in text and all(w in text for w in words)
