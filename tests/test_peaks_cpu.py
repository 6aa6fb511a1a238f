"""Heat-map peaks without a GPU: hand-computed known answers of the numpy restatement (tests/peaks_ref.py) that the GPU tests hold
jcm_hm_peaks to, evaluation.peaks_to_pixels on a literal, and the --peaks flag with its three refusals."""
import numpy as np
import pytest

import peaks_ref as R
import joint_cnn_mrf_amd  # noqa: F401
from joint_cnn_mrf_amd import evaluation
from joint_cnn_mrf_amd import main as M

INF = np.float32(np.inf)


def _one(v, P, threshold=0.0):
    """One map [HH,WW] -> (cells [P,2], offsets [P,2], scores [P], count) through the batched entry point."""
    r = R.hm_peaks(np.asarray(v, np.float32)[None, :, :, None], P, threshold)
    assert r['cells'].dtype == np.int32 and r['offsets'].dtype == np.float32 and r['scores'].dtype == np.float32 and r['count'].dtype == np.int32
    return r['cells'][0, 0].tolist(), r['offsets'][0, 0].tolist(), r['scores'][0, 0].tolist(), int(r['count'][0, 0])


def test_a_plateau_yields_its_first_pixel():
    """Three 8-connected pixels of value 5: (0,1) has no earlier neighbour of its value; (0,2) and (1,2) have one each."""
    v = [[0, 5, 5, 0],
         [0, 0, 5, 0],
         [0, 0, 0, 0]]
    cells, offsets, scores, count = _one(v, 2)
    assert count == 1
    assert cells == [[0, 1], [-1, -1]]
    assert offsets == [[0.0, 0.25], [0.0, 0.0]]               # row 0: clipped; columns: v(0,2) = 5 > v(0,0) = 0
    assert scores == [5.0, 0.0]


def test_corner_and_edge_clip_the_offset():
    v = np.zeros((4, 5), np.float32)
    v[0, 0] = 3                                               # corner: both axes clipped
    v[3, 2], v[3, 1] = 2, 1                                   # bottom edge: rows clipped, columns 1 (left) against 0 (right)
    cells, offsets, scores, count = _one(v, 3)
    assert count == 2
    assert cells == [[0, 0], [3, 2], [-1, -1]]
    assert offsets == [[0.0, 0.0], [0.0, -0.25], [0.0, 0.0]]
    assert scores == [3.0, 2.0, 0.0]


def test_equal_separated_maxima_are_ordered_by_index_and_missing_slots_are_filler():
    v = np.zeros((3, 7), np.float32)
    v[1, 5] = 4
    v[1, 1] = 4
    v[2, 3] = 1
    cells, offsets, scores, count = _one(v, 5)
    assert count == 3
    assert cells == [[1, 1], [1, 5], [2, 3], [-1, -1], [-1, -1]]     # 4 at index 8 before 4 at index 12, then the 1
    assert offsets == [[0.0, 0.0]] * 5                        # equal neighbours everywhere, and row 2 is the border
    assert scores == [4.0, 4.0, 1.0, 0.0, 0.0]
    assert _one(v, 1)[0] == [[1, 1]]                          # P below the number of maxima: the first P of the same order


def test_threshold_is_strict():
    v = np.zeros((3, 3), np.float32)
    v[1, 1] = 0.75
    assert _one(v, 2, threshold=0.5)[3] == 1
    cells, offsets, scores, count = _one(v, 2, threshold=0.75)
    assert count == 0 and cells == [[-1, -1]] * 2 and offsets == [[0.0, 0.0]] * 2 and scores == [0.0, 0.0]
    # the all-zero map under the default threshold 0: nothing either; under a negative one its first pixel (the plateau rule)
    assert _one(np.zeros((3, 3)), 2)[3] == 0
    assert _one(np.zeros((3, 3)), 2, threshold=-1.0)[:1] == ([[0, 0], [-1, -1]],)


def test_offset_signs_on_an_asymmetric_bump():
    v = np.zeros((5, 5), np.float32)
    v[2, 2] = 9
    v[1, 2], v[3, 2] = 3, 5                                   # below (row 3) is higher: +
    v[2, 1], v[2, 3] = 6, 2                                   # left (column 1) is higher: -
    cells, offsets, scores, count = _one(v, 1)
    assert count == 1 and cells == [[2, 2]] and offsets == [[0.25, -0.25]] and scores == [9.0]
    cells, offsets, scores, count = _one(v[::-1, ::-1], 1)
    assert count == 1 and cells == [[2, 2]] and offsets == [[-0.25, 0.25]]


def test_logit_map_of_minus_infinity_makes_no_nan():
    v = np.full((4, 4), -INF, np.float32)
    v[2, 1] = -3.5
    r = R.hm_peaks(v[None, :, :, None], 3, threshold=-INF)
    assert r['count'].tolist() == [[1]]
    assert r['cells'][0, 0].tolist() == [[2, 1], [-1, -1], [-1, -1]]
    assert r['scores'][0, 0].tolist() == [-3.5, 0.0, 0.0]
    assert r['offsets'][0, 0].tolist() == [[0.0, 0.0]] * 3     # -inf on both sides: equal, no difference is formed
    assert not np.isnan(r['offsets']).any() and not np.isnan(r['scores']).any()
    assert _one(v, 3, threshold=0.0)[3] == 0                  # -3.5 is not above the default threshold


def test_batched_layout():
    hm = np.zeros((2, 3, 4, 3), np.float32)
    hm[0, 1, 2, 0] = 1
    hm[1, 2, 3, 2] = 2
    r = R.hm_peaks(hm, 2)
    assert r['cells'].shape == (2, 3, 2, 2) and r['offsets'].shape == (2, 3, 2, 2) and r['scores'].shape == (2, 3, 2) and r['count'].shape == (2, 3)
    assert r['count'].tolist() == [[1, 0, 0], [0, 0, 1]]
    assert r['cells'][0, 0, 0].tolist() == [1, 2] and r['cells'][1, 2, 0].tolist() == [2, 3] and r['scores'][1, 2, 0] == 2
    cached = R.hm_peaks(hm, 2, cand=R.all_local_maxima(hm))
    assert all(np.array_equal(r[k], cached[k]) for k in r)


def test_peaks_to_pixels_on_a_literal():
    peaks = {'cells': np.array([[[[2, 3], [-1, -1]]]], np.int32), 'offsets': np.array([[[[0.25, -0.25], [0, 0]]]], np.float32),
             'scores': np.array([[[0.5, 0]]], np.float32), 'count': np.array([[1]], np.int32)}
    px = evaluation.peaks_to_pixels(peaks)
    assert px.dtype == np.float32 and px.shape == (1, 1, 2, 3)
    assert px.tolist() == [[[[18.0, 22.0, 0.5], [-1.0, -1.0, 0.0]]]]      # (2 + 0.25) * 8, (3 - 0.25) * 8; the filler is not scaled
    assert evaluation.peaks_to_pixels(peaks, stride=4)[0, 0].tolist() == [[9.0, 11.0, 0.5], [-1.0, -1.0, 0.0]]


def test_parser_knows_peaks_and_the_three_refusals(tmp_path):
    a = M.build_parser().parse_args(['--use_sm', '--peaks', '4'])
    assert a.peaks == 4 and M.build_parser().parse_args([]).peaks == 0
    mat = str(tmp_path / 'p.mat')

    def refused(argv):
        hps = M.hps
        try:
            with pytest.raises(SystemExit) as ei:
                M.main(argv)
        finally:
            M.hps = hps                                       # main() stores its arguments in the module global
        return ei.value.code
    assert refused(['--train', '--synthetic', '--debug', '--peaks', '2', '--predictions', mat]) == M.PEAKS_IS_EVALUATION_ONLY
    assert refused(['--synthetic', '--debug', '--peaks', '2']) == M.PEAKS_NEEDS_PREDICTIONS
    assert refused(['--synthetic', '--debug', '--peaks', '2', '--predictions', mat, '--u8_images']) == M.PEAKS_NOT_WITH_U8_IMAGES
    for text, words in ((M.PEAKS_IS_EVALUATION_ONLY, ('--peaks', '--train')), (M.PEAKS_NEEDS_PREDICTIONS, ('--peaks', '--predictions')),
                        (M.PEAKS_NOT_WITH_U8_IMAGES, ('--peaks', '--u8_images'))):
        assert all(w in text for w in words)
