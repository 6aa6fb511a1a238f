"""The host side of the zoom pass without a GPU: the restatement of the window fit (tests/fit_windows_ref.py) against
tests/fit_ref.py, evaluation.window_to_source against the forward pixel-centre mapping, predict.zoom_windows' arithmetic and skip rules,
ZOOM_TORSO_PIXELS against the annotations it is a statistic of, and the command line's refusals."""
import argparse
import os

import numpy as np
import pytest
from numpy.testing import assert_array_equal

import fit_ref as F
import fit_windows_ref as W
import joint_cnn_mrf_amd  # noqa: F401
from joint_cnn_mrf_amd import evaluation as EV
from joint_cnn_mrf_amd import main as M
from joint_cnn_mrf_amd import predict as P

HERE = os.path.dirname(os.path.abspath(__file__))


def test_whole_image_window_is_the_fit():
    rs = np.random.RandomState(3)
    img = rs.randint(0, 256, (37, 53, 3)).astype(np.uint8)
    for pad in (0, 114):
        out, geom = W.fit_window(img, 0, 0, 37, 53, 24, 36, pad)
        want, wgeom = F.fit(img, 24, 36, pad)
        assert geom == wgeom == (0, 1, 24, 34)
        assert_array_equal(out, want)


def test_window_is_pad_then_crop():
    rs = np.random.RandomState(4)
    img = rs.randint(0, 256, (9, 11, 3)).astype(np.uint8)
    big = np.pad(img, ((20, 20), (20, 20), (0, 0)), constant_values=114)
    for y0, x0, h, w in ((2, 3, 4, 5), (-3, -4, 7, 8), (5, 6, 10, 10), (-2, -2, 13, 15), (-20, 0, 5, 5), (8, 10, 1, 1), (0, 11, 3, 3)):
        assert_array_equal(W.window(img, y0, x0, h, w, 114), big[20 + y0:20 + y0 + h, 20 + x0:20 + x0 + w])
    assert_array_equal(W.desc7(np.array([(1, 9, 11), (299, 5, 5)]), [(1, -1, 2, 3, 4)]), np.array([(299, 5, 5, -1, 2, 3, 4)], np.int64))


def test_fit_geometry_is_the_restatements():
    for (h, w), (OH, OW), want in F.GEOMETRY_KAT:
        assert EV.fit_geometry(h, w, OH, OW) == want == F.geometry(h, w, OH, OW)


def test_window_to_source_inverts_the_forward_mapping():
    """Two windows of one 100 x 150 image: one reaching past the top left corner (its padded part is inside the content rectangle and outside the
    image), one wide window inside (bars above and below its content).  A grid of source positions goes forward through the fit's pixel-centre
    mapping and comes back."""
    sizes = np.array([(100, 150)], np.int64)
    windows = np.array([(0, -20, -30, 80, 120), (0, 40, 10, 20, 120)], np.int64)
    geom = np.array([EV.fit_geometry(wh, ww, 48, 72) + (wh, ww) for _, _, _, wh, ww in windows], np.int32)
    assert geom.tolist() == [[0, 0, 48, 72, 80, 120], [18, 0, 12, 72, 20, 120]]
    ys, xs = np.meshgrid(np.arange(0, 100, 7.0), np.arange(0, 150, 11.0), indexing='ij')
    src = np.stack([ys, xs], -1).reshape(-1, 2)                                     # positions in the image
    pts = np.empty((2, len(src), 3))
    for n, (_, wy0, wx0, wh, ww) in enumerate(windows):
        y0, x0, ch, cw = geom[n, :4]
        pts[n, :, 0] = (src[:, 0] - wy0 + 0.5) * ch / wh - 0.5 + y0
        pts[n, :, 1] = (src[:, 1] - wx0 + 0.5) * cw / ww - 0.5 + x0
        pts[n, :, 2] = np.arange(len(src))                                          # a score column passes through
    got, inside = EV.window_to_source(pts, geom, windows, sizes)
    real = ~((pts[..., 0] < 0) & (pts[..., 1] < 0))      # a frame position negative in both entries is a filler row by fit_to_source's convention
    assert real.sum() > 400 and not real.all()
    np.testing.assert_allclose(got[..., :2][real], np.broadcast_to(src, (2,) + src.shape)[real], rtol=0, atol=1e-9)
    assert_array_equal(got[..., :2][~real], pts[..., :2][~real])
    assert_array_equal(got[..., 2], pts[..., 2])
    for n, (_, wy0, wx0, wh, ww) in enumerate(windows):
        in_window = (src[:, 0] >= wy0 - 0.5) & (src[:, 0] < wy0 + wh - 0.5) & (src[:, 1] >= wx0 - 0.5) & (src[:, 1] < wx0 + ww - 0.5)
        assert_array_equal(inside[n], in_window)                                    # every src position lies in the image
        assert in_window.any() and not in_window.all() and not inside[n][~real[n]].any()
    # the three kinds of place, on window 0 and window 1: frame pixels (row, col)
    probe = np.array([[(4.0, 5.0), (30.0, 40.0), (-1.0, -1.0)],       # window 0: its padded part (maps to (-13, -21.2)); the image; a filler row
                      [(3.0, 30.0), (20.0, 30.0), (40.0, 3.0)]])      # window 1: the bar above; the image; the bar below
    got, inside = EV.window_to_source(probe, geom, windows, sizes)
    assert inside.tolist() == [[False, True, False], [False, True, False]]
    assert got[0, 2].tolist() == [-1.0, -1.0]
    assert got[0, 0].tolist() == [(4 + 0.5) * 80 / 48 - 0.5 - 20, (5 + 0.5) * 120 / 72 - 0.5 - 30] and (got[0, 0] < -0.5).all()
    assert_array_equal(got[1, 1], EV.fit_to_source(probe[1:, 1:2], geom[1:])[0][0, 0] + (40, 10))
    # the far edges of the image: a point maps to row h - 0.5 exactly and is outside, one just before is inside
    edge = np.array([[(35.5, 10.0), (35.2, 10.0)]])      # a window over rows [40, 120) of the 100 rows: (35.5 + 0.5) * 80 / 48 - 0.5 + 40 = 99.5
    g80 = np.array([(0, 0, 48, 72, 80, 120)], np.int32)
    got, inside = EV.window_to_source(edge, g80, np.array([(0, 40, 30, 80, 120)]), np.array([(100, 150)]))
    assert got[0, 0, 0] == 99.5 and 98.9 < got[0, 1, 0] < 99.1 and inside.tolist() == [[False, True]]
    with pytest.raises(ValueError):
        EV.window_to_source(probe, geom, windows[:, :4], sizes)
    with pytest.raises(ValueError):
        EV.window_to_source(probe, geom, np.array([(0, 0, 0, 5, 5), (1, 0, 0, 5, 5)]), sizes)


def test_zoom_torso_pixels_is_the_median_of_the_annotations():
    xy = np.load(os.path.join(HERE, 'golden', 'flic_train_xy.npy'))      # [N, (x, y), 9]
    pts = xy.transpose(0, 2, 1)
    d = np.sqrt((((pts[:, 0] + pts[:, 3]) / 2 - (pts[:, 6] + pts[:, 7]) / 2) ** 2).sum(-1))
    assert abs(P.ZOOM_TORSO_PIXELS - float(np.median(d))) <= 1e-9
    assert_array_equal(P.torso_length(pts[:, :, ::-1]), d)      # (row, col) or (x, y): a distance
    assert P.ZOOM_TORSO_JOINTS == ((P.JOINT_NAMES.index('lsho'), P.JOINT_NAMES.index('rsho')), (P.JOINT_NAMES.index('lhip'), P.JOINT_NAMES.index('rhip')))


def _person(t, centre, lean=0.0):
    """Nine joints (row, col) whose shoulder midpoint lies t / 2 above `centre` and whose hip midpoint t / 2 below it (leaning by `lean` columns)."""
    cy, cx = centre
    sm = np.zeros((9, 2))
    sm[0], sm[3] = (cy - t / 2, cx - 20 - lean / 2), (cy - t / 2, cx + 20 - lean / 2)
    sm[6], sm[7] = (cy + t / 2, cx - 12 + lean / 2), (cy + t / 2, cx + 12 + lean / 2)
    return sm


@pytest.mark.parametrize('k', (0.25, 1, 3))
def test_zoom_windows_size_and_centre(k):
    """A 960 x 1440 photo (fitted by 2: geom (0, 0, 480, 720, 960, 1440)); a person whose torso is k * ZOOM_TORSO_PIXELS long at torso cell
    (22, 61).  The window is round(480 k) rows high, 3:2, centred on the cell's pixel, and its centre is cell (30, 45) of the second pass.  (At
    k = 0.25 the torso is 32.7 pixels, just above the two cells -- 32 pixels of this photo -- below which a person is skipped.)"""
    geom = np.array([(0, 0, 480, 720, 960, 1440)])
    cell = np.array([(22, 61)])
    cy, cx = (22 * 8 + 0.5) * 2 - 0.5, (61 * 8 + 0.5) * 2 - 0.5
    sm = _person(k * P.ZOOM_TORSO_PIXELS, (cy, cx))[None]
    wins, cells, skipped = P.zoom_windows(sm, np.ones((1, 9), bool), cell, geom)
    wh = int(round(480 * k))
    assert wins.dtype == np.int64 and cells.dtype == np.int32 and skipped.dtype == bool
    assert wins[0, 3] == wh and wins[0, 4] == (3 * wh + 1) // 2
    assert wins[0].tolist() == [0, int(np.floor(cy + 0.5)) - wh // 2, int(np.floor(cx + 0.5)) - wins[0, 4] // 2, wh, (3 * wh + 1) // 2]
    assert abs(int(cells[0, 0]) - 30) <= 1 and abs(int(cells[0, 1]) - 45) <= 1
    assert not skipped[0]
    assert P.torso_length(sm)[0] == pytest.approx(k * P.ZOOM_TORSO_PIXELS, abs=1e-9)
    # a leaning torso is measured between the midpoints, and `image` is passed through
    lean = _person(k * P.ZOOM_TORSO_PIXELS, (cy, cx), lean=30.0)[None]
    w2, _, _ = P.zoom_windows(lean, np.ones((1, 9), bool), cell, geom, image=[5])
    assert w2[0, 0] == 5 and w2[0, 3] == int(np.floor(np.hypot(k * P.ZOOM_TORSO_PIXELS, 30.0) * 480 / P.ZOOM_TORSO_PIXELS + 0.5))


def test_zoom_windows_centre_follows_the_letterbox():
    """A 300 x 400 image sits at columns [40, 680) of the frame: the cell's pixel goes back through that fit, and a window near the image's
    corner reaches past it (negative origin)."""
    geom = np.array([(0, 40, 480, 640, 300, 400)])
    cell = np.array([(3, 8)])
    centre = EV.fit_to_source(np.array([(24.0, 64.0)]), geom)[0][0]
    assert centre.tolist() == [(24 + 0.5) * 300 / 480 - 0.5, (64 - 40 + 0.5) * 400 / 640 - 0.5]
    sm = _person(60.0, centre)[None]
    wins, cells, skipped = P.zoom_windows(sm, np.ones((1, 9), bool), cell, geom)
    wh = int(np.floor(60.0 * 480 / P.ZOOM_TORSO_PIXELS + 0.5))
    assert wins[0].tolist() == [0, int(np.floor(centre[0] + 0.5)) - wh // 2, int(np.floor(centre[1] + 0.5)) - ((3 * wh + 1) // 2) // 2, wh, (3 * wh + 1) // 2]
    assert wins[0, 1] < 0 and wins[0, 2] < 0 and not skipped[0]
    assert abs(int(cells[0, 0]) - 30) <= 1 and abs(int(cells[0, 1]) - 45) <= 1


def test_zoom_windows_skip_rules():
    geom = np.array([(0, 0, 480, 720, 1920, 2880)] * 9)
    cell = np.array([(30, 45)] * 9)
    centre = ((30 * 8 + 0.5) * 4 - 0.5, (45 * 8 + 0.5) * 4 - 0.5)
    two_cells = 16 * 1920 / 480                                                     # 64 pixels of the image
    sm = np.stack([_person(t, centre) for t in (400.0, 400.0, 400.0, 400.0, 400.0, two_cells - 0.5, two_cells, 2974.0, 2972.0)])
    inside = np.ones((9, 9), bool)
    inside[1, 0] = inside[2, 3] = inside[3, 6] = inside[4, 7] = False               # each of the four torso joints in turn
    inside[0, (1, 2, 4, 5, 8)] = False                                              # the other joints do not matter
    wins, cells, skipped = P.zoom_windows(sm, inside, cell, geom)
    # 2974 px -> wh = 10928, ww = 16392 > 16384; 2972 px -> wh = 10921, ww = 16382
    assert wins[7, 3:].tolist() == [10928, 16392] and wins[8, 3:].tolist() == [10921, 16382]
    assert skipped.tolist() == [False, True, True, True, True, True, False, True, False]
    # a torso cell out in a bar, far from the image, with a small torso: the window shares no pixel with the image
    g = np.array([(0, 225, 480, 270, 640, 360)])                                    # a portrait image: bars left and right
    far = EV.fit_to_source(np.array([(240.0, 8.0)]), g)[0][0]
    assert far[1] < -250
    small = _person(40.0, (300.0, 100.0))[None]                                     # 40 > 16 * 640 / 480: not the quantisation rule
    wins, _, skipped = P.zoom_windows(small, np.ones((1, 9), bool), np.array([(30, 1)]), g)
    assert wins[0, 2] + wins[0, 4] <= 0 and skipped.tolist() == [True]
    with pytest.raises(ValueError):
        P.zoom_windows(sm, inside[:, :8], cell, geom)


def test_predict_images_zoom_needs_use_sm():
    with pytest.raises(ValueError, match='use_sm'):
        P.predict_images(None, [np.zeros((4, 4, 3), np.uint8)], use_sm=False, zoom=True)


def test_cli_refusals(tmp_path):
    assert M.build_parser().parse_args(['--zoom']).zoom and not M.build_parser().parse_args([]).zoom
    keep = argparse.Namespace(**vars(M.hps))
    out = ['--predictions', str(tmp_path / 'o.json')]
    try:
        for argv, message, word in ((['--predict', str(tmp_path / 'a.npy')] + out, M.ZOOM_NEEDS_USE_SM, '--use_sm'),
                                    (['--use_sm'] + out, M.ZOOM_NEEDS_PREDICT, '--predict'),
                                    (['--use_sm', '--train'], M.ZOOM_NEEDS_PREDICT, '--predict')):
            with pytest.raises(SystemExit) as ei:
                M.main(['--synthetic', '--debug', '--gpus', '0', '--zoom'] + argv)
            assert str(ei.value) == message and word in message and '--zoom' in message, argv
    finally:
        M.hps = keep
    assert not (tmp_path / 'o.json').exists()
