"""The float64 restatement of the letterbox fit (tests/fit_ref.py; include/jcm.h: jcm_fit_images) pinned without a GPU: the
geometry's known answers, identity and constant images, the inverse mapping evaluation.fit_to_source, and -- where PIL is installed -- the
distance from PIL's antialiased bilinear resize."""
import sys

import numpy as np
import pytest
from numpy.testing import assert_array_equal

import fit_ref as F
import joint_cnn_mrf_amd  # noqa: F401
from joint_cnn_mrf_amd import evaluation as EV
from joint_cnn_mrf_amd import predict as PR


@pytest.mark.parametrize('case', F.GEOMETRY_KAT, ids=lambda c: '%dx%d' % c[0])
def test_geometry_known_answers(case):
    (h, w), (OH, OW), want = case
    assert F.geometry(h, w, OH, OW) == want
    y0, x0, ch, cw = want
    assert 1 <= ch <= OH and 1 <= cw <= OW and (ch == OH or cw == OW) and 0 <= y0 and y0 + ch <= OH and 0 <= x0 and x0 + cw <= OW


def test_flagship_geometry():
    assert F.geometry(1080, 1920, 480, 720) == (37, 0, 405, 720)
    assert F.geometry(480, 720, 480, 720) == (0, 0, 480, 720)
    assert F.geometry(1000, 700, 480, 720) == (0, 192, 480, 336)
    assert F.geometry(211, 317, 480, 720) == (0, 0, 479, 720)


def test_identity_on_equal_size():
    img = F.kat_images()[4]
    out, geom = F.fit(img, 12, 18, pad=114)
    assert geom == (0, 0, 12, 18)
    assert_array_equal(out, img)
    for lo, wt in F.axis_taps(12, 12):      # the outer taps get weight 0
        assert sorted(wt.tolist()) in ([0.0, 1.0], [0.0, 0.0, 1.0])


def test_constant_image_stays_constant():
    for (h, w), (OH, OW), (y0, x0, ch, cw) in F.GEOMETRY_KAT:
        out, _ = F.fit(np.full((h, w, 3), 255, np.uint8), OH, OW, pad=7)
        assert (out[y0:y0 + ch, x0:x0 + cw] == 255).all()
        bars = np.ones((OH, OW), bool)
        bars[y0:y0 + ch, x0:x0 + cw] = False
        assert (out[bars] == 7).all()


def test_weights_are_normalised_and_bounded():
    for n, m in ((576, 18), (595, 19), (7, 12), (1, 12), (1080, 405), (53, 34)):
        taps = F.axis_taps(n, m)
        assert max(len(wt) for _, wt in taps) <= 66
        for lo, wt in taps:
            assert lo >= 0 and lo + len(wt) <= n and abs(wt.sum() - 1.0) < 1e-12 and (wt >= 0).all()


def test_fit_to_source_inverts_the_pixel_centre_mapping():
    geom = np.array([(3, 0, 6, 18, 13, 40), (0, 4, 12, 9, 7, 5)], np.int32)
    for b, (y0, x0, ch, cw, h, w) in enumerate(geom.tolist()):
        corners = np.array([[(y0, x0, 0.5), (y0, x0 + cw - 1, 0.25), (y0 + ch - 1, x0, 0.125), (y0 + ch - 1, x0 + cw - 1, 1.0)]] * 2, np.float32)
        got, inside = EV.fit_to_source(corners, geom[[b, b]])
        assert inside.all() and got.shape == corners.shape
        # the centre of content pixel o is source coordinate (o + 0.5) * n / m - 0.5: the first and last content pixels
        want_r = [0.5 * h / ch - 0.5, (ch - 0.5) * h / ch - 0.5]
        want_c = [0.5 * w / cw - 0.5, (cw - 0.5) * w / cw - 0.5]
        np.testing.assert_allclose(got[0, :, 0], [want_r[0], want_r[0], want_r[1], want_r[1]], rtol=0, atol=1e-12)
        np.testing.assert_allclose(got[0, :, 1], [want_c[0], want_c[1], want_c[0], want_c[1]], rtol=0, atol=1e-12)
        assert_array_equal(got[..., 2], corners[..., 2].astype(np.float64))      # scores pass through
        # and forward again: source coordinate s maps to content (s + 0.5) * m / n - 0.5
        back_r = (got[0, :, 0] + 0.5) * ch / h - 0.5 + y0
        np.testing.assert_allclose(back_r, corners[0, :, 0], rtol=0, atol=1e-9)


def test_fit_to_source_filler_and_outside():
    geom = np.array([(3, 0, 6, 18, 13, 40)], np.int32)
    pts = np.array([[[-1, -1, 0], [0, 5, 1], [9, 5, 1], [3, 17, 1]]], np.float32)      # filler, in the top bar, in the bottom bar, inside
    got, inside = EV.fit_to_source(pts, geom)
    assert inside.tolist() == [[False, False, False, True]]
    assert got[0, 0].tolist() == [-1, -1, 0]
    with pytest.raises(ValueError):
        EV.fit_to_source(pts, geom[:, :4])


def test_identity_geometry_maps_points_to_themselves():
    geom = np.array([(0, 0, 480, 720, 480, 720)], np.int32)
    pts = np.array([[[8.0, 16.0], [472.0, 712.0]]])
    got, inside = EV.fit_to_source(pts, geom)
    assert_array_equal(got, pts)
    assert inside.all()


def test_against_pil_bilinear():
    """PIL's BILINEAR resize is the same triangle filter in fixed-point arithmetic: at most 2 grey levels apart on the seven cases (measured: 1)."""
    Image = pytest.importorskip('PIL.Image')
    worst = 0
    for img, ((h, w), (OH, OW), (y0, x0, ch, cw)) in zip(F.kat_images(), F.GEOMETRY_KAT):
        want = np.asarray(Image.fromarray(img).resize((cw, ch), Image.BILINEAR))
        got = F.fit(img, OH, OW)[0][y0:y0 + ch, x0:x0 + cw]
        d = int(np.abs(got.astype(np.int64) - want.astype(np.int64)).max())
        print('fit_ref vs PIL BILINEAR %3dx%-3d -> %2dx%-2d  max |diff| = %d' % (h, w, ch, cw, d))
        worst = max(worst, d)
        assert d <= 2, ((h, w), d)
    print('fit_ref vs PIL BILINEAR worst %d' % worst)


def test_non_npy_without_pil_names_the_file(tmp_path, monkeypatch):
    """A format other than .npy needs PIL; without it SystemExit names the file and says to pass .npy (PIL hidden from the import system here)."""
    monkeypatch.setitem(sys.modules, 'PIL', None)
    path = str(tmp_path / 'photo.png')
    with pytest.raises(SystemExit) as ei:
        PR.load_image(path)
    assert path in str(ei.value) and '.npy' in str(ei.value)
    np.save(str(tmp_path / 'f.npy'), np.zeros((4, 4, 3), np.float32))
    with pytest.raises(SystemExit):
        PR.load_image(str(tmp_path / 'f.npy'))
