"""The pose renderer without a GPU: the restatement (tests/render_ref.py) against closed forms a reader can check by hand,
predict.skeleton_primitives on hand-built results, and the command line's three refusals."""
import argparse

import numpy as np
import pytest
from numpy.testing import assert_array_equal

import render_ref as R
import joint_cnn_mrf_amd  # noqa: F401
from joint_cnn_mrf_amd import main as M
from joint_cnn_mrf_amd import predict as P

WHITE = 0xFFFFFF


def black(h=9, w=9):
    return np.zeros((h, w, 3), np.uint8)


def test_disc_closed_form():
    """Centre (64, 64) = pixel (4, 4), r = 8: of that pixel's samples (+-2, +-2) -> 8, (+-2, +-6) -> 40 lie within 64, (+-6, +-6) -> 72 do not: 12 of 16;
    the nearest sample of a neighbour is 10 away.  (255 * 12 * 255 + 2040) // 4080 = 191."""
    assert R.coverage(9, 9, 64, 64, 64, 64, 8)[4, 4] == 12
    out = R.draw(black(), [(64, 64, 64, 64, 8, WHITE, 255)])
    want = black()
    want[4, 4] = 191
    assert_array_equal(out, want)


def test_limb_closed_form():
    out = R.draw(black(), [(64, 32, 64, 96, 16, WHITE, 255)])
    assert_array_equal(out[4, 2:7], np.full((5, 3), 255))
    assert_array_equal(out[3, 2:7], np.full((5, 3), 128))      # samples at 50 and 54 of 42, 46, 50, 54 are within 16 of row 64: 8 of 16
    assert_array_equal(out[5, 2:7], np.full((5, 3), 128))
    assert not out[2].any() and not out[6].any() and not out[:2].any() and not out[7:].any()


def test_alpha_zero_and_r_zero():
    rs = np.random.RandomState(1)
    img = rs.randint(0, 256, (9, 9, 3)).astype(np.uint8)
    assert_array_equal(R.draw(img, [(64, 32, 64, 96, 16, WHITE, 0)]), img)
    assert_array_equal(R.draw(img, [(64, 32, 64, 96, 0, WHITE, 255)]), img)      # no sample lies ON the centre line: offsets are even, never 0


def test_painters_order():
    first, second = (64, 64, 64, 64, 64, 0xFF0000, 255), (64, 64, 64, 64, 64, 0x0000FF, 255)
    assert tuple(R.draw(black(), [first, second])[4, 4]) == (0, 0, 255)
    assert tuple(R.draw(black(), [second, first])[4, 4]) == (255, 0, 0)


def test_mirror_law():
    rs = np.random.RandomState(2)
    h, w = 11, 14
    img = rs.randint(0, 256, (h, w, 3)).astype(np.uint8)
    prims = []
    for _ in range(12):
        ay, by = rs.randint(-40, 16 * h + 40, 2)
        ax, bx = rs.randint(-40, 16 * w + 40, 2)
        prims.append((ay, ax, by, bx, rs.randint(0, 60), rs.randint(0, 1 << 24), rs.randint(0, 256)))
    mirrored = [(ay, 16 * (w - 1) - ax, by, 16 * (w - 1) - bx, r, rgb, al) for ay, ax, by, bx, r, rgb, al in prims]
    assert_array_equal(R.draw(np.ascontiguousarray(img[:, ::-1]), mirrored), R.draw(img, prims)[:, ::-1])


def test_tint_one_hot():
    """A 3 x 4 map, stride 8, onto a 24 x 32 image with the identity fit: pixel (y, x) reads the map at (y / 8, x / 8).  The one-hot cell (1, 2) is
    pixel (8, 16); (8, 12) lies half way to cell (1, 1): floor(127.5 + 0.5) = 128; (10, 16) a quarter towards cell (2, 2): floor(191.25 + 0.5) = 191."""
    hm = np.zeros((3, 4, 2), np.float32)
    hm[1, 2, 0] = 0.37
    geom, mask = (0, 0, 24, 32), (1, 6)      # joint 0 tints R; joint 1 (an all-zero map) would tint G and B
    out = R.tint(black(24, 32), hm, geom, mask, 255, 8)
    assert tuple(out[8, 16]) == (255, 0, 0) and tuple(out[8, 12]) == (128, 0, 0) and tuple(out[10, 16]) == (191, 0, 0)
    assert not out[:, :, 1:].any() and not out[16:].any() and not out[:, 24:].any() and not out[0].any()
    half = R.tint(black(24, 32), hm, geom, mask, 128, 8)
    assert half[8, 16, 0] == 128 and half[8, 12, 0] == (128 * 128 + 127) // 255 == 64 and half[10, 16, 0] == (191 * 128 + 127) // 255 == 96
    assert_array_equal(R.tint(black(24, 32), hm, geom, mask, 0, 8), black(24, 32))
    bright = np.full((24, 32, 3), 200, np.uint8)
    assert tuple(R.tint(bright, hm, geom, mask, 255, 8)[8, 16]) == (255, 200, 200)      # saturating


# ------------------------------------------------------------------ predict.skeleton_primitives
def person(offset=0.0, inside=None):
    pts = np.array([(10, 40), (30, 45), (50, 50), (10, 20), (30, 15), (50, 10), (60, 38), (60, 22), (2, 30)], np.float64) + offset
    return pts, np.ones(9, bool) if inside is None else np.asarray(inside, bool)


def result(size=(480, 720), **kw):
    sm, inside = person()
    r = {'size': size, 'sm': sm, 'sm_inside': inside, 'pd': sm + 1.0, 'pd_inside': inside.copy()}
    r.update(kw)
    return r


def test_tables():
    assert len(P.SKELETON) == 9 and P.SKELETON[-1] == (P.NECK, 8)
    assert [P.JOINT_NAMES[j] for j in (0, 1, 2, 6, 8)] == ['lsho', 'lelb', 'lwri', 'lhip', 'nose']
    assert P.JOINT_RGB[8] == 0xFF0000 and P.JOINT_RGB[0] == P.JOINT_RGB[3] == 0x00FF00 and P.JOINT_RGB[1] == 0x0000FF
    assert P.JOINT_RGB[2] == 0xFFFF00 and P.JOINT_RGB[6] == P.JOINT_RGB[7] == 0xFF00FF
    assert P.HEAT_MASK == (2, 4, 3, 2, 4, 3, 5, 5, 1)


def test_skeleton_primitives_one_person():
    pr = P.skeleton_primitives([result()])
    assert pr.dtype == np.int32 and pr.shape == (18, 8) and (pr[:, 0] == 0).all()
    limbs, discs = pr[:9], pr[9:]
    assert (limbs[:, 5] == 32).all() and (discs[:, 5] == 64).all()      # 2 * 1200 // 75 = 32 sixteenths = 2 px
    assert (limbs[:, 7] == 192).all() and (discs[:, 7] == 255).all()
    assert limbs[:, 6].tolist() == [P.JOINT_RGB[b] for _, b in P.SKELETON] and discs[:, 6].tolist() == list(P.JOINT_RGB)
    assert limbs[0, 1:5].tolist() == [160, 640, 480, 720]               # lsho (10, 40) - lelb (30, 45)
    assert limbs[8, 1:5].tolist() == [160, 480, 32, 480]                # neck = ((160 + 160) // 2, (640 + 320) // 2) - nose (2, 30)
    assert (discs[:, 1:3] == discs[:, 3:5]).all() and discs[2, 1:3].tolist() == [800, 800]
    assert P.skeleton_primitives([result()], which='pd')[0, 1:5].tolist() == [176, 656, 496, 736]
    big = P.skeleton_primitives([result(size=(1080, 1920))])
    assert (big[:9, 5] == 80).all() and (big[9:, 5] == 160).all()
    small = P.skeleton_primitives([result(size=(40, 60))])
    assert (small[:9, 5] == 16).all()
    half = P.skeleton_primitives([result(sm=person(0.26)[0])])             # floor(16 * 10.26 + 0.5) = 164; the neck halves 164 + 164 and 644 + 324
    assert half[0, 1:3].tolist() == [164, 644] and half[8, 1:3].tolist() == [164, 484]
    with pytest.raises(ValueError):
        P.skeleton_primitives([result()], which='pose')


def test_skeleton_primitives_skips_what_is_not_inside():
    inside = np.ones(9, bool)
    inside[[1, 3]] = False                                                   # lelb: two limbs go; rsho: three more and the neck
    pr = P.skeleton_primitives([result(sm_inside=inside), result()])
    first, second = pr[pr[:, 0] == 0], pr[pr[:, 0] == 1]
    assert second.shape[0] == 18 and first.shape[0] == 3 + 7
    assert first[:3, 6].tolist() == [P.JOINT_RGB[5], P.JOINT_RGB[6], P.JOINT_RGB[7]]      # relb - rwri, lsho - lhip, lhip - rhip
    assert first[3:, 6].tolist() == [P.JOINT_RGB[j] for j in (0, 2, 4, 5, 6, 7, 8)]
    assert (np.diff(pr[:, 0]) >= 0).all()


def test_skeleton_primitives_people_and_zoom():
    a, b = person(), person(100.0)
    people = {'count': 2, 'sm': np.stack([a[0], b[0], np.full((9, 2), -1.0)]), 'sm_inside': np.stack([a[1], b[1], np.zeros(9, bool)])}
    r = result(people=people)
    pr = P.skeleton_primitives([r])
    assert pr.shape[0] == 36 and pr[18, 1:5].tolist() == [1760, 2240, 2080, 2320]
    assert P.skeleton_primitives([r], which='pd').shape[0] == 18            # the part detector has one set of joints per image
    z, zi = person(3.0)
    zoom = [{'zoomed': True, 'sm': z, 'sm_inside': zi, 'pd': z + 2.0, 'pd_inside': zi},
            {'zoomed': False, 'sm': b[0], 'sm_inside': b[1], 'pd': r['pd'], 'pd_inside': r['pd_inside']}]
    r = result(people=people, zoom=zoom)
    pr = P.skeleton_primitives([r])
    assert pr.shape[0] == 36 and pr[0, 1:5].tolist() == [208, 688, 528, 768] and pr[18, 1:5].tolist() == [1760, 2240, 2080, 2320]
    assert_array_equal(P.skeleton_primitives([r], zoom=False), P.skeleton_primitives([result(people=people)]))
    assert P.skeleton_primitives([r], which='pd')[0, 1:5].tolist() == [240, 720, 560, 800]
    assert P.skeleton_primitives([result(people=dict(people, count=0))]).shape == (0, 8)


def test_render_images_refuses_heat_without_maps():
    with pytest.raises(ValueError, match='heat'):
        P.render_images(None, [black()], [result()], heat='torso')
    with pytest.raises(ValueError):
        P.render_images(None, [black()], [])


def test_cli_refusals(tmp_path):
    args = M.build_parser().parse_args([])
    assert args.render is None and args.render_heat is None and M.hps.render is None and M.hps.render_heat is None
    assert [m for _, m in M.FLAG_RULES[-3:]] == [M.RENDER_NEEDS_PREDICT, M.RENDER_HEAT_NEEDS_RENDER, M.RENDER_HEAT_SM_NEEDS_USE_SM]
    keep = argparse.Namespace(**vars(M.hps))
    predict = ['--predict', str(tmp_path / 'a.npy'), '--predictions', str(tmp_path / 'o.json')]
    try:
        for argv, message, word in ((['--render', str(tmp_path / 'r')], M.RENDER_NEEDS_PREDICT, '--predict'),
                                    (['--render_heat', 'pd'] + predict, M.RENDER_HEAT_NEEDS_RENDER, '--render'),
                                    (['--render', str(tmp_path / 'r'), '--render_heat', 'sm'] + predict, M.RENDER_HEAT_SM_NEEDS_USE_SM, '--use_sm')):
            with pytest.raises(SystemExit) as ei:
                M.main(['--synthetic', '--debug', '--gpus', '0'] + argv)
            assert str(ei.value) == message and word in message, argv
    finally:
        M.hps = keep
    assert not (tmp_path / 'o.json').exists() and not (tmp_path / 'r').exists()
