"""The antialiased affine sample without a device: hand-computed answers of its numpy restatement tests/affine_aa_ref.py, the host
side of it in augmentation.py (affine_footprint, fixed_affine, AffineDraw.width, affine_joints_inside), the aliasing case that is its reason, and the
rules of the new command-line flags -- which are walked behind every earlier table, so each recorded refusal keeps its message."""
import argparse
import json
import os

import numpy as np
import pytest
import torch

import affine_aa_ref as A
import affine_ref as R
import joint_cnn_mrf_amd  # noqa: F401
from joint_cnn_mrf_amd import augmentation, main as M

HERE = os.path.dirname(os.path.abspath(__file__))
f32 = np.float32
IDENTITY_FWD = [1.0, 0.0, 0.0, 0.0, 1.0, 0.0]


def test_hand_computed_answers_of_the_restatement():
    """A 4 x 4 source v[j, i] = 4 j + i, w = 2, the output read half a pixel down and right: every number below is dyadic, so the answers are exact."""
    v = (4.0 * np.arange(4)[:, None] + np.arange(4)[None, :])[:, :, None]
    g = [1.0, 0.0, 0.5, 0.0, 1.0, 0.5] + IDENTITY_FWD
    count = np.zeros((4, 4), np.int64)
    out = A.sample_values(v, g, 2.0, 0.5, count)
    # interior, pixel (1, 1) reads (1.5, 1.5): columns 0..3 weigh .25 .75 .75 .25 (Sx = 2), row sums 8 j + 3 = 3, 11, 19, 27,
    # acc = .25 * 3 + .75 * 11 + .75 * 19 + .25 * 27 = 30, out = 30 / 4
    assert A.triangle_taps(1.5, 2.0) == [(0, 0.25), (1, 0.75), (2, 0.75), (3, 0.25)]
    assert out[1, 1, 0] == f32(7.5) and count[1, 1] == 16
    # border, pixel (0, 0) reads (0.5, 0.5): columns -1..2, column -1 and row -1 are pad = 0.5 and take part: row -1 sums to 2 * .5 = 1, row j >= 0 to
    # .25 * .5 + .75 * 4 j + .75 * (4 j + 1) + .25 * (4 j + 2) = 7 j + 1.375; acc = .25 * 1 + .75 * 1.375 + .75 * 8.375 + .25 * 15.375 = 11.40625
    assert [i for i, _ in A.triangle_taps(0.5, 2.0)] == [-1, 0, 1, 2]
    assert out[0, 0, 0] == f32(11.40625 / 4) == f32(2.8515625)
    # a tap of weight exactly 0 is skipped: position 1.0 with w = 2 has the columns 0, 1, 2, not -1 and 3
    assert A.triangle_taps(1.0, 2.0) == [(0, 0.5), (1, 1.0), (2, 0.5)]


def test_footprint_of_similarity_maps():
    ang = [0.0, 0.3, -np.pi / 9, 2.0]
    for scale, want in [(0.25, 4.0), (0.5, 2.0), (1.0, 1.0), (2.0, 1.0)]:
        p = np.array([[k % 2, 0.0, 1.0, a, scale, 0.1, -0.2] for k, a in enumerate(ang)], np.float64)
        _, g = augmentation.affine_geometry(p, 480, 720)
        assert augmentation.affine_footprint(g).tolist() == [want] * len(ang)
    _, g = augmentation.affine_geometry(np.array([[0, 0.0, 1.0, 0.2, 0.75, 0.0, 0.0]]), 16, 24)
    assert abs(augmentation.affine_footprint(g)[0] - 4.0 / 3.0) < 1e-11
    with pytest.raises(ValueError):
        augmentation.affine_footprint(np.zeros((2, 6)))


def test_draws_carry_the_width():
    d = augmentation.fixed_affine(3, 16, 24, 0.5, angle=0.1, pad=0.25)
    assert len(d) == 3 and d.width.tolist() == [2.0] * 3 and d.pad == 0.25 and np.array_equal(d.colour, np.tile(f32([0, 0, 1]), (3, 1)))
    assert np.array_equal(d.geom, np.tile(d.geom[:1], (3, 1))) and d[1:].width.tolist() == [2.0] * 2
    assert augmentation.fixed_affine(2, 16, 24, 0.5, antialias=False).width is None
    assert augmentation.fixed_affine(1, 16, 24, 1.0, flip=True).colour[0, 0] == 1
    plain = augmentation.draw_affine(np.random.RandomState(4), 5, 16, 24, pad=0.5)
    aa = augmentation.draw_affine(np.random.RandomState(4), 5, 16, 24, pad=0.5, antialias=True)
    assert plain.width is None and plain[1:3].width is None
    assert np.array_equal(aa.geom, plain.geom) and np.array_equal(aa.colour, plain.colour)      # the same draw from the generator
    assert np.array_equal(aa.width, augmentation.affine_footprint(plain.geom)) and (aa.width >= 1).all() and (aa.width <= 2).all()
    with pytest.raises(ValueError):
        augmentation.fixed_affine(1, 16, 24, 0.2)                                                 # wider than 9 x 9 taps
    for bad in ([0.5, 1.0], [1.0, np.nan], [1.0, 4.5], [1.0]):
        with pytest.raises(ValueError):
            augmentation.AffineDraw(plain.colour[:2], plain.geom[:2], width=bad)


def test_width_one_is_the_plain_restatement_bit_for_bit():
    rs = np.random.RandomState(0)
    H, W = 16, 24
    x = (rs.randint(0, 256, (2, H, W, 3)).astype(f32) / f32(255))
    cells = np.stack([rs.randint(0, H // 8 + 1, (2, 10)), rs.randint(0, W // 8 + 1, (2, 10))], axis=2)
    p = np.array([[0, 0.05, 1.1, 0.2, 1.5, 0.1, -0.1], [1, 0.0, 1.0, 0.0, 1.0, 0.0, 0.0]], np.float64)
    col, g = augmentation.affine_geometry(p, H, W)
    assert augmentation.affine_footprint(g).tolist() == [1.0, 1.0]
    xa, ya, ma = A.augment(x, cells, col, g, augmentation.affine_footprint(g), 0.5)
    xr, yr, mr = R.augment(x, cells, col, g, 0.5)
    assert np.array_equal(xa.view(np.uint32), xr.view(np.uint32)) and np.array_equal(ya, yr) and np.array_equal(ma, mr)


def checkerboard_case():
    """A 16 x 24 one-pixel checkerboard at scale 0.5, moved a quarter of an output pixel so that the output pixels read the source AT its pixels
    (every other one, in both directions): -> (img float32 [16,24,3], colour row, geom row)."""
    H, W = 16, 24
    img = np.repeat(((np.arange(H)[:, None] + np.arange(W)[None, :]) % 2).astype(f32)[:, :, None], 3, axis=2)
    col, g = augmentation.affine_geometry(np.array([[0, 0.0, 1.0, 0.0, 0.5, 0.25 / W, 0.25 / H]], np.float64), H, W)
    return img, col[0], g[0]


# at most 25 taps of positive weight (w = 2), each two rounded float64 operations of relative error 2^-53, the weights themselves carrying the rounding
# of a position of size 2^4 (2^-49): under 2^-43 in all; the issue's outside limit is 1e-6
CHECKERBOARD_BOUND = 2.0 ** -40


def test_the_checkerboard_aliases_under_the_plain_sample_and_not_under_the_antialiased_one():
    img, col, g = checkerboard_case()
    H, W = img.shape[:2]
    assert CHECKERBOARD_BOUND <= 1e-6 and augmentation.affine_footprint(g[None])[0] == 2.0
    aa = A.sample_image(img, col, g, 2.0, 0.5)
    plain = R.sample_image(img, col, g, 0.5)
    inside = A.taps_inside(g, 2.0, H, W)
    assert inside.sum() >= 40                                                                     # the middle of the picture
    worst_aa, worst_plain = np.abs(aa.astype(np.float64) - 0.5)[inside].max(), np.abs(plain.astype(np.float64) - 0.5)[inside].max()
    print('checkerboard at scale 0.5: antialiased within %.3g of 0.5 on %d pixels, plain off by %.3g' % (worst_aa, inside.sum(), worst_plain))
    assert worst_aa <= CHECKERBOARD_BOUND
    assert worst_plain >= 0.25


def test_joints_that_leave_the_frame_are_found():
    H, W = 16, 24
    cells = np.zeros((3, 10, 2), np.int64)
    cells[:, :, 0], cells[:, :, 1] = 1, 1                    # the point (11.5, 11.5), 3.75 right and 4 below the centre (11.5, 7.5) ... at scale 1
    cells[1, 4] = [0, 2]                                     # (19.5, 3.5)
    cells[2, 9] = [2, 3]                                     # the torso point on row 2 = H / 8: (27.5, 19.5), outside already
    geom = lambda s, **kw: augmentation.fixed_affine(3, H, W, s, **kw).geom
    assert augmentation.affine_joints_inside(cells, geom(1.0), H, W).tolist() == [True, True, False]
    # scale 1.5 about (11.5, 7.5): (11.5, 11.5) -> (11.5, 13.5) inside; (19.5, 3.5) -> (23.5, 1.5) inside; scale 2: (19.5, 3.5) -> (27.5, -0.5) outside
    assert augmentation.affine_joints_inside(cells, geom(1.5), H, W).tolist() == [True, True, False]
    assert augmentation.affine_joints_inside(cells, geom(2.0), H, W).tolist() == [True, False, False]
    # scale 4: (11.5, 11.5) -> (11.5, 23.5) outside
    assert augmentation.affine_joints_inside(cells, geom(4.0), H, W).tolist() == [False, False, False]
    # the edge itself is inside: [0, W] x [0, H] is closed -- (11.5, 11.5) -> (11.5, 16.0) at scale 2.125
    assert augmentation.affine_joints_inside(cells[:1], geom(2.125)[:1], H, W).tolist() == [True]
    assert augmentation.affine_joints_inside(cells[:1], geom(2.25)[:1], H, W).tolist() == [False]
    # a quarter turn about the centre maps (19.5, 3.5) to 8 beside and 4 below... both directions of rotation keep (11.5, 11.5) inside a 16 x 24 frame
    assert augmentation.affine_joints_inside(cells[:1], geom(1.0, angle=np.pi / 2)[:1], H, W).tolist() == [True]
    # ... and it agrees with where the restatement clamps
    for s in (1.0, 1.5, 2.0, 4.0):
        g = geom(s)
        for b in range(3):
            px, py = 8.0 * cells[b, :, 1] + 3.5, 8.0 * cells[b, :, 0] + 3.5
            qx, qy = (g[b, 6] * px + g[b, 7] * py) + g[b, 8], (g[b, 9] * px + g[b, 10] * py) + g[b, 11]
            free = bool(((qx >= 0) & (qx <= W) & (qy >= 0) & (qy <= H)).all())
            assert augmentation.affine_joints_inside(cells[b:b + 1], g[b:b + 1], H, W)[0] == free
    with pytest.raises(ValueError):
        augmentation.affine_joints_inside(cells[:, :9], geom(1.0), H, W)


# ------------------------------------------------------------------ the command line
def refusal(argv):
    keep = argparse.Namespace(**vars(M.hps))
    try:
        M.main(list(argv) + ['--gpus', '99'])
        return None
    except SystemExit as e:
        return e.code
    finally:
        M.hps = keep


NO_DEVICE = '--gpus [99]: device 99 does not exist (%d visible)' % torch.cuda.device_count()
SWEEP = ['--eval_scale', '0.5', '1.5', '--scale_curve', 'c.json']


def test_the_new_rules():
    assert refusal(SWEEP) == NO_DEVICE and refusal(SWEEP + ['--synthetic', '--debug', '--use_sm']) == NO_DEVICE
    assert refusal(['--eval_scale', '0.5']) == M.EVAL_SCALE_NEEDS_SCALE_CURVE
    assert refusal(['--scale_curve', 'c.json']) == M.SCALE_CURVE_NEEDS_EVAL_SCALE
    for flag in ('--multiscale', '--flip_test', '--u8_images'):
        assert refusal(SWEEP + [flag]) == M.EVAL_SCALE_SINGLE_SCALE_ONLY
    assert refusal(SWEEP + ['--infer_torso', '--use_sm']) == M.EVAL_SCALE_SINGLE_SCALE_ONLY
    assert refusal(SWEEP + ['--train']) == M.EVAL_SCALE_IS_EVALUATION_ONLY
    assert refusal(SWEEP + ['--predict', 'a.png', '--predictions', 'p.json']) == M.EVAL_SCALE_IS_EVALUATION_ONLY
    assert refusal(['--eval_scale', '0.2', '1', '--scale_curve', 'c.json']) == '--eval_scale 0.2 1: 0.25 <= S <= 4'
    assert refusal(['--eval_scale', '4.5', '--scale_curve', 'c.json']) == '--eval_scale 4.5: 0.25 <= S <= 4'
    assert refusal(['--eval_scale', 'nan', '--scale_curve', 'c.json']) == '--eval_scale nan: 0.25 <= S <= 4'
    assert refusal(['--eval_scale', '0.25', '4', '--scale_curve', 'c.json']) == NO_DEVICE
    assert refusal(['--augm_antialias']) == M.AUGM_ANTIALIAS_NEEDS_AUGM_AFFINE
    assert refusal(['--augm_antialias', '--train']) == M.AUGM_ANTIALIAS_NEEDS_AUGM_AFFINE
    assert refusal(['--augm_antialias', '--augm_affine']) == M.AUGM_AFFINE_NEEDS_TRAIN                  # the earlier table speaks first
    assert refusal(['--augm_antialias', '--augm_affine', '--train', '--augm_scale', '0.2', '1']) == M.AUGM_ANTIALIAS_SCALE_FLOOR
    assert refusal(['--augm_antialias', '--augm_affine', '--train', '--augm_scale', '0.25', '1']) == NO_DEVICE
    for feed in ([], ['--device_data'], ['--device_data', '--u8_images']):
        assert refusal(['--augm_antialias', '--augm_affine', '--train'] + feed) == NO_DEVICE
    assert M.EVAL_SCALE_RULES[0][1] == M.EVAL_SCALE_NEEDS_SCALE_CURVE and len(M.EVAL_SCALE_RULES) == 7


def test_every_recorded_refusal_keeps_its_message_with_the_new_flags_added():
    """The cases of tests/test_cli_rules_cpu.py (tests/golden/cli_refusals.json) with the new flags behind them: the new table is walked last, so a
    combination that was refused is refused with the same words, and one that passed ends in the device message or in a message of the new table."""
    with open(os.path.join(HERE, 'golden', 'cli_refusals.json')) as fh:
        doc = json.load(fh)
    recorded = '--gpus [99]: device 99 does not exist (0 visible)'
    new = {m for _, m in M.EVAL_SCALE_RULES if isinstance(m, str)}
    keep = argparse.Namespace(**vars(M.hps))
    wrong, refused = [], 0
    for added in (SWEEP, ['--augm_antialias']):
        for argv, m in doc['cases']:
            want = doc['messages'][m]
            try:
                M.main(list(argv) + added)
                got = None
            except SystemExit as e:
                got = e.code
            finally:
                M.hps = keep
            if want == recorded:
                ok = got == NO_DEVICE or got in new
            else:
                ok, refused = got == want, refused + 1
            if not ok:
                wrong.append((argv + added, want, got))
    assert refused > 1000
    assert not wrong, '%d cases differ; the first: %r' % (len(wrong), wrong[0])


def test_the_command_line_itself_refuses(tmp_path):
    from cli_util import run_cli
    r = run_cli(['--eval_scale', '0.5', '--gpus', '99'], str(tmp_path))
    assert r.returncode != 0 and M.EVAL_SCALE_NEEDS_SCALE_CURVE in r.stderr
    r = run_cli(SWEEP + ['--train', '--flip_test', '--gpus', '99'], str(tmp_path))
    assert r.returncode != 0 and M.FLIP_TEST_IS_EVALUATION_ONLY in r.stderr and 'eval_scale' not in r.stderr
