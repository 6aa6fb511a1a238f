"""Images of any size through the tower (predict.py, main.py --predict): predict_images against the composition of the calls it
is made of -- Engine.fit_images, Engine.forward(torso='infer'), evaluation.fit_to_source -- and the command line against predict_images, on the
narrow parameters and generated priors of --synthetic --debug."""
import argparse
import json
import os

import numpy as np
import pytest
import torch
from numpy.testing import assert_array_equal

from cli_util import run_cli
import joint_cnn_mrf_amd  # noqa: F401
from joint_cnn_mrf_amd import evaluation as EV
from joint_cnn_mrf_amd import predict as P
from joint_cnn_mrf_amd import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = ((480, 720), (300, 400), (640, 360))


def _images():
    rs = np.random.RandomState(21)
    return [rs.randint(0, 256, (h, w, 3)).astype(np.uint8) for h, w in SIZES]


def _params():
    """What main.initial_params makes for --synthetic --debug --use_sm."""
    p = synth.make_pd_params(debug=True)
    p.update(synth.make_sm_params(synth.synthetic_priors(), kind='init'))
    return p


@pytest.fixture(scope='module')
def world():
    """One engine, the three images, and the one forward on their fitted frames that every comparison shares."""
    from joint_cnn_mrf_amd.engine import Engine
    eng = Engine(device=0).load_params(_params())
    images = _images()
    x, geom = eng.fit_images(images)
    r = eng.forward(x, 'infer', use_sm=True, want_prob=False, peaks=2, decode=True)
    torch.cuda.synchronize()
    yield eng, images, x, geom, r
    eng.close()


def _points(coords):
    return coords.cpu().numpy().transpose(0, 2, 1).astype(np.float64) * 8


def test_predict_images_is_fit_forward_and_map_back(world):
    eng, images, x, geom, r = world
    timing = {}
    got = P.predict_images(eng, images, use_sm=True, peaks=2, decode=True, batch_size=2, timing=timing)      # two batches: 2 + 1 images
    assert len(got) == 3 and timing['fit_ms'] > 0 and timing['forward_ms'] > 0
    assert_array_equal(geom[:, 4:], np.array(SIZES, np.int32))
    assert geom[:, :4].tolist() == [[0, 0, 480, 720], [0, 40, 480, 640], [0, 225, 480, 270]]
    want = {k: EV.fit_to_source(_points(r[k + '_coords']), geom) for k in ('pd', 'sm')}
    want_pk = {k: EV.fit_to_source(EV.peaks_to_pixels(r[k + '_peaks']), geom) for k in ('pd', 'sm')}
    want_pose = EV.fit_to_source(EV.pose_to_pixels(r['pose'], r['pd_peaks']), geom)
    cells = r['torso_cell'].cpu().numpy()
    for b, g in enumerate(got):
        assert g['size'] == SIZES[b] and g['joint_names'] == list(P.JOINT_NAMES) and g['geom'] == tuple(geom[b].tolist())
        for k in ('pd', 'sm'):
            assert g[k].shape == (9, 2)
            assert_array_equal(g[k], want[k][0][b])
            assert_array_equal(g[k + '_inside'], want[k][1][b])
            assert_array_equal(g[k + '_peaks'], want_pk[k][0][b])
            assert_array_equal(g[k + '_peaks_inside'], want_pk[k][1][b])
        assert_array_equal(g['pose'], want_pose[0][b])
        assert g['torso_cell'] == tuple(cells[b].tolist())
        h, w = SIZES[b]
        inside = g['pd_inside']
        assert ((g['pd'][inside] > -0.5) & (g['pd'][inside] < [h - 0.5, w - 0.5])).all()      # a point of the content lies in the source image


def test_equal_size_image_is_the_plain_forward(world):
    """The 480x720 image is fitted as a bit copy, so its joints are those of the forward on the image itself, in its own pixels: coords * 8."""
    eng, images, x, geom, r = world
    assert_array_equal(x[0].cpu().numpy(), images[0])
    own = eng.forward(torch.as_tensor(images[0][None], device='cuda:0'), 'infer', use_sm=True, want_prob=False)
    got = P.predict_images(eng, images[:1], use_sm=True)[0]
    torch.cuda.synchronize()
    assert_array_equal(got['pd'], _points(own['pd_coords'])[0])
    assert_array_equal(got['sm'], _points(own['sm_coords'])[0])
    assert got['pd_inside'].all() and got['sm_inside'].all()
    assert got['torso_cell'] == tuple(own['torso_cell'].cpu().numpy()[0].tolist())


def test_without_spatial_model_and_with_people(world):
    eng, images, x, geom, r = world
    got = P.predict_images(eng, images, use_sm=False)
    for b, g in enumerate(got):
        assert 'sm' not in g and 'torso_cell' not in g
        assert_array_equal(g['pd'], EV.fit_to_source(_points(r['pd_coords']), geom)[0][b])
    got = P.predict_images(eng, images, use_sm=True, people=2)
    r2 = eng.forward(x, 'infer', use_sm=True, want_prob=False, people=2)
    torch.cuda.synchronize()
    cm = r2['people']['sm_coords'].cpu().numpy()      # [B,M,2,K]
    for b, g in enumerate(got):
        assert g['people']['count'] == int(r2['people']['count'][b]) and g['people']['sm'].shape == (2, 9, 2)
        pts = cm[b].transpose(0, 2, 1).astype(np.float64)
        pts = np.where(pts < 0, -1.0, pts * 8)
        want, inside = EV.fit_to_source(pts[None], geom[b:b + 1])
        assert_array_equal(g['people']['sm'], want[0])
        assert_array_equal(g['people']['sm_inside'], inside[0])
        assert_array_equal(g['sm'], EV.fit_to_source(_points(r2['sm_coords']), geom)[0][b])
    with pytest.raises(ValueError):
        P.predict_images(eng, [])
    with pytest.raises(TypeError):
        P.predict_images(eng, [images[0].astype(np.float32)])


# ------------------------------------------------------------------ the command line
def test_cli_predict(world, tmp_path):
    """Three .npy files in a directory (expanded in sorted order) -> the JSON document holds predict_images' values; one JSON line on stdout."""
    eng, images, x, geom, r = world
    d = tmp_path / 'photos'
    d.mkdir()
    for i, im in enumerate(images):
        np.save(str(d / ('img%d.npy' % i)), im)
    (d / 'notes.txt').write_text('not an image')
    out = str(tmp_path / 'out' / 'pred.json')
    res = run_cli(['--synthetic', '--debug', '--use_sm', '--gpus', '0', '--batch_size', '2', '--peaks', '2', '--predict', str(d), '--predictions', out], str(tmp_path))
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    line = json.loads(res.stdout.strip().splitlines()[-1])
    assert line['predict'] is True and line['n_images'] == 3 and line['fit_ms'] > 0 and line['forward_ms'] > 0
    doc = json.load(open(out))
    assert doc['joint_names'] == list(P.JOINT_NAMES) and doc['frame'] == [480, 720]
    assert [os.path.basename(e['path']) for e in doc['images']] == ['img0.npy', 'img1.npy', 'img2.npy']
    want = P.predict_images(eng, images, use_sm=True, peaks=2, batch_size=2)
    for e, g in zip(doc['images'], want):
        assert tuple(e['size']) == g['size'] and tuple(e['torso_cell']) == g['torso_cell']
        for k in ('pd', 'sm', 'pd_peaks', 'sm_peaks'):
            assert_array_equal(np.array(e[k], np.float64), g[k])
            assert_array_equal(np.array(e[k + '_inside'], bool), g[k + '_inside'])


def test_cli_refusals(tmp_path):
    """--predict with --train, --multiscale, --flip_test, --det_curve, --device_data or without --predictions: refused with the flag's message
    constant, before any device is touched (so the parser is driven in-process; main() assigns the module's hps, which is put back)."""
    from joint_cnn_mrf_amd import main as M
    base = ['--synthetic', '--debug', '--gpus', '0', '--predict', str(tmp_path / 'a.npy')]
    keep = argparse.Namespace(**vars(M.hps))
    try:
        for extra, message in ((['--train'], M.PREDICT_NOT_WITH_TRAIN), (['--multiscale'], M.PREDICT_NOT_WITH_MULTISCALE), (['--flip_test'], M.PREDICT_NOT_WITH_FLIP_TEST),
                               (['--det_curve', str(tmp_path / 'c.json')], M.PREDICT_NOT_WITH_DET_CURVE), (['--device_data'], M.PREDICT_NOT_WITH_DEVICE_DATA)):
            with pytest.raises(SystemExit) as ei:
                M.main(base + ['--predictions', str(tmp_path / 'o.json')] + extra)
            assert str(ei.value) == message and extra[0] in message, extra
        with pytest.raises(SystemExit) as ei:
            M.main(base)
        assert str(ei.value) == M.PREDICT_NEEDS_PREDICTIONS
    finally:
        M.hps = keep
    res = run_cli(base + ['--predictions', str(tmp_path / 'o.json'), '--flip_test'], str(tmp_path))      # and once through the real entry point
    assert res.returncode != 0 and '--flip_test' in res.stderr
    assert not (tmp_path / 'o.json').exists()
