"""Pictures of --predict (predict.render_images, main.py --render): the PNG files of the command line against render_images on
the same results, the predictions document against the one written without --render, and predict_images' keys with and without keep_maps, on
the narrow parameters and generated priors of --synthetic --debug."""
import json
import os
import struct
import zlib

import numpy as np
import pytest
import torch
from numpy.testing import assert_array_equal

from cli_util import run_cli
import render_ref as R
import joint_cnn_mrf_amd  # noqa: F401
from joint_cnn_mrf_amd import predict as P
from joint_cnn_mrf_amd import synth

pytestmark = pytest.mark.gpu
SIZES = ((120, 180), (75, 100), (160, 90))
KEYS = {'size', 'joint_names', 'geom', 'pd', 'pd_inside', 'sm', 'sm_inside', 'torso_cell'}      # predict_images(use_sm=True) before keep_maps existed


def _images():
    rs = np.random.RandomState(31)
    return [rs.randint(0, 256, (h, w, 3)).astype(np.uint8) for h, w in SIZES]


def decode_png(data):
    """What summary.encode_png writes: 8-bit RGB, one IDAT, every row with the Sub filter."""
    assert data[:8] == b'\x89PNG\r\n\x1a\n'
    at, chunks = 8, {}
    while at < len(data):
        n, kind = struct.unpack('>I4s', data[at:at + 8])
        chunks[kind] = data[at + 8:at + 8 + n]
        at += 12 + n
    w, h, depth, colour = struct.unpack('>IIBB', chunks[b'IHDR'][:10])
    assert (depth, colour) == (8, 2)
    rows = np.frombuffer(zlib.decompress(chunks[b'IDAT']), np.uint8).reshape(h, 1 + 3 * w)
    assert (rows[:, 0] == 1).all()
    return np.cumsum(rows[:, 1:].reshape(h, w, 3).astype(np.int64), axis=1).astype(np.uint8)


@pytest.fixture(scope='module')
def world():
    from joint_cnn_mrf_amd.engine import Engine
    p = synth.make_pd_params(debug=True)
    p.update(synth.make_sm_params(synth.synthetic_priors(), kind='init'))
    eng = Engine(device=0).load_params(p)
    yield eng, _images()
    eng.close()


def test_keep_maps_adds_one_key_and_changes_no_value(world):
    eng, images = world
    plain = P.predict_images(eng, images, use_sm=True, batch_size=2)
    kept = P.predict_images(eng, images, use_sm=True, batch_size=2, keep_maps=True)
    for a, b in zip(plain, kept):
        assert set(a) == KEYS and set(b) == KEYS | {'maps'}
        for k in KEYS:
            assert_array_equal(np.asarray(a[k]), np.asarray(b[k]))
        assert set(b['maps']) == {'pd', 'sm'} and all(m.shape == (60, 90, 9) and m.is_cuda and m.dtype == torch.float32 for m in b['maps'].values())
    assert set(P.predict_images(eng, images[:1], use_sm=False, keep_maps=True)[0]['maps']) == {'pd'}
    assert P.predictions_document(['a', 'b', 'c'], kept) == P.predictions_document(['a', 'b', 'c'], plain)


def test_render_images_is_the_restatement(world):
    """render_images = skeleton_primitives + Engine.render_poses batch by batch: against tests/render_ref.py on the same primitives and maps."""
    eng, images = world
    res = P.predict_images(eng, images, use_sm=True, batch_size=2, keep_maps=True)
    prims = P.skeleton_primitives(res)
    assert prims.shape[0] > 0
    timing = {}
    got = P.render_images(eng, images, res, batch_size=2, timing=timing)
    assert timing['render_ms'] > 0 and [g.shape for g in got] == [im.shape for im in images]
    for g, want in zip(got, R.render(images, prims)):
        assert_array_equal(g, want)
    hm = np.stack([r['maps']['pd'].cpu().numpy() for r in res])
    geom = np.array([r['geom'][:4] for r in res], np.int32)
    want = R.render(images, P.skeleton_primitives(res, which='pd'), hm=hm, geom=geom, heat_mask=P.HEAT_MASK, heat_gain=255, stride=8)
    for g, w in zip(P.render_images(eng, images, res, heat='pd', which='pd', batch_size=2), want):
        assert_array_equal(g, w)
    with pytest.raises(ValueError, match='keep_maps'):
        P.render_images(eng, images, P.predict_images(eng, images, use_sm=True), heat='sm')


def test_cli_render(world, tmp_path):
    eng, images = world
    d = tmp_path / 'photos'
    d.mkdir()
    for i, im in enumerate(images):
        np.save(str(d / ('img%d.npy' % i)), im)
    base = ['--synthetic', '--debug', '--use_sm', '--gpus', '0', '--batch_size', '2', '--predict', str(d)]
    plain, drawn, pics = str(tmp_path / 'plain.json'), str(tmp_path / 'drawn.json'), str(tmp_path / 'pics')
    res = run_cli(base + ['--predictions', plain], str(tmp_path))
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    assert 'render_ms' not in json.loads(res.stdout.strip().splitlines()[-1])
    res = run_cli(base + ['--predictions', drawn, '--render', pics, '--render_heat', 'sm'], str(tmp_path))
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    assert json.loads(res.stdout.strip().splitlines()[-1])['render_ms'] > 0
    assert open(plain, 'rb').read() == open(drawn, 'rb').read()
    assert sorted(os.listdir(pics)) == ['00000_img0.png', '00001_img1.png', '00002_img2.png']
    results = P.predict_images(eng, images, use_sm=True, batch_size=2, keep_maps=True)
    want = P.render_images(eng, images, results, heat='sm', batch_size=2)
    for name, w, im in zip(sorted(os.listdir(pics)), want, images):
        got = decode_png(open(os.path.join(pics, name), 'rb').read())
        assert_array_equal(got, w)
        assert (got != im).any()
