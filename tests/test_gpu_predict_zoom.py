"""The zoom pass of predict_images (predict.py, main.py --predict --zoom) on the narrow parameters and generated priors of
--synthetic --debug: zoom=True leaves every existing key as it was, every 'zoom' entry equals the composition it is made of -- zoom_windows,
Engine.fit_windows, Engine.torso_infer(cells=), Engine.forward, evaluation.window_to_source -- exactly, skipped people keep their pass-1 values,
people=2 gives an entry per counted slot, and the command line writes the entries."""
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
ENTRY_KEYS = {'zoomed', 'window', 'torso_len', 'pd', 'pd_inside', 'sm', 'sm_inside'}


def _images():
    rs = np.random.RandomState(21)
    return [rs.randint(0, 256, (h, w, 3)).astype(np.uint8) for h, w in SIZES]


def _params():
    """What main.initial_params makes for --synthetic --debug --use_sm (the parameters of tests/test_gpu_predict.py)."""
    p = synth.make_pd_params(debug=True)
    p.update(synth.make_sm_params(synth.synthetic_priors(), kind='init'))
    return p


@pytest.fixture(scope='module')
def world():
    """One engine, the three images, and the two runs every comparison shares: predict_images without and with the zoom pass."""
    from joint_cnn_mrf_amd.engine import Engine
    eng = Engine(device=0).load_params(_params())
    images = _images()
    timing = {}
    plain = P.predict_images(eng, images, use_sm=True, peaks=2, batch_size=2)
    zoomed = P.predict_images(eng, images, use_sm=True, peaks=2, batch_size=2, zoom=True, timing=timing)
    yield eng, images, plain, zoomed, timing
    eng.close()


def _equal(a, b, what):
    if isinstance(a, dict):
        assert a.keys() == b.keys(), what
        for k in a:
            _equal(a[k], b[k], what + '.' + k)
    elif isinstance(a, np.ndarray):
        assert_array_equal(a, b, err_msg=what)
    else:
        assert a == b, what


def _manual(eng, images, persons, batch_size=2):
    """The second pass by hand for persons = [(image, sm, sm_inside, torso cell)]: (windows, skipped, {key: (points, inside)} of the kept)."""
    image = np.array([p[0] for p in persons])
    sizes = [im.shape[:2] for im in images]
    geom1 = np.array([EV.fit_geometry(*sizes[b], *P.FRAME) + sizes[b] for b in image])
    wins, cells, skipped = P.zoom_windows(np.stack([p[1] for p in persons]), np.stack([p[2] for p in persons]),
                                          np.array([p[3] for p in persons]), geom1, image=image)
    keep = np.flatnonzero(~skipped)
    second = {}
    if len(keep):
        x2, geom2 = eng.fit_windows(images, wins[keep])
        cells_dev = torch.as_tensor(cells[keep], device='cuda:0')
        coords = {'pd': [], 'sm': []}
        for lo in range(0, len(keep), batch_size):
            torso = eng.torso_infer(None, cells=cells_dev[lo:lo + batch_size].contiguous())['torso']
            r2 = eng.forward(x2[lo:lo + batch_size], torso=torso, use_sm=True, want_prob=False)
            for k in coords:
                coords[k].append(r2[k + '_coords'])
        torch.cuda.synchronize()
        for k in coords:
            pts = torch.cat(coords[k]).cpu().numpy().transpose(0, 2, 1).astype(np.float64) * 8
            second[k] = EV.window_to_source(pts, geom2, wins[keep], np.array(sizes))
    return wins, skipped, keep, second


def _check_entries(entries, persons, pd_of, wins, skipped, keep, second):
    assert len(entries) == len(persons)
    at = {int(i): n for n, i in enumerate(keep)}
    for i, (e, (b, sm, sm_inside, _)) in enumerate(zip(entries, persons)):
        assert set(e) == ENTRY_KEYS
        assert e['zoomed'] is (not bool(skipped[i])) and e['window'] == tuple(wins[i, 1:].tolist())
        assert e['torso_len'] == float(P.torso_length(sm))
        if e['zoomed']:
            for k in ('pd', 'sm'):
                assert e[k].shape == (9, 2) and e[k + '_inside'].dtype == bool
                assert_array_equal(e[k], second[k][0][at[i]])
                assert_array_equal(e[k + '_inside'], second[k][1][at[i]])
        else:
            assert_array_equal(e['sm'], sm)
            assert_array_equal(e['sm_inside'], sm_inside)
            assert_array_equal(e['pd'], pd_of[b][0])
            assert_array_equal(e['pd_inside'], pd_of[b][1])


def test_zoom_keeps_every_existing_key(world):
    eng, images, plain, zoomed, timing = world
    assert timing['fit_ms'] > 0 and timing['forward_ms'] > 0 and timing['zoom_fit_ms'] >= 0 and timing['zoom_forward_ms'] >= 0
    for b, (a, z) in enumerate(zip(plain, zoomed)):
        assert 'zoom' not in a and set(z) == set(a) | {'zoom'}
        _equal(a, {k: v for k, v in z.items() if k != 'zoom'}, 'image %d' % b)


def test_zoom_entries_are_the_manual_composition(world):
    eng, images, plain, zoomed, timing = world
    # predict_images zooms batch by batch (2 + 1 images); the composition here takes all three at once: the windows name the same images
    persons = [(b, r['sm'], r['sm_inside'], r['torso_cell']) for b, r in enumerate(plain)]
    wins, skipped, keep, second = _manual(eng, images, persons)
    entries = [z['zoom'] for z in zoomed]
    assert all(len(e) == 1 for e in entries)
    _check_entries([e[0] for e in entries], persons, {b: (r['pd'], r['pd_inside']) for b, r in enumerate(plain)}, wins, skipped, keep, second)
    if len(keep):
        assert timing['zoom_fit_ms'] > 0 and timing['zoom_forward_ms'] > 0


def test_skipped_person_keeps_the_first_pass(world):
    """A 480 x 60 image fills a twelfth of the frame's width: on these parameters a torso joint of the first pass lies in a bar, so the person
    is skipped -- zoomed False, the pass-1 joints -- beside a person of the same batch who is zoomed."""
    eng, images, plain, zoomed, timing = world
    narrow = np.random.RandomState(22).randint(0, 256, (480, 60, 3)).astype(np.uint8)
    pair = [images[1], narrow]
    base = P.predict_images(eng, pair, use_sm=True)
    got = P.predict_images(eng, pair, use_sm=True, zoom=True)
    persons = [(b, r['sm'], r['sm_inside'], r['torso_cell']) for b, r in enumerate(base)]
    wins, skipped, keep, second = _manual(eng, pair, persons)
    assert not base[1]['sm_inside'][[0, 3, 6, 7]].all() and skipped.tolist() == [False, True]
    _check_entries([g['zoom'][0] for g in got], persons, {b: (r['pd'], r['pd_inside']) for b, r in enumerate(base)}, wins, skipped, keep, second)
    e = got[1]['zoom'][0]
    assert e['zoomed'] is False
    assert_array_equal(e['sm'], base[1]['sm'])
    assert_array_equal(e['pd'], base[1]['pd'])
    assert got[0]['zoom'][0]['zoomed'] is True


def test_zoom_with_people(world):
    eng, images, plain, zoomed, timing = world
    got = P.predict_images(eng, images, use_sm=True, people=2, zoom=True)
    base = P.predict_images(eng, images, use_sm=True, people=2)
    persons, entries = [], []
    for b, (g, a) in enumerate(zip(got, base)):
        _equal(a, {k: v for k, v in g.items() if k != 'zoom'}, 'image %d' % b)
        n = g['people']['count']
        assert 1 <= n <= 2 and len(g['zoom']) == n
        persons.extend((b, g['people']['sm'][m], g['people']['sm_inside'][m], g['people']['torso_cell'][m]) for m in range(n))
        entries.extend(g['zoom'])
    wins, skipped, keep, second = _manual(eng, images, persons, batch_size=16)
    _check_entries(entries, persons, {b: (r['pd'], r['pd_inside']) for b, r in enumerate(base)}, wins, skipped, keep, second)


def test_zoom_needs_use_sm(world):
    eng, images = world[:2]
    with pytest.raises(ValueError):
        P.predict_images(eng, images, use_sm=False, zoom=True)


def test_cli_predict_zoom(world, tmp_path):
    """--predict --zoom in a fresh process: the document's 'zoom' entries are predict_images', and the JSON line says so."""
    eng, images, plain, zoomed, timing = world
    d = tmp_path / 'photos'
    d.mkdir()
    for i, im in enumerate(images):
        np.save(str(d / ('img%d.npy' % i)), im)
    out = str(tmp_path / 'pred.json')
    res = run_cli(['--synthetic', '--debug', '--use_sm', '--gpus', '0', '--batch_size', '2', '--peaks', '2',
                   '--predict', str(d), '--predictions', out, '--zoom'], str(tmp_path))
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    line = json.loads(res.stdout.strip().splitlines()[-1])
    assert line['predict'] is True and line['zoom'] is True and line['zoom_fit_ms'] >= 0 and line['zoom_forward_ms'] >= 0
    doc = json.load(open(out))
    for e, g in zip(doc['images'], zoomed):
        assert_array_equal(np.array(e['sm'], np.float64), g['sm'])
        assert len(e['zoom']) == len(g['zoom']) == 1
        ze, zg = e['zoom'][0], g['zoom'][0]
        assert set(ze) == ENTRY_KEYS and ze['zoomed'] is zg['zoomed'] and tuple(ze['window']) == zg['window'] and ze['torso_len'] == zg['torso_len']
        for k in ('pd', 'sm'):
            assert_array_equal(np.array(ze[k], np.float64), zg[k])
            assert_array_equal(np.array(ze[k + '_inside'], bool), zg[k + '_inside'])
