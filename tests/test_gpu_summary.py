"""TensorBoard summaries on the GPU (csrc/summary.hip, joint_cnn_mrf_amd/summary.py): the segmented statistics and
TF-1.x histograms against numpy, the quantiser and the heat-map overlays against the restatements of tests/tb_ref.py, and the
command line end to end through the independent event-file decoder."""
import io
import os
import re
import sys

import numpy as np
import pytest
import torch

from cli_util import run_cli
import joint_cnn_mrf_amd  # noqa: F401
from joint_cnn_mrf_amd import synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tb_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIM = R.default_limits()


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), device='cuda:0')


def _engine():
    from joint_cnn_mrf_amd.engine import Engine
    p = synth.make_pd_params(debug=True, bn='trained', conv6_gain=8.0)
    p.update(synth.make_sm_params(synth.synthetic_priors(), kind='trained'))
    return Engine(device=0).load_params(p), p


def _check_stats(st, cn, u_segments, what=''):
    """st / cn rows against numpy float64 on the float32 values u of each segment (finite values only)."""
    for i, u in enumerate(u_segments):
        u = np.asarray(u, np.float32)
        fin = u[np.isfinite(u)].astype(np.float64)
        mn, mx, num, s, ss, counts = R.histogram(fin, LIM)
        assert cn[i, 0] == num and cn[i, 1] == int((fin > 0).sum()) and cn[i, 2] == u.size - fin.size, (what, i)
        assert np.array_equal(cn[i, 3:], counts), (what, i, np.nonzero(cn[i, 3:] != counts))
        assert st[i, 0] == mn and st[i, 1] == mx, (what, i, st[i, :2], mn, mx)
        # fixed-order fold in double vs numpy's pairwise sum: both within a few double roundings of sum(|u|)
        tol = 1e-13 * max(np.abs(fin).sum(), 1e-300) * 8
        assert abs(st[i, 2] - s) <= tol, (what, i, st[i, 2], s)
        assert abs(st[i, 3] - ss) <= 1e-13 * max(ss, 1e-300) * 8, (what, i, st[i, 3], ss)


def _adversarial(rng):
    f32 = np.float32
    vals = [0.0, -0.0, 1e-45, -1e-45, 1e-40, -3e-39, 3.4e38, -3.4e38, 1.0, -1.0, 1e-12, -1e-12]
    for k in list(range(0, 774, 37)) + [1, 2, 772, 773]:                 # floats on and either side of bucket edges
        e = f32(LIM[LIM.size // 2 + 1 + k])
        for v in (np.nextafter(e, f32(0)), e, np.nextafter(e, f32(np.inf))):
            vals += [float(v), -float(v)]
    return np.array(vals, np.float32)


def test_stats_against_numpy_adversarial():
    """Segments of length 0, 1, odd and longer than one chunk of the grid; ±0, denormals, edge neighbours, ±3.4e38; scale 1 (the values
    sit on the edges) and a non-trivial scale (fp32 product).  Bucket counts exact, two calls bitwise identical; a NaN / Inf segment is
    counted and the host raises ValueError naming the tensor; the handle keeps working."""
    from joint_cnn_mrf_amd import summary as S
    eng, _ = _engine()
    rng = np.random.RandomState(3)
    adv = _adversarial(rng)
    big = (rng.standard_normal(200_003) * 0.01).astype(np.float32)
    big[::97] = adv[np.arange(big[::97].size) % adv.size]
    pos = rng.uniform(0, 5, 31).astype(np.float32)
    data = np.concatenate([adv, big, pos, np.array([2.5], np.float32)])
    segs = [(0, 0), (data.size - 1, 1), (adv.size + big.size, 31), (0, adv.size), (adv.size, big.size), (5, 77_777)]
    d = dev(data)
    for scale in (1.0, 0.7310585):
        st, cn = eng.tensor_stats(d, segs, scale=scale)
        st2, cn2 = eng.tensor_stats(d, segs, scale=scale)
        assert st.tobytes() == st2.tobytes() and cn.tobytes() == cn2.tobytes()
        u = [np.float32(scale) * data[o:o + n] for o, n in segs]
        _check_stats(st, cn, u, 'scale %g' % scale)
        assert st[0, 0] == sys.float_info.max and st[0, 1] == -sys.float_info.max and cn[0, 0] == 0      # empty: TF's initial min / max
    bad = data.copy()
    bad[7] = np.nan
    bad[adv.size + 11] = np.inf
    st, cn = eng.tensor_stats(dev(bad), segs, scale=1.0)
    assert cn[3, 2] == 1 and cn[4, 2] == 1 and cn[2, 2] == 0
    with pytest.raises(ValueError, match='grads/conv5/weights/gradients'):
        S.histogram_value('grads/conv5/weights/gradients', st[3], cn[3])
    _, cn_over = eng.tensor_stats(d, [(0, adv.size)], scale=2.0)          # 2 * 3.4e38 overflows to inf: counted, not binned
    assert cn_over[0, 2] == 2
    st3, cn3 = eng.tensor_stats(d, segs, scale=1.0)
    _check_stats(st3, cn3, [data[o:o + n] for o, n in segs], 'after NaN')
    with pytest.raises(RuntimeError, match='one stored trainable tensor|jcm_train_begin|clip_norm'):
        eng.tensor_stats(None, [(0, 10)])                                  # no training state: refused, no device access
    eng.close()


def test_full_width_parameters_and_gradients():
    """After one real training step at full width (218 tensors, 58.7 M elements): the stored parameters read in place and the clipped
    gradients against numpy on the copied data."""
    from joint_cnn_mrf_amd.engine import Engine
    from joint_cnn_mrf_amd.train import Trainer
    p = synth.make_pd_params(debug=False, bn='trained')
    p.update(synth.make_sm_params(synth.synthetic_priors(), kind='init'))
    eng = Engine(device=0).load_params(p)
    tr = Trainer(eng, use_sm=True)
    trainable = {k: int(np.asarray(v).size) for k, v in p.items() if not k.endswith(('moving_mean', 'moving_variance'))}
    assert [n for n, _, _ in tr.layout] == sorted(trainable) and tr.n_elements == sum(trainable.values()) > 58_000_000
    x, y = dev(synth.make_images(2, seed=5)), dev(synth.make_targets(2, seed=6))
    tr.loss_and_grads(x, y)
    norm = tr.apply(want_norm=True)
    segs = [(o, c) for _, o, c in tr.layout]
    st, cn = eng.tensor_stats(None, segs)
    flat = np.concatenate([tr.get_tensor(n, (c,)) for n, _, c in tr.layout])
    _check_stats(st, cn, [flat[o:o + c] for o, c in segs], 'params')
    stg, cng = eng.tensor_stats(tr.grads, segs, clip_norm=4.0)
    f = np.float32(4.0) / max(np.float32(norm), np.float32(4.0))
    g = tr.grads.cpu().numpy()
    _check_stats(stg, cng, [g[o:o + c] * f for o, c in segs], 'grads')
    eng.close()


def test_quantiser_branches():
    eng, _ = _engine()
    rng = np.random.RandomState(9)
    for C in (1, 3):
        x = rng.uniform(-0.3, 2.0, (5, 37, 53, C)).astype(np.float32)
        x[1] = np.abs(x[1])                          # min >= 0: 255 / max
        x[2] = 0.0                                   # all zero: scale 0
        x[3] *= 1e-7                                 # max below 1e-6: scale 0, offset 128
        x[4, 3, 4, 0] = np.nan                       # non-finite pixels: left out of min / max, drawn red
        x[4, 5, 6, C - 1] = np.inf
        x[4, 7, 8, 0] = -50.0
        got = eng.image_u8(dev(x)).cpu().numpy()
        for b in range(5):
            want = R.normalize_float_image(x[b])
            assert np.array_equal(got[b], want), (C, b, np.argwhere(got[b] != want)[:5])
        assert got[2].max() == 0 and (got[3] == 128).all()
        assert got[4, 3, 4, 0] == 255 and (C == 1 or (got[4, 3, 4, 1:] == 0).all())
    eng.close()


def test_overlays_against_restatement():
    eng, _ = _engine()
    rng = np.random.RandomState(11)
    B = 3
    x = rng.uniform(0, 1, (B, 480, 720, 3)).astype(np.float32)
    x[2] *= 0.5
    x[1, 100, 200, 1] = np.nan
    hm = rng.exponential(1.0, (B, 60, 90, 9)).astype(np.float32)
    hm /= hm.sum(axis=(1, 2), keepdims=True)
    got = eng.hm_overlay(dev(x), dev(hm), n=B).cpu().numpy()
    assert got.shape == (B, 10, 480, 720, 3)
    want32 = R.overlay_u8(x, hm, np.float32)
    assert np.array_equal(got, want32), np.argwhere(got != want32)[:5]
    want64 = R.overlay_u8(x, hm, np.float64)
    assert np.abs(got.astype(int) - want64.astype(int)).max() <= 1
    assert (got[1, :, 100, 200] == [255, 0, 0]).all()                 # the NaN pixel: red in every picture
    first2 = eng.hm_overlay(dev(x), dev(hm), n=2).cpu().numpy()
    assert np.array_equal(first2, got[:2])
    eng.close()


def _run_ok(args, cwd, timeout=900):
    r = run_cli(args, cwd, timeout=timeout)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return r.stdout


def _events(d):
    files = [f for f in os.listdir(d) if f.startswith('events.out.tfevents.')]
    assert len(files) == 1, files
    evs = R.read_events(os.path.join(d, files[0]), check_crc=True)
    assert evs[0]['file_version'] == 'brain.Event:2'
    by_step = {}
    for e in evs[1:]:
        for v in e['values']:
            by_step.setdefault(e['step'], {})[v['tag']] = v
    return by_step


def _sizes(use_sm=True):
    p = synth.make_pd_params(debug=True)
    if use_sm:
        p.update(synth.make_sm_params(synth.synthetic_priors(), kind='init'))
    return {k: int(np.asarray(v).size) for k, v in p.items()}


def test_cli_train_writes_summaries(tmp_path):
    from PIL import Image
    D = tmp_path / 'tb'
    out = _run_ok(['--train', '--debug', '--use_sm', '--synthetic', '--synthetic_size', '8', '--batch_size', '4', '--gpus', '0', '0', '--n_epochs', '2',
                '--tb_dir', str(D), '--model_path', str(tmp_path / 'models_ex')], str(tmp_path))
    runs = os.listdir(str(D))
    assert len(runs) == 1 and sorted(os.listdir(str(D / runs[0]))) == ['test', 'train']
    printed = {}
    for line in out.splitlines():
        m = re.match(r'Epoch (\d+)\s+test_dr (\S+) (\S+)\s+train_dr (\S+) (\S+)\s+test_mse (\S+) (\S+)\s+train_mse (\S+) (\S+)', line)
        if m:
            v = [float(t) for t in m.groups()[1:]]
            printed[int(m.group(1))] = {'test': [v[4], v[5], v[0], v[1]], 'train': [v[6], v[7], v[2], v[3]]}
    assert sorted(printed) == [0, 1, 2]
    sizes = _sizes()
    trainable = [k for k in sizes if not k.endswith(('moving_mean', 'moving_variance'))]
    for split in ('train', 'test'):
        ev = _events(str(D / runs[0] / split))
        assert sorted(ev) == [0, 1, 2]
        for step, tags in ev.items():
            want = ['main/mse_pd', 'main/mse_sm', 'main/det_rate_pd', 'main/det_rate_sm', 'input/image/0', 'input/image/3',
                    'hm_pred_spatial_model_lwri/image/0', 'hm_target_nose/image/3', 'img_plus_all_joints_pred_part_detector/image/0',
                    'pre_activ_pairwise_energies_lsho_lelb/std', 'pre_activ_pairwise_biases_nose_torso/histogram',
                    'pairwise_potential_lsho_lelb/image/0', 'conv_filters_1/w_conv1/image/15', 'grads/conv5/weights']
            if step > 0:
                want += ['grads/conv5/weights/gradients', 'grads/conv5/weights/gradients_1', 'grads/energy_lsho_lelb/gradients']
            missing = [t for t in want if t not in tags]
            assert not missing, (split, step, missing)
            assert 'input/image/4' not in tags and 'conv_filters_1/w_conv1/image/16' not in tags      # debug width: 16 conv1 filters
            assert ('grads/conv5/weights/gradients' in tags) == (step > 0)
            for i, name in enumerate(['main/mse_pd', 'main/mse_sm', 'main/det_rate_pd', 'main/det_rate_sm']):
                assert abs(tags[name]['simple_value'] - printed[step][split][i]) <= 1e-3, (split, step, name)
            for n in trainable:
                assert tags['grads/' + n]['histo']['num'] == sizes[n], n
                assert sum(tags['grads/' + n]['histo']['bucket']) == sizes[n], n
                if step > 0 and ('weights' in n or 'energy' in n):
                    assert tags['grads/%s/gradients' % n]['histo']['num'] == sizes[n]
            for tag, v in tags.items():
                if 'image' in v:
                    im = np.asarray(Image.open(io.BytesIO(v['image']['png'])))
                    h, w = v['image']['height'], v['image']['width']
                    if tag.startswith(('input', 'hm_', 'img_plus')):
                        assert (h, w) == (480, 720) and im.shape == (480, 720, 3), tag
                    elif tag.startswith('pairwise_potential'):
                        assert im.shape == (120, 180), tag
                    elif tag.startswith('pairwise_biases'):
                        assert im.shape == (60, 90), tag
                    else:
                        assert im.shape == (5, 5, 3), tag


def test_cli_eval_summaries_and_default_off(tmp_path):
    """The evaluation run with --tb_dir writes the step-0 summaries without the gradient parts; without --tb_dir nothing is written."""
    common = ['--debug', '--use_sm', '--synthetic', '--synthetic_size', '4', '--batch_size', '2', '--gpus', '0']
    D = tmp_path / 'tb'
    _run_ok(common + ['--tb_dir', str(D)], str(tmp_path))
    run = os.listdir(str(D))[0]
    for split in ('train', 'test'):
        ev = _events(str(D / run / split))
        assert sorted(ev) == [0]
        tags = ev[0]
        assert 'hm_pred_spatial_model_lwri/image/1' in tags and 'grads/conv5/weights' in tags
        assert not any(t.endswith('/gradients') or t.endswith('/gradients_1') for t in tags)
    plain = tmp_path / 'plain'
    plain.mkdir()
    _run_ok(common, str(plain))
    for dirpath, _, files in os.walk(str(plain)):
        assert not any(f.startswith('events.out.tfevents') for f in files), dirpath
    assert not os.path.exists(str(plain / 'tb'))
