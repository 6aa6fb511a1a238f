"""bench.py as it is run for every change: a plain run measures the headline configuration only (contract keys, exactly --steps timed steps,
no roofline / other configurations / CPU baseline / detail file), and --dump-outputs writes what the timed path returned in its last step."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(flags, cwd, timeout=600):
    env = dict(os.environ)
    for k in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK', 'JCM_BENCH_FORCE_DIST'):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py')] + flags, cwd=cwd, env=env, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, 'bench.py %s failed (%d)\n%s\n%s' % (' '.join(flags), r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    return json.loads(lines[-1])


def test_plain_run_line_and_dumped_coordinates(tmp_path):
    from joint_cnn_mrf_amd import synth
    from joint_cnn_mrf_amd.engine import Engine
    import bench
    out = tmp_path / 'out'
    d = _bench(['--gpus', '1', '--debug', '--batch', '2', '--steps', '3', '--warmup', '1', '--dump-outputs', str(out)], str(tmp_path))
    for k in ('metric', 'value', 'unit', 'higher_is_better', 'dtype', 'ms_per_step', 'median_ms_per_step'):
        assert k in d, k
    assert d['steps'] == 3 and d['warmup'] == 1 and d['n_gpus'] == 1 and d['unit'] == 'images/sec' and d['higher_is_better'] is True
    assert abs(d['value'] - 2 / (d['ms_per_step'] * 1e-3)) <= 1e-3 * d['value']
    for k in ('roofline', 'cpu_baseline', 'configs', 'ms_per_step_profiled', 'detail'):
        assert k not in d, k
    assert not (tmp_path / 'bench_detail.json').exists()
    assert sorted(os.listdir(out)) == ['pd_coords.npy', 'sm_coords.npy']
    # the same images and weights through the engine directly
    params = synth.make_pd_params(debug=True)
    params.update(synth.make_sm_params(synth.synthetic_priors(), kind='init'))
    x, torso = bench.resident_inputs(2, 0, torch.device('cuda', 0))
    eng = Engine(device=0).load_params(params)
    r = eng.forward(x, torso, use_sm=True, want_prob=False)
    torch.cuda.synchronize()
    for k in ('pd_coords', 'sm_coords'):
        got = np.load(out / (k + '.npy'))
        assert got.dtype == np.float32 and got.shape == (2, 2, 9), (k, got.dtype, got.shape)
        np.testing.assert_array_equal(got, r[k].cpu().numpy().astype(np.float32))
    eng.close()


def test_training_run_dumps_losses_and_parameter_sample(tmp_path):
    out = tmp_path / 'out'
    d = _bench(['--gpus', '1', '--train', '--debug', '--batch', '2', '--steps', '2', '--warmup', '1', '--dump-outputs', str(out)], str(tmp_path))
    assert d['steps'] == 2 and 'training' in d['metric']
    assert sorted(os.listdir(out)) == ['losses.npy', 'params_sample.npy']
    losses, sample = np.load(out / 'losses.npy'), np.load(out / 'params_sample.npy')
    assert losses.dtype == sample.dtype == np.float32 and np.isfinite(losses).all() and np.isfinite(sample).all()
    assert losses.ndim == 1 and losses.size >= 2 and np.abs(losses).max() > 0
    assert 0 < sample.size <= 1 << 20 and np.abs(sample).max() > 0
