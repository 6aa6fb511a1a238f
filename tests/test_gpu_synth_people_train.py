"""A tower learns from rendered people: the data path of `--synth_people` (eval_run.load_data), a debug-width part detector, a small
fixed number of training steps on 32 rendered people, and the cross entropy on 16 people it has not seen."""
import os

import numpy as np
import pytest
import torch

import joint_cnn_mrf_amd  # noqa: F401
from joint_cnn_mrf_amd import main as M

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
UNIFORM = float(np.log(60 * 90))      # 8.594: the cross entropy of a uniform map against any target that sums to 1
N_STEPS = 80
BATCH = 8


def held_out_ce(eng, x, y):
    """The part detector's cross entropy on (x, y): -sum over the cells of y * log(p), the mean over images and joints, in float64 on the host."""
    tot, n = 0.0, 0
    for lo in range(0, x.shape[0], BATCH):
        xb = torch.as_tensor(np.ascontiguousarray(x[lo:lo + BATCH], np.float32), device=eng.device)
        yb = torch.as_tensor(np.ascontiguousarray(y[lo:lo + BATCH, :, :, 9:], np.float32), device=eng.device)
        p = eng.forward(xb, yb, use_sm=False)['pd_prob'].cpu().numpy().astype(np.float64)
        t = y[lo:lo + BATCH, :, :, :9].astype(np.float64)
        tot += float(-(t * np.log(np.maximum(p, 1e-300))).sum())
        n += p.shape[0] * 9
    return tot / n


def train(tmp_path, n_steps, report=None, every=4):
    """-> (the losses of every step [n_steps,4], the held-out cross entropy before and after).  report(step, ce): called every `every` steps."""
    from joint_cnn_mrf_amd.dist import Towers
    poses = np.load(os.path.join(HERE, 'golden', 'flic_train_xy.npy'))
    path = str(tmp_path / 'poses80.npy')
    np.save(path, poses[::50][:80])      # 80 poses: 64 to train on, of which --synthetic_size keeps 32, and 16 held out
    args = M.build_parser().parse_args(['--train', '--debug', '--synth_people', path, '--synthetic_size', '32', '--batch_size', str(BATCH), '--gpus', '0'])
    x_train, y_train, x_test, y_test, pairwise = M.load_data(args)
    assert x_train.shape == (32, 480, 720, 3) and x_train.dtype == np.float32 and x_test.shape[0] == 16 and y_test.shape == (16, 60, 90, 10)
    assert len(pairwise) == 90      # priors.build_pairwise_distributions of the training cells
    params, _ = M.run_params(args, pairwise)
    towers = Towers(params, args.gpus, precision=args.precision)
    try:
        tt = M.TowerTrainer(towers, params, optimizer=args.optimizer, lr=args.lr, lmbd=args.lmbd, use_sm=False, n_updates_total=10 ** 6)
        eng = towers.engines[0]
        before = held_out_ce(eng, x_test, y_test)
        rng = np.random.RandomState(args.seed)
        losses, step = [], 0
        while step < n_steps:
            order = rng.permutation(32)
            for lo in range(0, 32, BATCH):
                if step == n_steps:
                    break
                idx = order[lo:lo + BATCH]
                losses.append(tt.train_step(np.ascontiguousarray(x_train[idx]), np.ascontiguousarray(y_train[idx])).cpu().numpy().copy())
                step += 1
                if report and step % every == 0:
                    report(step, held_out_ce(eng, x_test, y_test))
        return np.stack(losses), before, held_out_ce(eng, x_test, y_test)
    finally:
        towers.close()


def test_a_tower_learns_something_that_transfers_to_unseen_people(tmp_path):
    """N_STEPS = 80 is the measured count.  On an MI355X (train() for 320 steps, batch 8, Adam 0.001, the held-out cross entropy of the part detector in
    inference mode): 8.6124 before the first step; 8.4410 after 4 steps; then a hump ABOVE log(5400) = 8.5942 -- 9.57, 11.28, 12.43, 12.88, 11.91, 10.33,
    9.59, 9.98, 9.44 after 8, 12, .., 40 steps -- while the training loss falls from 9.41 to about 2.5; and past it 7.067 after 60 steps, 6.967 after 80,
    6.838, 6.701, 6.622, 6.613, 6.637, 6.507, 6.684, 6.494, 6.494, 6.552, 6.856, 6.949 after 100, 120, .., 320.  Every count from 60 to 320 passes; 80 is
    the smallest measured count past the hump with a clear margin (1.63 under the bound).  The hump is the stretch in which the weights move fastest and
    inference still reads BatchNorm moving statistics (decay 0.9) that are mostly the initial ones -- supposed from its timing, not isolated.  The
    full-width run on all 3189 poses is tools/synth_people_train.py (profiles/synth_people_train.json: held-out loss 2.63 beside a training loss of 2.60)."""
    losses, before, after = train(tmp_path, N_STEPS)
    print('held-out cross entropy: %.4f before, %.4f after %d steps (uniform %.4f)' % (before, after, N_STEPS, UNIFORM))
    assert losses.shape == (N_STEPS, 4) and np.isfinite(losses).all()
    assert np.isfinite(after) and after < UNIFORM


def test_the_command_line_trains_on_fresh_people_and_dumps_pictures(tmp_path):
    """--train --device_data --u8_images --synth_people --synth_fresh --synth_dump end to end in a fresh process: two epochs on 8 rendered people
    (the second on a set drawn again on the device), the progress lines finite, 16 PNG files of the test set."""
    from cli_util import run_cli
    poses = np.load(os.path.join(HERE, 'golden', 'flic_train_xy.npy'))
    path = str(tmp_path / 'poses80.npy')
    np.save(path, poses[::50][:80])
    r = run_cli(['--train', '--debug', '--use_sm', '--device_data', '--u8_images', '--synth_people', path, '--synth_fresh', '--synth_dump', str(tmp_path / 'dump'),
                 '--synthetic_size', '8', '--batch_size', '4', '--n_epochs', '2', '--gpus', '0', '--model_path', str(tmp_path / 'models_ex')], str(tmp_path))
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith('Epoch ')]
    assert len(lines) == 3
    for ln in lines:
        values = [float(v) for v in ln.split()[2:] if not v.startswith(('test_', 'train_'))]
        assert len(values) == 8 and np.isfinite(values).all(), ln
    pngs = sorted(os.listdir(str(tmp_path / 'dump')))
    assert pngs == ['%05d.png' % i for i in range(16)]
    with open(str(tmp_path / 'dump' / pngs[0]), 'rb') as fh:
        assert fh.read(8) == b'\x89PNG\r\n\x1a\n'
