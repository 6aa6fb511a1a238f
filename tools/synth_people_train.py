"""Trains on rendered people and measures on people the tower has not seen.  One run = a training stage and an evaluation stage,
each a child process of this tool whose exit status is checked; the first failure stops everything.
  train: --train --device_data --u8_images --synth_fresh --use_sm on the first 80 % of the poses (full width, fp32, batch 16, the reference's Adam
         settings: lr 0.001 with its piecewise schedule over --epochs, lmbd 0.001), a new set of scenes every epoch, until --epochs are done or --minutes
         have passed; then eval_error on the held-out set and the variables as an .npz.
  eval:  on the last 20 % of the poses, rendered from the test seed: the eval_curves detection rates at r = 1..20, every joint, part detector and
         spatial model; the same with flip_test=True; the same through multiscale.get_predictions; the mean torso_cell_dist of torso='infer'.
The run 'augm' is the same with --augm_affine, the run 'augm_aa' with --augm_affine --augm_antialias.  --keep_state leaves state_<run>.npz in
<outdir> (tools/scale_sweep_measure.py reads it).  Writes <outdir>/synth_people_train.json, one entry per run (an existing file keeps its other runs).
    python tools/synth_people_train.py <outdir> [--runs plain,augm,augm_aa] [--epochs 40] [--minutes 10] [--poses P.npy] [--limit N] [--debug] [--revision R]
These are rates on rendered figures and say nothing about FLIC."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
BATCH = 16


def cli(a, train, augm):
    v = ['--use_sm', '--u8_images', '--synth_people', a.poses, '--batch_size', str(BATCH), '--gpus', '0', '--seed', '0'] + (['--debug'] if a.debug else [])
    if train:
        v += ['--train', '--device_data', '--synth_fresh', '--optimizer', 'adam', '--lr', '0.001', '--lmbd', '0.001', '--n_epochs', str(a.epochs)]
        v += {'augm': ['--augm_affine'], 'augm_aa': ['--augm_affine', '--augm_antialias']}.get(augm, [])
    else:
        v += ['--restore', '--restore_path', os.path.join(a.outdir, 'state_%s.npz' % a.run)]
    return v


def stage_train(a):
    import torch
    from joint_cnn_mrf_amd import checkpoint, evaluation
    from joint_cnn_mrf_amd import main as M
    from joint_cnn_mrf_amd.dataset import DeviceDataset
    from joint_cnn_mrf_amd.dist import Towers
    augm = a.run if a.run in ('augm', 'augm_aa') else None
    args = M.build_parser().parse_args(cli(a, True, augm))
    t0 = time.time()
    people = {}
    x_train, y_train, x_test, y_test, pairwise = M.load_data(args, people)
    n_train = x_train.shape[0]
    params, _ = M.run_params(args, pairwise)
    towers = Towers(params, args.gpus, precision=args.precision)
    eng = towers.engines[0]
    kw = dict(augment_rng=np.random.RandomState(args.seed + 1), augment_kind='affine', affine_kw={'antialias': True} if augm == 'augm_aa' else None) if augm else {}
    tt = M.TowerTrainer(towers, params, optimizer=args.optimizer, lr=args.lr, lmbd=args.lmbd, use_sm=True, n_updates_total=args.n_epochs * n_train // BATCH, **kw)
    ds = DeviceDataset(x_train, y_train, device=eng.device, reserve_bytes=(2 << 30) if a.debug else (64 << 30), image_dtype='uint8', cells=people['cells_train'])
    del x_train
    rng = np.random.RandomState(args.seed)
    t_train, epochs, history = time.time(), 0, []
    for epoch in range(1, args.n_epochs + 1):
        if epoch > 1:
            ds.rerender_people(eng, people['poses'], people['train_idx'], M.people_seed(args, epoch))
        acc, n = torch.zeros(4, dtype=torch.float64, device=eng.device), 0
        for idx in ds.epoch_indices(rng, BATCH, shuffle=True):
            acc += tt.train_step_indexed(ds, idx).to(torch.float64)
            n += 1
        mean = (acc / n).cpu().numpy()
        if not np.isfinite(mean).all():
            raise SystemExit('epoch %d: the training losses are not finite: %s' % (epoch, mean))
        epochs = epoch
        history.append([float(v) for v in mean[:3]])
        print('epoch %d  train loss_tower %.4f loss_pd %.4f loss_sm %.4f  (%.0f s)' % (epoch, mean[0], mean[1], mean[2], time.time() - t_train), flush=True)
        if time.time() - t_train > a.minutes * 60:
            break
    train_seconds = time.time() - t_train
    te = [float(v) for v in evaluation.eval_error(x_test, y_test, eng, BATCH, True, [2], 10)]
    state = checkpoint.session_state(tt.trainers[0], params)
    np.savez(os.path.join(a.outdir, 'state_%s.npz' % a.run), **state)
    doc = {'flags': cli(a, True, augm), 'n_train': int(n_train), 'n_test': int(x_test.shape[0]), 'epochs_planned': int(args.n_epochs), 'epochs': int(epochs),
           'steps': int(epochs * (n_train // BATCH)), 'train_seconds': train_seconds, 'wall_seconds': time.time() - t0,
           'final_train_loss': {'pd': history[-1][1], 'sm': history[-1][2]}, 'train_loss_by_epoch_pd_sm': [h[1:] for h in history],
           'final_test_loss': {'pd': te[0], 'sm': te[1]}, 'test_dr_lwri_r10': {'pd': te[2], 'sm': te[3]}}
    with open(os.path.join(a.outdir, 'train_%s.json' % a.run), 'w') as fh:
        json.dump(doc, fh)
    towers.close()


def stage_eval(a):
    import torch
    from joint_cnn_mrf_amd import evaluation, multiscale
    from joint_cnn_mrf_amd import main as M
    from joint_cnn_mrf_amd.engine import Engine
    from joint_cnn_mrf_amd.eval_run import det_curves_of_predictions
    args = M.build_parser().parse_args(cli(a, False, None))
    _xt, _yt, x_test, y_test, _ = M.load_data(args)
    params, _ = M.run_params(args, None)
    eng = Engine(device=0, precision=args.precision, n_joints=9).load_params(params)
    names = [str(n) for n in M.joint_names[:9]]

    def curves(pair):
        return {'pd': pair[0].as_dict(names), 'sm': pair[1].as_dict(names)}
    doc = {'n_images': int(x_test.shape[0])}
    doc['plain'] = curves(evaluation.eval_curves(x_test, y_test, eng, BATCH, True))
    doc['flip_test'] = curves(evaluation.eval_curves(x_test, y_test, eng, BATCH, True, flip_test=True))
    xf = x_test.astype(np.float32) / np.float32(255)
    pd, sm = multiscale.get_predictions(eng, xf, np.asarray(y_test), use_sm=True)[:2]
    doc['multiscale'] = curves(det_curves_of_predictions(eng, pd, sm, y_test))
    cells = []
    for lo in range(0, xf.shape[0], BATCH):
        r = eng.forward(torch.as_tensor(xf[lo:lo + BATCH], device=eng.device), 'infer', use_sm=True)
        cells.append(r['torso_cell'].cpu().numpy())
    got = np.concatenate(cells).astype(np.float64)
    ann = np.asarray(y_test)[:, :, :, 9].reshape(len(y_test), -1).argmax(axis=1)
    doc['infer_torso'] = {'torso_cell_dist_mean': float(np.sqrt((got[:, 0] - ann // 90) ** 2 + (got[:, 1] - ann % 90) ** 2).mean())}
    for k in ('plain', 'flip_test', 'multiscale'):
        print('%s: lwri r=10 pd %.2f sm %.2f; all joints r=10 pd %.2f sm %.2f' % (
            k, doc[k]['pd']['lwri'][9], doc[k]['sm']['lwri'][9], np.mean([doc[k]['pd'][n][9] for n in names]), np.mean([doc[k]['sm'][n][9] for n in names])), flush=True)
    print('infer_torso: %s' % doc['infer_torso'], flush=True)
    with open(os.path.join(a.outdir, 'eval_%s.json' % a.run), 'w') as fh:
        json.dump(doc, fh)
    eng.close()


def revision():
    try:
        return subprocess.check_output(['git', 'rev-parse', 'HEAD'], cwd=ROOT, stderr=subprocess.DEVNULL, text=True).strip()
    except Exception:
        return 'unknown (not a git checkout)'


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('outdir')
    ap.add_argument('--runs', default='plain,augm')
    ap.add_argument('--epochs', type=int, default=40)
    ap.add_argument('--minutes', type=float, default=10.0)
    ap.add_argument('--poses', default=os.path.join(ROOT, 'tests', 'golden', 'flic_train_xy.npy'))
    ap.add_argument('--limit', type=int, default=0, help='use the first N poses only (a rehearsal)')
    ap.add_argument('--debug', action='store_true', help='the quarter-width tower (a rehearsal)')
    ap.add_argument('--revision', default=None)
    ap.add_argument('--keep_state', action='store_true', help='leave state_<run>.npz, the trained variables, in <outdir>')
    ap.add_argument('--stage', default=None, choices=['train', 'eval'])
    ap.add_argument('--run', default=None)
    a = ap.parse_args()
    os.makedirs(a.outdir, exist_ok=True)
    if a.stage:
        import joint_cnn_mrf_amd  # noqa: F401
        return stage_train(a) if a.stage == 'train' else stage_eval(a)
    if a.limit:
        sub = os.path.join(a.outdir, 'poses_%d.npy' % a.limit)
        np.save(sub, np.load(a.poses)[:a.limit])
        a.poses = sub
    path = os.path.join(a.outdir, 'synth_people_train.json')
    doc = json.load(open(path)) if os.path.exists(path) else {}
    doc.update(note='detection rates (percent) on rendered figures; they say nothing about FLIC', revision=a.revision or revision(), batch=BATCH,
               poses=os.path.basename(a.poses), debug=bool(a.debug))
    for run in a.runs.split(','):
        for stage in ('train', 'eval'):
            cmd = [sys.executable, os.path.abspath(__file__), a.outdir, '--stage', stage, '--run', run, '--epochs', str(a.epochs), '--minutes', str(a.minutes),
                   '--poses', a.poses] + (['--debug'] if a.debug else [])
            print('+ %s %s' % (run, stage), flush=True)
            rc = subprocess.call(cmd)
            if rc != 0:
                sys.exit('%s %s ended with status %d; stopping' % (run, stage, rc))
        doc[run] = dict(json.load(open(os.path.join(a.outdir, 'train_%s.json' % run))), **json.load(open(os.path.join(a.outdir, 'eval_%s.json' % run))))
        with open(path, 'w') as fh:
            json.dump(doc, fh, indent=1)
        if not a.keep_state:
            os.remove(os.path.join(a.outdir, 'state_%s.npz' % run))
    print('wrote %s' % path)


if __name__ == '__main__':
    main()
