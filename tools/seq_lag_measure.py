"""What a lag buys on rendered clips: the set-up of tools/seq_fit_measure.py -- the same tower training (a child process, or --state),
the same --clips (32) held-out clips of --frames (32) frames from RandomState(--seed), every odd clip with a scene cut, the placeholders
predict.SEQ_SIGMA / SEQ_RHO -- and, beside the per-frame arg-max, Engine.seq_filter, Engine.seq_smooth (marginal) and Engine.seq_viterbi, one row
per lag in --lags (1 2 4 8 16): Engine.seq_smooth_lag over each clip, flushed.  Detection rate at r = 10 % of the torso length, per joint and mean.
Writes <outdir>/seq_lag.json.
    python tools/seq_lag_measure.py <outdir> [--state S.npz] [--epochs 40] [--minutes 10] [--clips 32] [--frames 32] [--lags 1 2 4 8 16] [--seed 0] [--debug]
These are rates on rendered figures, one run; they say nothing about real video."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
from seq_fit_measure import BATCH, RADIUS_PERCENT, train  # noqa: E402


def measure(a, state_path):
    import torch
    import joint_cnn_mrf_amd  # noqa: F401
    from joint_cnn_mrf_amd import data, dataset, predict
    from joint_cnn_mrf_amd import main as M
    from joint_cnn_mrf_amd.engine import Engine
    from joint_cnn_mrf_amd.eval_run import people_split
    from joint_cnn_mrf_amd.evaluation import DetCurve
    args = M.build_parser().parse_args(['--use_sm', '--u8_images', '--synth_people', a.poses, '--batch_size', str(BATCH), '--gpus', '0', '--seed', '0', '--restore',
                                        '--restore_path', state_path] + (['--debug'] if a.debug else []))
    params, _ = M.run_params(args, None)
    eng = Engine(device=0, precision=args.precision, n_joints=9).load_params(params)
    poses = np.asarray(np.load(a.poses), np.float64)
    test = people_split(poses.shape[0])[1]
    if test.shape[0] < 2 * a.clips:
        sys.exit('%d test poses cannot make %d clips of two poses each' % (test.shape[0], a.clips))
    rng = np.random.RandomState(a.seed)      # the draws of seq_fit_measure.measure, in its order: the same clips
    pick = rng.permutation(test)[:2 * a.clips].reshape(a.clips, 2)
    S, T, K = a.clips, a.frames, 9
    maps, argmax, targets = [], [], []
    for s in range(S):
        cut = T // 2 if s % 2 else None
        other = poses[int(rng.randint(0, poses.shape[0]))]
        x, _rec, _prims, xy = dataset.render_clip(eng, rng, poses[pick[s, 0]], poses[pick[s, 1]], T, other, cuts=() if cut is None else (cut,))
        y = torch.as_tensor(data.target_heat_maps(data.joint_cells(xy)), device=eng.device)
        hm, am = [], []
        for lo in range(0, T, BATCH):
            r = eng.forward(x[lo:lo + BATCH], y[lo:lo + BATCH, :, :, K:].contiguous(), use_sm=True, want_prob=True)
            hm.append(r['sm_prob'])
            am.append(r['sm_coords'])
        maps.append(torch.cat(hm))
        argmax.append(torch.cat(am))
        targets.append(y)
    hm = torch.stack(maps).contiguous()                     # [S,T,60,90,9]
    names = list(predict.JOINT_NAMES[:K])

    def rate(coords):      # int32 [S,T,2,K] -> percent per joint at r = 10
        dc = DetCurve(eng, radii=[RADIUS_PERCENT])
        coords = coords.reshape(S, T, 2, K)
        for s in range(S):
            dc.update(coords[s].contiguous(), targets[s])
        per = dc.rates()[:, 0]
        return dict({n: float(v) for n, v in zip(names, per)}, mean=float(per.mean()))

    sigma, rho = predict.SEQ_SIGMA, predict.SEQ_RHO
    doc = {'note': 'detection rates (percent) at r = 10 on rendered clips, one run; they say nothing about real video',
           'clips': S, 'frames': T, 'clips_with_a_cut': S // 2, 'seed': a.seed, 'debug': bool(a.debug), 'joint_names': names, 'sigma': sigma, 'rho': rho,
           'argmax': rate(torch.stack(argmax)), 'filter': rate(eng.seq_filter(hm, sigma, rho)['coords']),
           'marginal': rate(eng.seq_smooth(hm, sigma, rho, want_smoothed=False)['coords']), 'viterbi': rate(eng.seq_viterbi(hm, sigma, rho)['path']),
           'lag': {str(L): rate(eng.seq_smooth_lag(hm, sigma, rho, L, flush=True)['coords']) for L in a.lags}}
    eng.close()
    return doc


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('outdir')
    ap.add_argument('--state', default=None, help='an .npz of variables (what the training stage of tools/synth_people_train.py leaves): restore it, train nothing')
    ap.add_argument('--epochs', type=int, default=40)
    ap.add_argument('--minutes', type=float, default=10.0)
    ap.add_argument('--clips', type=int, default=32)
    ap.add_argument('--frames', type=int, default=32)
    ap.add_argument('--lags', type=int, nargs='+', default=[1, 2, 4, 8, 16])
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--poses', default=os.path.join(ROOT, 'tests', 'golden', 'flic_train_xy.npy'))
    ap.add_argument('--debug', action='store_true', help='the quarter-width tower (a rehearsal)')
    a = ap.parse_args()
    if a.clips < 1 or a.frames < 2 or min(a.lags) < 1:
        sys.exit('--clips >= 1, --frames >= 2 and --lags >= 1 are expected')
    os.makedirs(a.outdir, exist_ok=True)
    state, trained = (a.state, None) if a.state else train(a)      # the child process ends before this one opens the device
    doc = measure(a, state)
    if trained is not None:
        doc['training'] = {k: trained[k] for k in ('n_train', 'epochs', 'steps', 'train_seconds', 'final_train_loss', 'final_test_loss', 'test_dr_lwri_r10')}
        os.remove(state)
        os.remove(os.path.join(a.outdir, 'train_plain.json'))
    else:
        doc['training'] = {'restored': os.path.basename(a.state)}
    for k in ('argmax', 'filter', 'marginal', 'viterbi'):
        print('%-10s mean %.2f' % (k, doc[k]['mean']), flush=True)
    for L in a.lags:
        print('lag %-6d mean %.2f' % (L, doc['lag'][str(L)]['mean']), flush=True)
    with open(os.path.join(a.outdir, 'seq_lag.json'), 'w') as fh:
        json.dump(doc, fh, indent=1)
    print('wrote %s' % os.path.join(a.outdir, 'seq_lag.json'))


if __name__ == '__main__':
    main()
