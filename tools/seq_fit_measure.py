"""What tracking buys on rendered clips, and what the fit finds.  One run:
  train:   the training stage of tools/synth_people_train.py (run 'plain': 80 % of the poses, a new set of scenes every epoch) as a child process whose
           exit status is checked; it leaves its variables as an .npz.  --state PATH restores such a file instead and trains nothing.
  clips:   --clips (32) held-out clips of --frames (32) frames from pairs of TEST poses (the last 20 %), a second person from all poses, every odd
           clip with one scene cut in its middle, drawn by dataset.render_clip from RandomState(--seed); the joints of every frame are known.
  tower:   Engine.forward with the spatial model on every frame, the torso map the annotated one (as the evaluation of the training tool).
  tracks:  on the spatial model's maps [S,T,60,90,9]: the per-frame arg-max, Engine.seq_filter, Engine.seq_smooth (marginal) and Engine.seq_viterbi
           with the placeholders predict.SEQ_SIGMA / SEQ_RHO and with the values predict.seq_fit finds on these maps (--iters EM iterations, radius 16,
           from the placeholders).  Detection rate at r = 10 % of the torso length (Engine.det_curve against the frames' target maps), per joint and mean.
  truth:   beside the fitted sigma per joint and rho, the values computed directly from the clips' true joint cells: sigma_k from the mean squared
           cell displacement over the transitions without a cut through the M-step's own moment equation (predict.seq_sigma_of_moment), rho as the
           share of transitions that are cuts.
Writes <outdir>/seq_fit.json.
    python tools/seq_fit_measure.py <outdir> [--state S.npz] [--epochs 40] [--minutes 10] [--clips 32] [--frames 32] [--iters 10] [--seed 0] [--debug]
These are rates on rendered figures; they say nothing about real video."""
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
RADIUS_PERCENT = 10.0
FIT_RADIUS = 16


def train(a):
    cmd = [sys.executable, os.path.join(ROOT, 'tools', 'synth_people_train.py'), a.outdir, '--stage', 'train', '--run', 'plain', '--epochs', str(a.epochs),
           '--minutes', str(a.minutes), '--poses', a.poses] + (['--debug'] if a.debug else [])
    print('+ ' + ' '.join(cmd), flush=True)
    rc = subprocess.call(cmd)
    if rc != 0:
        sys.exit('the training stage ended with status %d; stopping' % rc)
    return os.path.join(a.outdir, 'state_plain.npz'), json.load(open(os.path.join(a.outdir, 'train_plain.json')))


def true_motion(cells, cut_at):
    """cells int64 [S,T,9,2] (row, col), cut_at: per clip the frame that starts a new scene or None -> (sigma [9], rho, transitions used)."""
    from joint_cnn_mrf_amd import predict
    S, T = cells.shape[:2]
    keep = np.ones((S, T - 1), bool)
    for s, c in enumerate(cut_at):
        if c is not None:
            keep[s, c - 1] = False
    d = (cells[:, 1:] - cells[:, :-1]).astype(np.float64)[keep]      # [n,9,2]
    moment = (d ** 2).sum(axis=2).mean(axis=0) / 2.0                 # per axis, as the M-step's squared / (2 moved)
    sigma = [predict.seq_sigma_of_moment(m, FIT_RADIUS)[0] for m in moment]
    return np.array(sigma), float((~keep).sum()) / keep.size, int(keep.sum())


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
    rng = np.random.RandomState(a.seed)
    pick = rng.permutation(test)[:2 * a.clips].reshape(a.clips, 2)
    S, T, K = a.clips, a.frames, 9
    maps, argmax, targets, cells, cut_at = [], [], [], [], []
    t0 = time.time()
    for s in range(S):
        cut = T // 2 if s % 2 else None
        other = poses[int(rng.randint(0, poses.shape[0]))]
        x, _rec, _prims, xy = dataset.render_clip(eng, rng, poses[pick[s, 0]], poses[pick[s, 1]], T, other, cuts=() if cut is None else (cut,))
        c = data.joint_cells(xy)
        y = torch.as_tensor(data.target_heat_maps(c), device=eng.device)
        hm, am = [], []
        for lo in range(0, T, BATCH):
            r = eng.forward(x[lo:lo + BATCH], y[lo:lo + BATCH, :, :, K:].contiguous(), use_sm=True, want_prob=True)
            hm.append(r['sm_prob'])
            am.append(r['sm_coords'])
        maps.append(torch.cat(hm))
        argmax.append(torch.cat(am))
        targets.append(y)
        cells.append(c[:, :K])
        cut_at.append(cut)
    hm = torch.stack(maps).contiguous()                     # [S,T,60,90,9]
    torch.cuda.synchronize()
    tower_seconds = time.time() - t0
    names = list(predict.JOINT_NAMES[:K])

    def rate(coords):      # int32 [S,T,2,K] or [S*T,2,K] -> percent per joint at r = 10
        dc = DetCurve(eng, radii=[RADIUS_PERCENT])
        coords = coords.reshape(S, T, 2, K)
        for s in range(S):      # a clip at a time: the batches the curves are used with elsewhere
            dc.update(coords[s].contiguous(), targets[s])
        per = dc.rates()[:, 0]
        return dict({n: float(v) for n, v in zip(names, per)}, mean=float(per.mean()))

    def tracks(sigma, rho):
        return {'filter': rate(eng.seq_filter(hm, sigma, rho)['coords']),
                'marginal': rate(eng.seq_smooth(hm, sigma, rho, want_smoothed=False)['coords']),
                'viterbi': rate(eng.seq_viterbi(hm, sigma, rho)['path'])}

    t0 = time.time()
    fit = predict.seq_fit(eng, hm, predict.SEQ_SIGMA, predict.SEQ_RHO, iters=a.iters, radius=FIT_RADIUS)
    fit_seconds = time.time() - t0
    true_sigma, true_rho, n_tr = true_motion(np.stack(cells), cut_at)
    doc = {'note': 'detection rates (percent) at r = 10 on rendered clips, one run; they say nothing about real video',
           'clips': S, 'frames': T, 'clips_with_a_cut': int(sum(c is not None for c in cut_at)), 'seed': a.seed, 'debug': bool(a.debug), 'joint_names': names,
           'tower_seconds': tower_seconds, 'fit_seconds': fit_seconds,
           'argmax': rate(torch.stack(argmax)),
           'placeholders': dict(tracks(predict.SEQ_SIGMA, predict.SEQ_RHO), sigma=predict.SEQ_SIGMA, rho=predict.SEQ_RHO),
           'fitted': dict(tracks(fit['sigma'], fit['rho']), sigma=fit['sigma'].tolist(), rho=fit['rho'], loglik=fit['loglik'].tolist(),
                          clamped=fit['clamped'].tolist(), iters=a.iters, radius=FIT_RADIUS),
           'true_cells': {'sigma': true_sigma.tolist(), 'rho': true_rho, 'transitions_without_cut': n_tr,
                          'how': 'sigma_k: seq_sigma_of_moment(mean squared cell displacement / 2, radius 16) over the transitions without a cut; rho: cuts / transitions'}}
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
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--poses', default=os.path.join(ROOT, 'tests', 'golden', 'flic_train_xy.npy'))
    ap.add_argument('--debug', action='store_true', help='the quarter-width tower (a rehearsal)')
    a = ap.parse_args()
    if a.clips < 1 or a.frames < 2:
        sys.exit('--clips >= 1 and --frames >= 2 are expected')
    os.makedirs(a.outdir, exist_ok=True)
    state, trained = (a.state, None) if a.state else train(a)      # the child process ends before this one opens the device
    doc = measure(a, state)
    if trained is not None:
        doc['training'] = {k: trained[k] for k in ('n_train', 'epochs', 'steps', 'train_seconds', 'final_train_loss', 'final_test_loss', 'test_dr_lwri_r10')}
        os.remove(state)
        os.remove(os.path.join(a.outdir, 'train_plain.json'))
    else:
        doc['training'] = {'restored': os.path.basename(a.state)}
    for k in ('argmax',):
        print('%-22s mean %.2f' % (k, doc[k]['mean']), flush=True)
    for k in ('placeholders', 'fitted'):
        print('%-22s filter %.2f  marginal %.2f  viterbi %.2f   sigma %s rho %.4g' % (k, doc[k]['filter']['mean'], doc[k]['marginal']['mean'], doc[k]['viterbi']['mean'],
                                                                                 np.round(doc[k]['sigma'], 3).tolist(), doc[k]['rho']), flush=True)
    print('true cells: sigma %s rho %.4g' % (np.round(doc['true_cells']['sigma'], 3).tolist(), doc['true_cells']['rho']), flush=True)
    with open(os.path.join(a.outdir, 'seq_fit.json'), 'w') as fh:
        json.dump(doc, fh, indent=1)
    print('wrote %s' % os.path.join(a.outdir, 'seq_fit.json'))


if __name__ == '__main__':
    main()
