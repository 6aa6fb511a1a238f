"""What flow-warped heat-map pooling buys on rendered clips.  One run, modelled on tools/seq_fit_measure.py, whose training stage and
constants it shares:
  train:   the training stage of tools/synth_people_train.py (run 'plain') as a child process whose exit status is checked; it leaves its variables as
           an .npz.  --state PATH restores such a file instead and trains nothing.
  clips:   --clips (32) held-out clips of --frames (32) frames from pairs of TEST poses (the last 20 %), a second person from all poses, every odd
           clip with one scene cut in its middle, drawn by dataset.render_clip from RandomState(--seed); the joints of every frame are known.
  tower:   Engine.forward with the spatial model on every frame, the torso map the annotated one.
  pooling: per clip ONE Engine.frame_flow call on its byte frames (the whole frame as the content rectangle, motion.flow_refs(T, --flow N), search
           radius --search D) and ONE Engine.hm_flow_pool on its maps with motion.flow_weights(N): what predict_sequence(flow=N) does.
  arms:    the per-frame arg-max, the pooled arg-max, and Engine.seq_filter, Engine.seq_smooth (marginal) and Engine.seq_viterbi on the plain and on
           the pooled maps [S,T,60,90,9], all with the placeholders predict.SEQ_SIGMA / SEQ_RHO.  Mean detection rate at r = 10 % of the torso length
           (Engine.det_curve against the frames' target maps), per joint and mean; over all clips, and over the clips without a cut alone -- the
           pooling reads across a cut, which nothing gates.
Writes <outdir>/seq_flow.json.
    python tools/seq_flow_measure.py <outdir> [--state S.npz] [--epochs 40] [--minutes 10] [--clips 32] [--frames 32] [--flow 2] [--search 8] [--seed 0] [--debug]
These are rates on rendered figures, from one run; they say nothing about real video."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from seq_fit_measure import BATCH, RADIUS_PERCENT, train  # noqa: E402

MODES = ('filter', 'marginal', 'viterbi')


def measure(a, state_path):
    import torch
    import joint_cnn_mrf_amd  # noqa: F401
    from joint_cnn_mrf_amd import data, dataset, motion, predict
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
    S, T, K, N = a.clips, a.frames, 9, a.flow
    ref, weights = motion.flow_refs(T, N), motion.flow_weights(N)
    maps, pooled, argmax, targets, cut_at = [], [], [], [], []
    moved = 0.0
    tower_seconds = flow_seconds = 0.0
    for s in range(S):
        cut = T // 2 if s % 2 else None
        other = poses[int(rng.randint(0, poses.shape[0]))]
        x, _rec, _prims, xy = dataset.render_clip(eng, rng, poses[pick[s, 0]], poses[pick[s, 1]], T, other, cuts=() if cut is None else (cut,))
        y = torch.as_tensor(data.target_heat_maps(data.joint_cells(xy)), device=eng.device)
        torch.cuda.synchronize()
        t0 = time.time()
        hm, am = [], []
        for lo in range(0, T, BATCH):
            r = eng.forward(x[lo:lo + BATCH], y[lo:lo + BATCH, :, :, K:].contiguous(), use_sm=True, want_prob=True)
            hm.append(r['sm_prob'])
            am.append(r['sm_coords'])
        hm = torch.cat(hm).contiguous()
        torch.cuda.synchronize()
        t1 = time.time()
        flow = eng.frame_flow(x, (0, 0, x.shape[1], x.shape[2]), ref, search=a.search)['flow']
        pooled.append(eng.hm_flow_pool(hm, flow, weights))
        torch.cuda.synchronize()
        t2 = time.time()
        tower_seconds, flow_seconds = tower_seconds + t1 - t0, flow_seconds + t2 - t1
        moved += float((flow != 0).any(dim=-1).float().mean())
        maps.append(hm)
        argmax.append(torch.cat(am))
        targets.append(y)
        cut_at.append(cut)
    hm, hp = torch.stack(maps).contiguous(), torch.stack(pooled).contiguous()      # [S,T,60,90,9] each
    names = list(predict.JOINT_NAMES[:K])
    whole = [s for s in range(S) if cut_at[s] is None]

    def rate_of(coords, clips):      # int32 [S,T,2,K] -> percent per joint at r = 10 over the named clips
        if not clips:
            return None
        dc = DetCurve(eng, radii=[RADIUS_PERCENT])
        for s in clips:      # a clip at a time: the batches the curves are used with elsewhere
            dc.update(coords[s].contiguous(), targets[s])
        per = dc.rates()[:, 0]
        return dict({n: float(v) for n, v in zip(names, per)}, mean=float(per.mean()))

    def rate(coords):
        coords = coords.reshape(S, T, 2, K)
        return {'all_clips': rate_of(coords, list(range(S))), 'clips_without_cut': rate_of(coords, whole)}

    def arms(m):
        sigma, rho = predict.SEQ_SIGMA, predict.SEQ_RHO
        return {'argmax': rate(eng.argmax_coords(m.view(S * T, *m.shape[2:]))), 'filter': rate(eng.seq_filter(m, sigma, rho)['coords']),
                'marginal': rate(eng.seq_smooth(m, sigma, rho, want_smoothed=False)['coords']), 'viterbi': rate(eng.seq_viterbi(m, sigma, rho)['path'])}

    doc = {'note': 'detection rates (percent) at r = 10 on rendered clips, one run; they say nothing about real video',
           'clips': S, 'frames': T, 'clips_with_a_cut': S - len(whole), 'seed': a.seed, 'debug': bool(a.debug), 'joint_names': names,
           'flow': N, 'search': a.search, 'weights': weights.tolist(), 'sigma': predict.SEQ_SIGMA, 'rho': predict.SEQ_RHO,
           'tower_seconds': tower_seconds, 'flow_and_pool_seconds': flow_seconds, 'share_of_cells_with_a_nonzero_flow': moved / S,
           'tower_argmax': rate(torch.stack(argmax)), 'plain': arms(hm), 'pooled': arms(hp)}
    torch.cuda.synchronize()
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
    ap.add_argument('--flow', type=int, default=2, help='the neighbouring frames on either side, 1..4')
    ap.add_argument('--search', type=int, default=8, help='the search radius of Engine.frame_flow, 1..16 pixels')
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--poses', default=os.path.join(ROOT, 'tests', 'golden', 'flic_train_xy.npy'))
    ap.add_argument('--debug', action='store_true', help='the quarter-width tower (a rehearsal)')
    a = ap.parse_args()
    if a.clips < 1 or a.frames < 2 or not 1 <= a.flow <= 4 or not 1 <= a.search <= 16:
        sys.exit('--clips >= 1, --frames >= 2, --flow in 1..4 and --search in 1..16 are expected')
    os.makedirs(a.outdir, exist_ok=True)
    state, trained = (a.state, None) if a.state else train(a)      # the child process ends before this one opens the device
    doc = measure(a, state)
    if trained is not None:
        doc['training'] = {k: trained[k] for k in ('n_train', 'epochs', 'steps', 'train_seconds', 'final_train_loss', 'final_test_loss', 'test_dr_lwri_r10')}
        os.remove(state)
        os.remove(os.path.join(a.outdir, 'train_plain.json'))
    else:
        doc['training'] = {'restored': os.path.basename(a.state)}
    print('%-8s tower arg-max %.2f' % ('', doc['tower_argmax']['all_clips']['mean']), flush=True)
    for k in ('plain', 'pooled'):
        print('%-8s arg-max %.2f  filter %.2f  marginal %.2f  viterbi %.2f' % ((k,) + tuple(doc[k][m]['all_clips']['mean'] for m in ('argmax',) + MODES)), flush=True)
    with open(os.path.join(a.outdir, 'seq_flow.json'), 'w') as fh:
        json.dump(doc, fh, indent=1)
    print('wrote %s' % os.path.join(a.outdir, 'seq_flow.json'))


if __name__ == '__main__':
    main()
