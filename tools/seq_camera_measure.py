"""What following the camera buys on rendered clips.  One run, the set-up of tools/seq_fit_measure.py:
  train:   its training stage (a child process; --state PATH restores an .npz instead and trains nothing).
  clips:   --clips (16) held-out clips of --frames (16) frames from pairs of TEST poses, a second person from all poses, no cuts, drawn by
           dataset.render_clip_pan from RandomState(--seed) at every pan speed of --speeds (0, 4 and 12 fitted pixels a frame): the camera moves by
           `speed` along a direction drawn per clip that turns round where the canvas ends.  The same scenes at every speed.
  tower:   Engine.forward with the spatial model on every frame, the torso map the annotated one.
  tracks:  on the spatial model's maps: the per-frame arg-max, Engine.seq_filter and Engine.seq_viterbi with the placeholders SEQ_SIGMA / SEQ_RHO,
           without a shift and with shift = motion.camera_shifts(Engine.frame_shift(...)['disp']) at the default search radius.
  rates:   the detection rate at r = 10 % of the torso length (Engine.det_curve against the frames' target maps), mean over the joints, the joints
           of frames in which a joint left the crop included as the target maps have them; and the share of frames whose estimated displacement is
           the true one.
Writes <outdir>/seq_camera.json.
    python tools/seq_camera_measure.py <outdir> [--state S.npz] [--epochs 40] [--minutes 10] [--clips 16] [--frames 16] [--speeds 0 4 12] [--seed 0] [--debug]
These are rates on rendered figures, whose sensor noise pans with the crop; they say nothing about real video."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
BATCH = 16
RADIUS_PERCENT = 10.0
MARGIN = (48, 72)


def pan_path(rng, T, speed, margin):
    """int [T,2]: a pan of `speed` pixels a frame (rounded per axis) along a direction drawn from rng, reflected where the crop would leave the canvas."""
    a = rng.uniform(0.0, 2.0 * np.pi)
    step = np.array([int(round(speed * np.sin(a))), int(round(speed * np.cos(a)))])
    pan, at = np.zeros((T, 2), np.int64), np.array(margin)
    for t in range(1, T):
        for ax in range(2):
            if not 0 <= at[ax] + step[ax] <= 2 * margin[ax]:
                step[ax] = -step[ax]
        pan[t] = step
        at = at + step
    return pan


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
    S, T, K = a.clips, a.frames, 9
    doc = {'note': 'mean detection rates (percent) at r = 10 on rendered clips whose sensor noise pans with the crop, one run; they say nothing about real video',
           'clips': S, 'frames': T, 'seed': a.seed, 'debug': bool(a.debug), 'margin': list(MARGIN), 'search': predict.SEQ_CAMERA_SEARCH,
           'sigma': predict.SEQ_SIGMA, 'rho': predict.SEQ_RHO, 'speeds': {}}
    for speed in a.speeds:
        rng = np.random.RandomState(a.seed)      # the same scenes at every speed
        pick = rng.permutation(test)[:2 * S].reshape(S, 2)
        dc = {k: DetCurve(eng, radii=[RADIUS_PERCENT]) for k in ('argmax', 'filter', 'viterbi', 'filter_camera', 'viterbi_camera')}
        exact = 0
        for s in range(S):
            other = poses[int(rng.randint(0, poses.shape[0]))]
            pan = pan_path(np.random.RandomState(a.seed * 1000 + s), T, speed, MARGIN)
            x, xy, _inside, true = dataset.render_clip_pan(eng, rng, poses[pick[s, 0]], poses[pick[s, 1]], T, pan, MARGIN, other)
            y = torch.as_tensor(data.target_heat_maps(data.joint_cells(xy)), device=eng.device)
            hm, am = [], []
            for lo in range(0, T, BATCH):
                r = eng.forward(x[lo:lo + BATCH], y[lo:lo + BATCH, :, :, K:].contiguous(), use_sm=True, want_prob=True)
                hm.append(r['sm_prob'])
                am.append(r['sm_coords'])
            hm = torch.cat(hm).contiguous()
            disp = eng.frame_shift(x, (0, 0, 480, 720))['disp'].cpu().numpy()
            exact += int((disp == true).all(axis=1).sum())
            shift, _ = predict.camera_shifts(disp)
            dc['argmax'].update(torch.cat(am).contiguous(), y)
            dc['filter'].update(eng.seq_filter(hm, predict.SEQ_SIGMA, predict.SEQ_RHO)['coords'], y)
            dc['viterbi'].update(eng.seq_viterbi(hm, predict.SEQ_SIGMA, predict.SEQ_RHO)['path'], y)
            dc['filter_camera'].update(eng.seq_filter(hm, predict.SEQ_SIGMA, predict.SEQ_RHO, shift=shift)['coords'], y)
            dc['viterbi_camera'].update(eng.seq_viterbi(hm, predict.SEQ_SIGMA, predict.SEQ_RHO, shift=shift)['path'], y)
        doc['speeds'][str(speed)] = dict({k: float(v.rates()[:, 0].mean()) for k, v in dc.items()}, disp_exact_share=exact / float(S * T))
    eng.close()
    return doc


def main():
    from seq_fit_measure import train
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('outdir')
    ap.add_argument('--state', default=None, help='an .npz of variables (what the training stage of tools/synth_people_train.py leaves): restore it, train nothing')
    ap.add_argument('--epochs', type=int, default=40)
    ap.add_argument('--minutes', type=float, default=10.0)
    ap.add_argument('--clips', type=int, default=16)
    ap.add_argument('--frames', type=int, default=16)
    ap.add_argument('--speeds', type=int, nargs='+', default=[0, 4, 12])
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--poses', default=os.path.join(ROOT, 'tests', 'golden', 'flic_train_xy.npy'))
    ap.add_argument('--debug', action='store_true', help='the quarter-width tower (a rehearsal)')
    a = ap.parse_args()
    if a.clips < 1 or a.frames < 2 or min(a.speeds) < 0 or max(a.speeds) > 35:
        sys.exit('--clips >= 1, --frames >= 2 and --speeds in 0..35 (the reach of the default search) are expected')
    os.makedirs(a.outdir, exist_ok=True)
    state, trained = (a.state, None) if a.state else train(a)      # the child process ends before this one opens the device
    doc = measure(a, state)
    if trained is not None:
        doc['training'] = {k: trained[k] for k in ('n_train', 'epochs', 'steps', 'train_seconds', 'final_train_loss', 'final_test_loss', 'test_dr_lwri_r10')}
        os.remove(state)
        os.remove(os.path.join(a.outdir, 'train_plain.json'))
    else:
        doc['training'] = {'restored': os.path.basename(a.state)}
    for speed, row in doc['speeds'].items():
        print('%3s px/frame: %s' % (speed, '  '.join('%s %.2f' % kv for kv in row.items())), flush=True)
    with open(os.path.join(a.outdir, 'seq_camera.json'), 'w') as fh:
        json.dump(doc, fh, indent=1)
    print('wrote %s' % os.path.join(a.outdir, 'seq_camera.json'))


if __name__ == '__main__':
    main()
