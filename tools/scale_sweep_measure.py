"""Measures what the affine augmentation buys in robustness to person scale, on rendered people: the two trainings of
tools/synth_people_train.py -- 'plain', and 'augm_aa' = --augm_affine --augm_antialias -- each followed by a sweep of the held-out set through
evaluation.eval_curves_affine at the scales 0.5, 0.75, 1.0 and 1.5 (antialiased sample, about the centre, pad 0), with the joint cells of the
rendered set.  Every stage is a child process whose exit status is checked; the first failure stops everything.
Writes <outdir>/scale_sweep.json: per run and scale the number of images counted (those none of whose joints leaves the frame) and the detection-rate
curves of the part detector and the spatial model, r = 1..20, every joint; the trainings' own figures go to <outdir>/synth_people_train.json.
    python tools/scale_sweep_measure.py <outdir> [--runs plain,augm_aa] [--epochs 40] [--minutes 10] [--poses P.npy] [--limit N] [--debug]
These are rates on rendered figures and say nothing about FLIC."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
SCALES = (0.5, 0.75, 1.0, 1.5)


def stage_sweep(a):
    import joint_cnn_mrf_amd  # noqa: F401
    import synth_people_train as T
    from joint_cnn_mrf_amd import evaluation
    from joint_cnn_mrf_amd import main as M
    from joint_cnn_mrf_amd.engine import Engine
    args = M.build_parser().parse_args(T.cli(a, False, None))
    people = {}
    _xt, _yt, x_test, _y_test, _ = M.load_data(args, people)
    params, _ = M.run_params(args, None)
    eng = Engine(device=0, precision=args.precision, n_joints=9).load_params(params)
    names = [str(n) for n in M.joint_names[:9]]
    curves = evaluation.eval_curves_affine(x_test, people['cells_test'], eng, T.BATCH, SCALES, use_sm=True)
    doc = {'n_images': int(x_test.shape[0]), 'scales': list(SCALES), 'counted': [int(curves[s][0].n_images) for s in SCALES], 'antialias': True, 'pd': {}, 'sm': {}}
    for s in SCALES:
        for key, c in zip(('pd', 'sm'), curves[s]):
            doc[key][str(s)] = {n: v for n, v in c.as_dict(names).items() if n in names} if c.n_images else None
        if curves[s][0].n_images:
            print('scale %g: %d images counted; lwri r=10 pd %.2f sm %.2f; all joints r=10 pd %.2f sm %.2f' % (
                s, curves[s][0].n_images, doc['pd'][str(s)]['lwri'][9], doc['sm'][str(s)]['lwri'][9],
                np.mean([doc['pd'][str(s)][n][9] for n in names]), np.mean([doc['sm'][str(s)][n][9] for n in names])), flush=True)
    with open(os.path.join(a.outdir, 'sweep_%s.json' % a.run), 'w') as fh:
        json.dump(doc, fh)
    eng.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('outdir')
    ap.add_argument('--runs', default='plain,augm_aa')
    ap.add_argument('--epochs', type=int, default=40)
    ap.add_argument('--minutes', type=float, default=10.0)
    ap.add_argument('--poses', default=os.path.join(ROOT, 'tests', 'golden', 'flic_train_xy.npy'))
    ap.add_argument('--limit', type=int, default=0, help='use the first N poses only (a rehearsal)')
    ap.add_argument('--debug', action='store_true', help='the quarter-width tower (a rehearsal)')
    ap.add_argument('--stage', default=None, choices=['sweep'])
    ap.add_argument('--run', default=None)
    a = ap.parse_args()
    os.makedirs(a.outdir, exist_ok=True)
    if a.stage:
        return stage_sweep(a)
    if a.limit:      # (the training tool is given the same file, so both stages see the same poses)
        sub = os.path.join(a.outdir, 'poses_%d.npy' % a.limit)
        np.save(sub, np.load(a.poses)[:a.limit])
        a.poses = sub
    path = os.path.join(a.outdir, 'scale_sweep.json')
    doc = json.load(open(path)) if os.path.exists(path) else {}
    doc.update(note='detection rates (percent) on rendered figures shown at other scales; they say nothing about FLIC', poses=os.path.basename(a.poses),
               debug=bool(a.debug), epochs_planned=a.epochs)
    common = ['--poses', a.poses] + (['--debug'] if a.debug else [])
    for run in a.runs.split(','):
        train = [sys.executable, os.path.join(ROOT, 'tools', 'synth_people_train.py'), a.outdir, '--runs', run, '--keep_state', '--epochs', str(a.epochs),
                 '--minutes', str(a.minutes)] + common
        sweep = [sys.executable, os.path.abspath(__file__), a.outdir, '--stage', 'sweep', '--run', run] + common
        for name, cmd in (('train', train), ('sweep', sweep)):
            print('+ %s %s' % (run, name), flush=True)
            rc = subprocess.call(cmd)
            if rc != 0:
                sys.exit('%s %s ended with status %d; stopping' % (run, name, rc))
        doc[run] = json.load(open(os.path.join(a.outdir, 'sweep_%s.json' % run)))
        with open(path, 'w') as fh:
            json.dump(doc, fh, indent=1)
        os.remove(os.path.join(a.outdir, 'state_%s.npz' % run))
    print('wrote %s' % path)


if __name__ == '__main__':
    main()
