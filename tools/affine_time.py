"""Times the affine training augmentation on a full-width fp32 engine, 16 images at 480 x 720 (maps 60 x 90 x 10), read through an index
from a device-resident data set of 32 images held as floats and as bytes:
(i) jcm_augment_affine_indexed(_u8) and jcm_augment_train_indexed(_u8) on the same data, alternated call by call in one process, device events around
    each of N calls after a warm-up;
(ii) Trainer.train_step_indexed without augmentation, with the reference's augmentation and with the affine one, alternated step by step.
Writes <outdir>/affine_time.json.
    python tools/affine_time.py <outdir> [calls=300] [steps=40] [--only-augment]"""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import joint_cnn_mrf_amd  # noqa: F401,E402
from joint_cnn_mrf_amd import augmentation, synth  # noqa: E402
from joint_cnn_mrf_amd.engine import Engine  # noqa: E402
from joint_cnn_mrf_amd.eval_run import byte_grid  # noqa: E402
from joint_cnn_mrf_amd.train import Trainer  # noqa: E402

B, N, H, W, h, w = 16, 32, 480, 720, 60, 90


def algorithmic_bytes(image_bytes):
    """Each source image read twice (the mean pass and the sampling pass; a sample reads about one source pixel per output pixel at scale 1), the cells read,
    each output written once."""
    return B * (2 * H * W * 3 * image_bytes + 10 * 2 * 4 + H * W * 3 * 4 + h * w * 10 * 4)


def event_time(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def stats(ms):
    a = np.sort(np.asarray(ms))
    return {'n': int(a.size), 'median_ms': float(np.median(a)), 'min_ms': float(a[0]), 'p90_ms': float(a[int(0.9 * (a.size - 1))])}


class Set:
    """What Trainer.loss_and_grads_indexed reads of a DeviceDataset."""

    def __init__(self, x, y, cells):
        self.x, self.y, self.cells = x, y, cells


def main():
    args = [a for a in sys.argv[1:] if not a.startswith('--')]
    only_augment = '--only-augment' in sys.argv
    if not args:
        sys.exit(__doc__)
    outdir = args[0]
    calls = int(args[1]) if len(args) > 1 else 300
    steps = int(args[2]) if len(args) > 2 else 40
    os.makedirs(outdir, exist_ok=True)
    xb = byte_grid(synth.make_images(N))
    x_u8 = torch.as_tensor(xb, device='cuda:0')
    x_f32 = torch.as_tensor(xb.astype(np.float32) / np.float32(255), device='cuda:0')
    y = torch.as_tensor(synth.make_targets(N), device='cuda:0')
    rng = np.random.RandomState(0)
    idx = rng.permutation(N)[:B].astype(np.int32)
    p6 = torch.as_tensor(augmentation.draw_params(rng, B), device='cuda:0')
    draw = augmentation.draw_affine(rng, B, H, W)                    # the default ranges: scale [0.5, 1.5], +-20 degrees, no shift
    res = {'B': B, 'N': N, 'H': H, 'W': W, 'h': h, 'w': w, 'calls': calls, 'device': torch.cuda.get_device_name(0),
           'affine_ranges': {'scale': list(augmentation.AFFINE_SCALE), 'max_angle': augmentation.MAX_ROTATE_ANGLE, 'shift': augmentation.AFFINE_SHIFT}}

    eng = Engine(device=0)
    cells = eng.joint_cells(y)
    xo, yo = torch.empty((B, H, W, 3), device='cuda:0'), torch.empty((B, h, w, 10), device='cuda:0')
    arms = {}
    for name, x in (('float', x_f32), ('byte', x_u8)):
        arms['affine_' + name] = lambda x=x: eng.augment_affine_indexed(x, cells, idx, draw.colour, draw.geom, draw.pad, xo, yo)
        arms['reference_' + name] = lambda x=x: eng.augment_train_indexed(x, y, idx, p6, xo, yo)
    times = {k: [] for k in arms}
    for _ in range(20):                                               # warm-up
        for fn in arms.values():
            fn()
    torch.cuda.synchronize()
    for _ in range(calls):                                            # alternated: the arms see the same clocks and neighbours
        for k, fn in arms.items():
            times[k].append(event_time(fn))
    for k in arms:
        res[k] = stats(times[k])
        if k.startswith('affine'):
            nbytes = algorithmic_bytes(4 if k.endswith('float') else 1)
            res[k].update(algorithmic_bytes=nbytes, GBps_at_median=nbytes / (res[k]['median_ms'] * 1e-3) / 1e9)
        print('%s: %s' % (k, res[k]), flush=True)
    for name in ('float', 'byte'):
        res['affine_over_reference_' + name] = res['affine_' + name]['median_ms'] / res['reference_' + name]['median_ms']
    eng.close()

    if not only_augment:
        params = synth.make_pd_params(debug=False)
        params.update(synth.make_sm_params(synth.synthetic_priors(), kind='init'))
        eng = Engine(device=0).load_params(params)
        tr = Trainer(eng, optimizer='adam', lr=1e-6, lmbd=0.001, use_sm=True)
        ds = Set(x_u8, y, eng.joint_cells(y))
        rng = np.random.RandomState(1)
        step = {'plain': lambda: tr.train_step_indexed(ds, idx),
                'reference': lambda: tr.train_step_indexed(ds, idx, augment=augmentation.draw_params(rng, B)),
                'affine': lambda: tr.train_step_indexed(ds, idx, augment=augmentation.draw_affine(rng, B, H, W))}
        for _ in range(3):
            for fn in step.values():
                fn()
        torch.cuda.synchronize()
        t = {k: [] for k in step}
        for _ in range(steps):
            for k, fn in step.items():
                t[k].append(event_time(fn))
        for k in step:
            res['train_step_' + k] = stats(t[k])
            print('train_step %s: %s' % (k, res['train_step_' + k]), flush=True)
        for k in ('reference', 'affine'):
            res['train_step_%s_delta_paired_median_ms' % k] = float(np.median(np.asarray(t[k]) - np.asarray(t['plain'])))
        eng.close()
    with open(os.path.join(outdir, 'affine_time%s.json' % ('_only' if only_augment else '')), 'w') as fh:
        json.dump(res, fh, indent=1)


if __name__ == '__main__':
    main()
