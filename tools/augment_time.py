"""Times the training-time augmentation on a full-width fp32 engine, 16 images at 480 x 720 (maps 60 x 90 x 10):
(i) jcm_augment_train alone, device events around each of N calls after a warm-up; (ii) Trainer.train_step with and
without augment=, alternated in one process.  Writes <outdir>/augment_time.json.
    python tools/augment_time.py <outdir> [calls=300] [steps=40]
Kernel times come from a separate run under rocprofv3 --kernel-trace --stats with `--only-augment` (part (i) only)."""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import joint_cnn_mrf_amd  # noqa: F401,E402
from joint_cnn_mrf_amd import augmentation, synth  # noqa: E402
from joint_cnn_mrf_amd.engine import Engine  # noqa: E402
from joint_cnn_mrf_amd.train import Trainer  # noqa: E402

B, H, W, h, w = 16, 480, 720, 60, 90


def algorithmic_bytes(B, H, W, h, w):
    """Each input read once, each output written once."""
    return 2 * (B * H * W * 3 + B * h * w * 10) * 4


def event_times(fn, n):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(n + 1)]
    ev[0].record()
    for i in range(n):
        fn()
        ev[i + 1].record()
    torch.cuda.synchronize()
    return [ev[i].elapsed_time(ev[i + 1]) for i in range(n)]


def stats(ms):
    a = np.sort(np.asarray(ms))
    return {'n': int(a.size), 'median_ms': float(np.median(a)), 'min_ms': float(a[0]), 'p90_ms': float(a[int(0.9 * (a.size - 1))])}


def main():
    args = [a for a in sys.argv[1:] if not a.startswith('--')]
    only_augment = '--only-augment' in sys.argv
    if not args:
        sys.exit(__doc__)
    outdir = args[0]
    calls = int(args[1]) if len(args) > 1 else 300
    steps = int(args[2]) if len(args) > 2 else 40
    os.makedirs(outdir, exist_ok=True)
    x = torch.as_tensor(synth.make_images(B), device='cuda:0')
    y = torch.as_tensor(synth.make_targets(B), device='cuda:0')
    p = augmentation.draw_params(np.random.RandomState(0), B)
    res = {'B': B, 'H': H, 'W': W, 'h': h, 'w': w, 'algorithmic_bytes': algorithmic_bytes(B, H, W, h, w),
           'device': torch.cuda.get_device_name(0)}

    eng = Engine(device=0)
    pd = torch.as_tensor(p, device='cuda:0')
    xo, yo = torch.empty_like(x), torch.empty_like(y)
    one = lambda: eng.augment_train(x, y, pd, xo, yo)
    event_times(one, 20)                                            # warm-up
    res['augment'] = stats(event_times(one, calls))
    res['augment']['GBps_at_median'] = res['algorithmic_bytes'] / (res['augment']['median_ms'] * 1e-3) / 1e9
    eng.close()
    print('augment: %s' % res['augment'], flush=True)
    if not only_augment:
        params = synth.make_pd_params(debug=False)
        params.update(synth.make_sm_params(synth.synthetic_priors(), kind='init'))
        eng = Engine(device=0).load_params(params)
        tr = Trainer(eng, optimizer='adam', lr=1e-6, lmbd=0.001, use_sm=True)
        rng = np.random.RandomState(1)
        plain = lambda: tr.train_step(x, y)
        aug = lambda: tr.train_step(x, y, augment=augmentation.draw_params(rng, B))
        for _ in range(3):
            plain()
            aug()
        t_plain, t_aug = [], []
        for _ in range(steps):                                      # alternated: the two arms see the same clocks and neighbours
            t_plain += event_times(plain, 1)
            t_aug += event_times(aug, 1)
        res['train_step'] = stats(t_plain)
        res['train_step_augment'] = stats(t_aug)
        res['train_step_delta_median_ms'] = res['train_step_augment']['median_ms'] - res['train_step']['median_ms']
        d = np.asarray(t_aug) - np.asarray(t_plain)
        res['train_step_delta_paired_median_ms'] = float(np.median(d))
        eng.close()
        print('train_step: %s\ntrain_step augment: %s\ndelta (paired median) %.4f ms'
              % (res['train_step'], res['train_step_augment'], res['train_step_delta_paired_median_ms']), flush=True)
    with open(os.path.join(outdir, 'augment_time%s.json' % ('_only' if only_augment else '')), 'w') as fh:
        json.dump(res, fh, indent=1)


if __name__ == '__main__':
    main()
