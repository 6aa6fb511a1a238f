"""Times the epoch loop's feeding of the training step on a full-width fp32 tower, batch 16 at 480 x 720:
  (a) the host-fed loop body: evaluation.get_next_batch on memory-mapped .npy files, then TowerTrainer.train_step;
  (b) DeviceDataset.epoch_indices, then TowerTrainer.train_step_indexed;
  (c) the floor: Trainer.train_step on one fixed device-resident batch;
each without and with augmentation.  The six arms are alternated step by step in one process after a warm-up; a step is timed
on the host from the start of its loop body to the end of its device work (synchronised), so (a) carries its host gather and
its pageable copy.  A second pass times blocks of consecutive steps with one synchronisation per block (the loop as it runs,
host work of a step overlapping the device work of the one before).  Also: the one-off upload (time, rate) and device-event
times of jcm_gather_batch, jcm_augment_train_indexed and gather followed by jcm_augment_train, alternated.
The data: N synthetic images and targets written as .npy into a temporary directory (about 1 GB; no data set is needed).
    timeout -k 10 900 python tools/epoch_time.py <outdir> [steps=32] [calls=200]
Writes <outdir>/epoch_time.json."""
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import joint_cnn_mrf_amd  # noqa: F401,E402
from joint_cnn_mrf_amd import augmentation, evaluation, synth  # noqa: E402
from joint_cnn_mrf_amd.dataset import DeviceDataset  # noqa: E402
from joint_cnn_mrf_amd.dist import Towers  # noqa: E402
from joint_cnn_mrf_amd.main import TowerTrainer  # noqa: E402

B, H, W, h, w = 16, 480, 720, 60, 90
N = 240                      # 240 x 4.15 MB = 995 MB of images
BLOCK = 8


def stats(ms):
    a = np.sort(np.asarray(ms, np.float64))
    return {'n': int(a.size), 'median_ms': float(np.median(a)), 'min_ms': float(a[0]), 'p10_ms': float(a[int(0.1 * (a.size - 1))]),
            'p90_ms': float(a[int(0.9 * (a.size - 1))]), 'max_ms': float(a[-1])}


def write_files(tmp):
    px, py = os.path.join(tmp, 'x.npy'), os.path.join(tmp, 'y.npy')
    x = np.lib.format.open_memmap(px, mode='w+', dtype=np.float32, shape=(N, H, W, 3))
    for lo in range(0, N, 16):
        x[lo:lo + 16] = synth.make_images(min(16, N - lo), seed=1000 + lo)
    x.flush()
    del x
    np.save(py, synth.make_targets(N, seed=77))
    return px, py


def event_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def main():
    args = [a for a in sys.argv[1:] if not a.startswith('--')]
    if not args:
        sys.exit(__doc__)
    outdir = args[0]
    steps = int(args[1]) if len(args) > 1 else 32
    calls = int(args[2]) if len(args) > 2 else 200
    os.makedirs(outdir, exist_ok=True)
    res = {'B': B, 'H': H, 'W': W, 'h': h, 'w': w, 'N': N, 'device': torch.cuda.get_device_name(0), 'block': BLOCK}
    tmp = tempfile.mkdtemp(prefix='epoch_time_')
    try:
        px, py = write_files(tmp)
        res['file_bytes'] = os.path.getsize(px) + os.path.getsize(py)
        xm, ym = np.load(px, mmap_mode='r'), np.load(py, mmap_mode='r')
        params = synth.make_pd_params(debug=False)
        params.update(synth.make_sm_params(synth.synthetic_priors(), kind='init'))
        towers = Towers(params, [0])
        eng = towers.engines[0]
        tt = TowerTrainer(towers, params, optimizer='adam', lr=1e-6, lmbd=0.001, use_sm=True)
        tr = tt.trainers[0]
        ds = DeviceDataset(px, py, device=0)
        res['upload'] = {'bytes': ds.nbytes, 'seconds': ds.upload_seconds, 'GBps': ds.nbytes / ds.upload_seconds / 1e9}
        print('upload: %s' % res['upload'], flush=True)
        xf, yf = ds.x[:B].clone(), ds.y[:B].clone()
        rng_a, rng_b, rng_p = np.random.RandomState(0), np.random.RandomState(0), np.random.RandomState(1)

        def endless(make):
            while True:
                for item in make():
                    yield item
        host_batches = endless(lambda: evaluation.get_next_batch(xm, ym, B, shuffle=True, rng=rng_a))
        index_batches = endless(lambda: ds.epoch_indices(rng_b, B, shuffle=True))

        def arm_a():
            bx, by = next(host_batches)
            tt.train_step(np.ascontiguousarray(bx, np.float32), np.ascontiguousarray(by, np.float32))

        def arm_b():
            tt.train_step_indexed(ds, next(index_batches))

        def arm_c(aug):
            tr.train_step(xf, yf, augment=augmentation.draw_params(rng_p, B) if aug else None)
        arms = []
        for aug in (False, True):
            sfx = '_augment' if aug else ''
            arms += [('a_host_fed' + sfx, arm_a, aug), ('b_indexed' + sfx, arm_b, aug), ('c_floor' + sfx, (lambda aug=aug: arm_c(aug)), aug)]

        def run(fn, aug, n):
            tt.augment_rng = rng_p if aug else None
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(n):
                fn()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3 / n
        for _ in range(3):                                                 # warm-up: filter spectra, workspace, page cache of a few batches
            for _name, fn, aug in arms:
                run(fn, aug, 1)
        per_step = {name: [] for name, _f, _a in arms}
        for _ in range(steps):                                             # alternated: every arm sees the same clocks and neighbours
            for name, fn, aug in arms:
                per_step[name].append(run(fn, aug, 1))
        res['step_synchronised'] = {k: stats(v) for k, v in per_step.items()}
        blocks = {name: [] for name, _f, _a in arms}
        for _ in range(max(4, steps // BLOCK)):
            for name, fn, aug in arms:
                blocks[name].append(run(fn, aug, BLOCK))
        res['step_in_blocks'] = {k: stats(v) for k, v in blocks.items()}
        for k in per_step:
            print('%-22s synchronised %s\n%-22s in blocks    %s' % (k, res['step_synchronised'][k], '', res['step_in_blocks'][k]), flush=True)

        # the kernels alone, device events, alternated
        idx = ds.epoch_indices(np.random.RandomState(2), B, shuffle=True)
        pd = torch.as_tensor(augmentation.draw_params(np.random.RandomState(3), B), device='cuda:0')
        xo, yo, xg, yg = torch.empty_like(xf), torch.empty_like(yf), torch.empty_like(xf), torch.empty_like(yf)
        k = [0]
        nxt = lambda: idx[k[0] % len(idx)]
        kern = {'gather_batch': lambda: eng.gather_batch(ds.x, ds.y, nxt(), xg, yg),
                'augment_train_indexed': lambda: eng.augment_train_indexed(ds.x, ds.y, nxt(), pd, xo, yo),
                'gather_then_augment_train': lambda: eng.augment_train(*eng.gather_batch(ds.x, ds.y, nxt(), xg, yg), pd, xo, yo),
                'augment_train': lambda: eng.augment_train(xf, yf, pd, xo, yo)}
        t = {name: [] for name in kern}
        for i in range(calls + 20):
            k[0] = i
            for name, fn in kern.items():
                ms = event_ms(fn)
                if i >= 20:
                    t[name].append(ms)
        res['kernels_device_events'] = {name: stats(v) for name, v in t.items()}
        batch_bytes = (B * H * W * 3 + B * h * w * 10) * 4
        res['batch_bytes'] = batch_bytes
        res['kernels_device_events']['gather_batch']['GBps_at_median'] = 2 * batch_bytes / (res['kernels_device_events']['gather_batch']['median_ms'] * 1e-3) / 1e9
        for name in kern:
            print('%-28s %s' % (name, res['kernels_device_events'][name]), flush=True)
        towers.close()
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    with open(os.path.join(outdir, 'epoch_time.json'), 'w') as fh:
        json.dump(res, fh, indent=1)


if __name__ == '__main__':
    main()
