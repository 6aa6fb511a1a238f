"""Times the renderer of rendered people for 16 and 64 images of 480 x 720: jcm_synth_people with the default scene of
synth.people_batch and with 64 primitives an image, alternated call by call in one process with jcm_gather_batch_u8 of the same batch (what a fresh
batch replaces) and with a device copy of the output's bytes; device events around each of N calls after a warm-up (the method of tools/affine_time.py).
The device times are the launches' only; what synth.people_batch costs on the host per batch is timed beside them with the host clock.
Writes <outdir>/synth_people_time.json.
    python tools/synth_people_time.py <outdir> [calls=300]"""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import joint_cnn_mrf_amd  # noqa: F401,E402
from joint_cnn_mrf_amd import synth  # noqa: E402
from joint_cnn_mrf_amd.engine import Engine  # noqa: E402

H, W, h, w = 480, 720, 60, 90
HOST_FEED_MS = 2.4      # a host-fed step costs 24.9 ms against 22.5 ms from device-resident data, 16 images


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


def full_lists(rng, recs, prims):
    """Every image's list filled up to 64 primitives with copies of its own, drawn at random."""
    out, first = [], 0
    recs = recs.copy()
    for r in recs:
        own = prims[r[17]:r[17] + r[16]]
        out.append(np.concatenate([own, own[rng.randint(0, own.shape[0], 64 - own.shape[0])]]))
        r[16], r[17] = 64, first
        first += 64
    return recs, np.concatenate(out)


def main():
    args = [a for a in sys.argv[1:] if not a.startswith('--')]
    if not args:
        sys.exit(__doc__)
    outdir = args[0]
    calls = int(args[1]) if len(args) > 1 else 300
    os.makedirs(outdir, exist_ok=True)
    poses = np.load(os.path.join(ROOT, 'tests', 'golden', 'flic_train_xy.npy'))
    eng = Engine(device=0)
    res = {'H': H, 'W': W, 'calls': calls, 'device': torch.cuda.get_device_name(0), 'host_feed_ms_per_16_images': HOST_FEED_MS}
    for B in (16, 64):
        rng = np.random.RandomState(B)
        idx_poses = rng.permutation(poses.shape[0])[:B]
        recs, prims, _xy, _cells, y = synth.people_batch(rng, poses, idx_poses)
        recs64, prims64 = full_lists(rng, recs, prims)
        out = torch.empty((B, H, W, 3), dtype=torch.uint8, device='cuda:0')
        x_all = eng.synth_people(recs, prims, H, W)
        y_all = torch.as_tensor(y, device='cuda:0')
        idx = rng.permutation(B).astype(np.int32)
        xo, yo = torch.empty((B, H, W, 3), device='cuda:0'), torch.empty((B, h, w, 10), device='cuda:0')
        arms = {'synth_default': lambda: eng.synth_people(recs, prims, H, W, out=out),
                'synth_64_prims': lambda: eng.synth_people(recs64, prims64, H, W, out=out),
                'gather_u8': lambda: eng.gather_batch(x_all, y_all, idx, xo, yo),
                'copy_bytes': lambda: out.copy_(x_all)}
        times = {k: [] for k in arms}
        for _ in range(20):
            for fn in arms.values():
                fn()
        torch.cuda.synchronize()
        for _ in range(calls):
            for k, fn in arms.items():
                times[k].append(event_time(fn))
        r = {k: stats(v) for k, v in times.items()}
        host = []      # what the device times above leave out: the scenes are built on the host, in Python (host clock, no device work)
        for _ in range(30):
            t0 = time.perf_counter()
            synth.people_batch(rng, poses, idx_poses)
            host.append((time.perf_counter() - t0) * 1e3)
        r['host_people_batch'] = stats(host)
        r['prims_default_mean'] = float(recs[:, 16].mean())
        r['output_bytes'] = int(out.numel())
        for k in ('synth_default', 'synth_64_prims'):
            r[k]['GBps_written_at_median'] = out.numel() / (r[k]['median_ms'] * 1e-3) / 1e9
            r[k]['over_gather_u8'] = r[k]['median_ms'] / r['gather_u8']['median_ms']
            r[k]['over_copy_bytes'] = r[k]['median_ms'] / r['copy_bytes']['median_ms']
        res['B%d' % B] = r
        print('B = %d: %s' % (B, json.dumps(r)), flush=True)
    res['kernel_16_images_under_host_feed'] = bool(res['B16']['synth_default']['median_ms'] < HOST_FEED_MS)
    res['kernel_plus_host_scenes_16_images_under_host_feed'] = bool(
        res['B16']['synth_default']['median_ms'] + res['B16']['host_people_batch']['median_ms'] < HOST_FEED_MS)
    eng.close()
    with open(os.path.join(outdir, 'synth_people_time.json'), 'w') as fh:
        json.dump(res, fh, indent=1)


if __name__ == '__main__':
    main()
