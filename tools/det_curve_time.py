"""Times the detection-rate curves on targets [B,60,90,10], B = 16 and B = 256, both arms in one process:
  (a) Engine.det_curve: 9 joints x 20 radii, one launch, the targets read once;
  (b) what ONE radius of one joint set cost before it: Engine.argmax_coords(y[..., :9].contiguous()) + evaluation.det_rate_from_coords.
Each arm is warmed up, then timed in blocks of `inner` calls between two device events (a block lasts milliseconds, a single call only
microseconds), the arms alternated block by block so that both see the same clocks and neighbours; the figures are per call: the median
over the blocks, the minimum and the 90th percentile.  A host clock around the same blocks (ending in a synchronise) is reported beside the
device events: where the two agree the arm is bound by the host's launches, not by the kernels.  Writes <outdir>/det_curve_time.json.
    python tools/det_curve_time.py <outdir> [blocks=60] [inner=50]"""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import joint_cnn_mrf_amd  # noqa: F401,E402
from joint_cnn_mrf_amd import evaluation, synth  # noqa: E402
from joint_cnn_mrf_amd.engine import Engine  # noqa: E402

K, RADII = 9, list(range(1, 21))


def block(fn, inner):
    """(device ms, host ms) of `inner` consecutive calls."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    e0.record()
    for _ in range(inner):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), (time.perf_counter() - t0) * 1e3


def stats(ms_per_call):
    a = np.sort(np.asarray(ms_per_call))
    return {'blocks': int(a.size), 'median_us': float(np.median(a) * 1e3), 'min_us': float(a[0] * 1e3), 'p90_us': float(a[int(0.9 * (a.size - 1))] * 1e3)}


def main():
    if len(sys.argv) < 2:
        sys.exit(__doc__)
    outdir = sys.argv[1]
    blocks = int(sys.argv[2]) if len(sys.argv) > 2 else 60
    inner = int(sys.argv[3]) if len(sys.argv) > 3 else 50
    os.makedirs(outdir, exist_ok=True)
    eng = Engine(device=0)
    res = {'device': torch.cuda.get_device_name(0), 'blocks': blocks, 'calls_per_block': inner, 'radii': len(RADII), 'joints': K, 'sizes': {}}
    for B in (16, 256):
        y = torch.as_tensor(synth.make_targets(B, seed=7), device='cuda:0')
        pred = torch.randint(0, 60, (B, 2, K), dtype=torch.int32, device='cuda:0')
        hits = torch.zeros(K, len(RADII), dtype=torch.int32, device='cuda:0')

        def curve():
            eng.det_curve(pred, y, RADII, hits=hits)

        def one_radius():
            true = eng.argmax_coords(y[..., :K].contiguous())
            evaluation.det_rate_from_coords(pred, true, 10, [2])
        for fn in (curve, one_radius):                              # warm-up: code objects, torch's allocator
            block(fn, inner)
        t = {'curve': ([], []), 'one_radius': ([], [])}
        for _ in range(blocks):                                     # alternated
            for name, fn in (('curve', curve), ('one_radius', one_radius)):
                dev, host = block(fn, inner)
                t[name][0].append(dev / inner)
                t[name][1].append(host / inner)
        r = {'target_bytes': int(y.numel() * 4)}
        for name in t:
            r[name] = {'device_events': stats(t[name][0]), 'host_clock': stats(t[name][1])}
        r['curve_over_one_radius_device_median'] = r['curve']['device_events']['median_us'] / r['one_radius']['device_events']['median_us']
        r['curve_GBps_at_median'] = r['target_bytes'] / (r['curve']['device_events']['median_us'] * 1e-6) / 1e9
        res['sizes'][str(B)] = r
        print('B=%d: %s' % (B, json.dumps(r)), flush=True)
    eng.close()
    with open(os.path.join(outdir, 'det_curve_time.json'), 'w') as fh:
        json.dump(res, fh, indent=1)


if __name__ == '__main__':
    main()
