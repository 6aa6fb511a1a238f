"""Times the antialiased affine sample beside the plain one: 16 images at 480 x 720 read through an index from a device-resident
data set of 32 images, held as floats and as bytes, at the fixed scales 1.5, 1.0, 0.75, 0.5 and 0.25 about the centre (no rotation, identity colour;
augmentation.fixed_affine).  Per scale and image type two arms -- jcm_augment_affine_aa_indexed(_u8) with the widths of the scale, and
jcm_augment_affine_indexed(_u8) with the same geometry -- alternated call by call in one process, device events around each of N calls after a
warm-up.  Reports each median beside the plain entry's median of the same run, their ratio, the filter half-width and the taps per output pixel
(counted on the host from the geometry: the products of the columns and rows of positive weight, averaged over the output pixels of one image).
Writes <outdir>/affine_aa_time.json.
    python tools/affine_aa_time.py <outdir> [calls=200]"""
import json
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import joint_cnn_mrf_amd  # noqa: F401,E402
from joint_cnn_mrf_amd import augmentation, synth  # noqa: E402
from joint_cnn_mrf_amd.engine import Engine  # noqa: E402
from joint_cnn_mrf_amd.eval_run import byte_grid  # noqa: E402

B, N, H, W, h, w = 16, 32, 480, 720, 60, 90
SCALES = (1.5, 1.0, 0.75, 0.5, 0.25)


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


def taps_per_pixel(g, width):
    """The mean number of taps of an output pixel of an H x W image under geom row g (no rotation: columns and rows separate)."""
    if width == 1.0:
        return 4.0

    def axis(n, a, c0):
        cnt = []
        for q in range(n):
            p = a * q + c0
            cnt.append(sum(1 for i in range(int(math.ceil(p - width)), int(math.floor(p + width)) + 1) if 1.0 - abs(p - i) / width > 0.0))
        return np.array(cnt, np.float64)
    return float(np.outer(axis(H, g[4], g[5]), axis(W, g[0], g[2])).mean())


def main():
    args = [a for a in sys.argv[1:] if not a.startswith('--')]
    if not args:
        sys.exit(__doc__)
    outdir = args[0]
    calls = int(args[1]) if len(args) > 1 else 200
    os.makedirs(outdir, exist_ok=True)
    xb = byte_grid(synth.make_images(N))
    x_u8 = torch.as_tensor(xb, device='cuda:0')
    x_f32 = torch.as_tensor(xb.astype(np.float32) / np.float32(255), device='cuda:0')
    y = torch.as_tensor(synth.make_targets(N), device='cuda:0')
    idx = np.random.RandomState(0).permutation(N)[:B].astype(np.int32)
    res = {'B': B, 'N': N, 'H': H, 'W': W, 'calls': calls, 'device': torch.cuda.get_device_name(0), 'scales': list(SCALES)}
    eng = Engine(device=0)
    cells = eng.joint_cells(y)
    xo, yo = torch.empty((B, H, W, 3), device='cuda:0'), torch.empty((B, h, w, 10), device='cuda:0')
    arms, meta = {}, {}
    for s in SCALES:
        d = augmentation.fixed_affine(B, H, W, s, pad=0.5)
        meta[s] = {'width': float(d.width[0]), 'taps_per_pixel': taps_per_pixel(d.geom[0], float(d.width[0]))}
        for name, x in (('float', x_f32), ('byte', x_u8)):
            arms[(s, name, 'aa')] = lambda x=x, d=d: eng.augment_affine_indexed(x, cells, idx, d.colour, d.geom, d.pad, xo, yo, width=d.width)
            arms[(s, name, 'plain')] = lambda x=x, d=d: eng.augment_affine_indexed(x, cells, idx, d.colour, d.geom, d.pad, xo, yo)
    times = {k: [] for k in arms}
    for _ in range(10):                                               # warm-up
        for fn in arms.values():
            fn()
    torch.cuda.synchronize()
    for _ in range(calls):                                            # alternated: the arms see the same clocks and neighbours
        for k, fn in arms.items():
            times[k].append(event_time(fn))
    for s in SCALES:
        for name in ('float', 'byte'):
            aa, plain = stats(times[(s, name, 'aa')]), stats(times[(s, name, 'plain')])
            key = 'scale_%g_%s' % (s, name)
            res[key] = dict(meta[s], aa=aa, plain=plain, aa_over_plain=aa['median_ms'] / plain['median_ms'],
                            paired_delta_median_ms=float(np.median(np.asarray(times[(s, name, 'aa')]) - np.asarray(times[(s, name, 'plain')]))))
            print('%s: width %.4g, %.1f taps/pixel, aa %.4f ms, plain %.4f ms, ratio %.2f' % (key, meta[s]['width'], meta[s]['taps_per_pixel'], aa['median_ms'],
                                                                                              plain['median_ms'], res[key]['aa_over_plain']), flush=True)
    eng.close()
    with open(os.path.join(outdir, 'affine_aa_time.json'), 'w') as fh:
        json.dump(res, fh, indent=1)


if __name__ == '__main__':
    main()
