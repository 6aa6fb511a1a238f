"""Times the torso inference at 64 fp32 images, full-width fp32 engine, spatial model on, want_prob=False:
  forward(torso='infer') beside forward(use_sm=True) with a GIVEN torso map, the same images, the same engine, alternated call by call in one
  process -- the difference is what inferring the torso adds; and jcm_torso_infer alone at the C ABI on the 64 probability maps of that forward,
  for every value of the option "torso_algo" (one: 1 = direct).
Each arm is warmed up, then timed in blocks of `inner` calls between two device events; the figures are per call: the median over the blocks, the
minimum and the 90th percentile.  Writes <outdir>/<name>.json.
    python tools/torso_time.py <outdir> [blocks=20] [inner=5] [--name torso_time]"""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import joint_cnn_mrf_amd  # noqa: F401,E402
from joint_cnn_mrf_amd import _lib, synth  # noqa: E402
from joint_cnn_mrf_amd.engine import Engine  # noqa: E402

ROUTES = {'direct': 1}


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


def alternate(arms, blocks, inner):
    for fn in arms.values():                                        # warm-up: code objects, filter spectra, torch's allocator
        block(fn, inner)
    t = {name: ([], []) for name in arms}
    for _ in range(blocks):
        for name, fn in arms.items():
            dev, host = block(fn, inner)
            t[name][0].append(dev / inner)
            t[name][1].append(host / inner)
    return {name: {'device_events': stats(t[name][0]), 'host_clock': stats(t[name][1])} for name in t}


def main():
    args = [a for a in sys.argv[1:] if not a.startswith('--')]
    name = sys.argv[sys.argv.index('--name') + 1] if '--name' in sys.argv else 'torso_time'
    if '--name' in sys.argv:
        args.remove(name)
    outdir = args[0]
    blocks, inner = (int(args[1]) if len(args) > 1 else 20), (int(args[2]) if len(args) > 2 else 5)
    B = 64
    params = synth.make_pd_params(debug=False, bn='trained', conv6_gain=8.0)
    params.update(synth.make_sm_params(synth.synthetic_priors(), kind='trained'))
    eng = Engine(device=0).load_params(params)
    x = torch.as_tensor(synth.make_images(B, seed=7), device='cuda:0')
    torso = torch.as_tensor(synth.make_torso(B, seed=8), device='cuda:0')
    doc = {'images': B, 'precision': 'fp32', 'blocks': blocks, 'inner': inner, 'device': torch.cuda.get_device_name(0)}
    arms = {'forward_given_torso': lambda: eng.forward(x, torso, use_sm=True, want_prob=False)}
    for route, value in ROUTES.items():
        def infer(value=value):
            eng.set_option('torso_algo', value)
            eng.forward(x, 'infer', use_sm=True, want_prob=False)
        arms['forward_infer_' + route] = infer
    doc['forward'] = alternate(arms, blocks, inner)
    base = doc['forward']['forward_given_torso']['device_events']['median_us']
    for route in ROUTES:
        doc['forward']['added_us_' + route] = doc['forward']['forward_infer_' + route]['device_events']['median_us'] - base
    prob = eng.forward(x, None, use_sm=False)['pd_prob']
    cell = torch.empty((B, 2), dtype=torch.int32, device='cuda:0')
    blob = torch.empty((B, 60, 90, 1), device='cuda:0')
    lib, h, p = eng._lib, eng._h, eng._p
    arms = {}
    for route, value in ROUTES.items():
        def kernel(value=value):
            lib.jcm_set_option(h, b'torso_algo', value)
            lib.jcm_torso_infer(h, p(prob), B, 60, 90, 9, p(None), p(None), p(cell), p(blob))
        _lib.check(lib.jcm_torso_infer(h, p(prob), B, 60, 90, 9, p(None), p(None), p(cell), p(blob)), 'jcm_torso_infer')
        arms['torso_infer_' + route] = kernel
    doc['kernel'] = alternate(arms, blocks, 4 * inner)
    os.makedirs(outdir, exist_ok=True)
    with open(os.path.join(outdir, name + '.json'), 'w') as fh:
        json.dump(doc, fh, indent=1)
    print(json.dumps({k: (v if not isinstance(v, dict) else {a: (b['device_events'] if isinstance(b, dict) else b) for a, b in v.items()}) for k, v in doc.items()}))
    eng.close()


if __name__ == '__main__':
    main()
