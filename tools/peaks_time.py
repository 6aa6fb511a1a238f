"""Times the heat-map peaks at [64,60,90,9] and [256,60,90,9], P = 4, both arms in one process:
  (a) jcm_hm_peaks on probabilities: reads the maps once, writes the four small outputs;
  (b) jcm_softmax_argmax with a probability output on logits of the same shape: reads the maps once and writes them back.
Both are called at the C ABI on preallocated outputs (the tensor allocations of the Python wrappers would be most of a call).  Each arm is
warmed up, then timed in blocks of `inner` calls between two device events, the arms alternated block by block so that both see the same
clocks and neighbours; the figures are per call: the median over the blocks, the minimum and the 90th percentile.  A host clock around the same
blocks (ending in a synchronise) is reported beside the device events: where the two agree the arm is bound by the host's launches, not by
the kernel.  With --forward: also Engine.forward() against Engine.forward(peaks=4) on a full-width fp32 engine, 64 images at 480x720, with the
spatial model, want_prob=False (so the peaks arm also pays for writing the two probability tensors), alternated call by call.
Writes <outdir>/peaks_time.json.
    python tools/peaks_time.py <outdir> [blocks=60] [inner=50] [--forward]"""
import ctypes
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

K, P, HH, WW = 9, 4, 60, 90


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
    for fn in arms.values():                                        # warm-up: code objects, torch's allocator
        block(fn, inner)
    t = {name: ([], []) for name in arms}
    for _ in range(blocks):
        for name, fn in arms.items():
            dev, host = block(fn, inner)
            t[name][0].append(dev / inner)
            t[name][1].append(host / inner)
    return {name: {'device_events': stats(t[name][0]), 'host_clock': stats(t[name][1])} for name in t}


def kernels(eng, blocks, inner):
    lib, h, p = eng._lib, eng._h, eng._p
    sizes = {}
    for B in (64, 256):
        logits = 3 * torch.randn(B, HH, WW, K, device='cuda:0')
        prob = torch.empty_like(logits)
        coords = torch.empty(B, 2, K, dtype=torch.int32, device='cuda:0')
        _lib.check(lib.jcm_softmax_argmax(h, p(logits), B, HH, WW, K, p(prob), p(coords)), 'jcm_softmax_argmax')
        hm = prob.clone()
        cells = torch.empty(B, K, P, 2, dtype=torch.int32, device='cuda:0')
        offsets = torch.empty(B, K, P, 2, device='cuda:0')
        scores = torch.empty(B, K, P, device='cuda:0')
        count = torch.empty(B, K, dtype=torch.int32, device='cuda:0')
        thr = ctypes.c_float(0.0)

        def peaks():
            lib.jcm_hm_peaks(h, p(hm), B, HH, WW, K, P, thr, p(cells), p(offsets), p(scores), p(count))

        def softmax_argmax():
            lib.jcm_softmax_argmax(h, p(logits), B, HH, WW, K, p(prob), p(coords))
        _lib.check(lib.jcm_hm_peaks(h, p(hm), B, HH, WW, K, P, thr, p(cells), p(offsets), p(scores), p(count)), 'jcm_hm_peaks')
        torch.cuda.synchronize()
        assert int(count.min()) == P and bool((cells[:, :, 0].permute(0, 2, 1) == coords).all())      # the timed call does the work
        r = alternate({'hm_peaks': peaks, 'softmax_argmax': softmax_argmax}, blocks, inner)
        r['map_bytes'] = int(hm.numel() * 4)
        r['peaks_over_softmax_argmax_device_median'] = r['hm_peaks']['device_events']['median_us'] / r['softmax_argmax']['device_events']['median_us']
        r['peaks_GBps_at_median'] = r['map_bytes'] / (r['hm_peaks']['device_events']['median_us'] * 1e-6) / 1e9
        sizes[str(B)] = r
        print('B=%d: %s' % (B, json.dumps(r)), flush=True)
    return sizes


def forward(blocks):
    B = 64
    params = synth.make_pd_params(debug=False)
    params.update(synth.make_sm_params(synth.synthetic_priors(), kind='init'))
    eng = Engine(device=0, precision='fp32').load_params(params)
    x = torch.as_tensor(np.concatenate([synth.make_images(16, seed=5)] * (B // 16)), device='cuda:0')
    torso = torch.as_tensor(synth.make_torso(B, seed=3), device='cuda:0')
    r = alternate({'forward': lambda: eng.forward(x, torso, use_sm=True, want_prob=False),
                   'forward_peaks4': lambda: eng.forward(x, torso, use_sm=True, want_prob=False, peaks=P)}, blocks, 1)
    r['peaks_cost_us_device_median'] = r['forward_peaks4']['device_events']['median_us'] - r['forward']['device_events']['median_us']
    r['peaks_cost_percent'] = 100 * r['peaks_cost_us_device_median'] / r['forward']['device_events']['median_us']
    eng.close()
    print('forward B=%d: %s' % (B, json.dumps(r)), flush=True)
    return r


def main():
    argv = [a for a in sys.argv[1:] if a != '--forward']
    if not argv:
        sys.exit(__doc__)
    outdir = argv[0]
    blocks = int(argv[1]) if len(argv) > 1 else 60
    inner = int(argv[2]) if len(argv) > 2 else 50
    os.makedirs(outdir, exist_ok=True)
    eng = Engine(device=0)
    res = {'device': torch.cuda.get_device_name(0), 'blocks': blocks, 'calls_per_block': inner, 'joints': K, 'peaks': P, 'sizes': kernels(eng, blocks, inner)}
    eng.close()
    if '--forward' in sys.argv[1:]:
        res['forward_fp32_b64'] = forward(min(blocks, 30))
    with open(os.path.join(outdir, 'peaks_time.json'), 'w') as fh:
        json.dump(res, fh, indent=1)


if __name__ == '__main__':
    main()
