"""Times pose decoding alone: Engine.pose_decode on hm10 [B,60,90,10] with P candidates per joint, B = 64 and P = 4 unless
given -- the three launches of jcm_pose_decode (tables, search, finish) -- and, beside it, Engine.hm_peaks on the nine joint maps, the launch
that makes its candidates.  Each arm is warmed up, then timed in blocks of `inner` calls between two device events (a block lasts
milliseconds, a single call only microseconds), the arms alternated block by block; the figures are per call: the median over the blocks, the
minimum and the 90th percentile.  A host clock around the same blocks (ending in a synchronise) is reported beside the device events: where
the two agree the arm is bound by the host's launches, not by the kernels.  Writes <outdir>/pose_decode_time.json.
    python tools/pose_decode_time.py <outdir> [blocks=60] [inner=50] [B=64] [P=4]"""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import joint_cnn_mrf_amd  # noqa: F401,E402
from joint_cnn_mrf_amd import synth  # noqa: E402
from joint_cnn_mrf_amd.engine import Engine  # noqa: E402


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
    blocks, inner, B, P = [int(sys.argv[i]) if len(sys.argv) > i else d for i, d in ((2, 60), (3, 50), (4, 64), (5, 4))]
    os.makedirs(outdir, exist_ok=True)
    params = synth.make_pd_params(debug=True, bn='trained', conv6_gain=8.0)      # the tower's width does not enter: only the spatial model's tables are read
    params.update(synth.make_sm_params(synth.synthetic_priors(), kind='trained'))
    eng = Engine(device=0).load_params(params)
    logits = 3 * torch.randn(B, 60, 90, 9, generator=torch.Generator().manual_seed(5))
    prob = torch.softmax(logits.reshape(B, 5400, 9), dim=1).reshape(B, 60, 90, 9)
    hm10 = torch.cat([prob, torch.as_tensor(synth.make_torso(B))], dim=3).to('cuda:0').contiguous()
    hm9 = hm10[..., :9].contiguous()
    peaks = eng.hm_peaks(hm9, max_peaks=P)
    torch.cuda.synchronize()
    assert int(peaks['count'].min()) == P      # the full P^9 poses per image
    out = {}

    def decode():
        out['pose'] = eng.pose_decode(hm10, peaks)

    def find_peaks():
        eng.hm_peaks(hm9, max_peaks=P)
    arms = (('pose_decode', decode), ('hm_peaks', find_peaks))
    for _, fn in arms:                                              # warm-up: code objects, torch's allocator, the workspace
        block(fn, inner)
    t = {name: ([], []) for name, _ in arms}
    for _ in range(blocks):                                         # alternated
        for name, fn in arms:
            dev, host = block(fn, inner)
            t[name][0].append(dev / inner)
            t[name][1].append(host / inner)
    res = {'device': torch.cuda.get_device_name(0), 'blocks': blocks, 'calls_per_block': inner, 'B': B, 'P': P, 'poses_per_image': P ** 9,
           'pose_changed': float((out['pose']['index'] != 0).any(dim=1).float().mean())}
    for name in t:
        res[name] = {'device_events': stats(t[name][0]), 'host_clock': stats(t[name][1])}
    res['poses_per_second_at_median'] = B * P ** 9 / (res['pose_decode']['device_events']['median_us'] * 1e-6)
    print(json.dumps(res), flush=True)
    eng.close()
    with open(os.path.join(outdir, 'pose_decode_time.json'), 'w') as fh:
        json.dump(res, fh, indent=1)


if __name__ == '__main__':
    main()
