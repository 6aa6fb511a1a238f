"""Times the per-layer activation summaries (--tb_activations) on a full-width fp32 engine, batch 14 at 480 x 720, spatial model on:
(i) summary.merged_summary of the evaluation run (no gradients) without and with activations=True, the two arms alternated, host clock around
each call ending in a synchronise; (ii) Engine.act_summary on the pre-activation of conv1_fullres [14,240,360,64], the largest tensor of the
chain, for 1 and 4 tower slices: device events per call, and the GB/s of z read + activation written + pictures written.
Writes <outdir>/activ_summary_time.json.
    python tools/activ_summary_time.py <outdir> [rounds=3] [calls=20]"""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import joint_cnn_mrf_amd  # noqa: F401,E402
from joint_cnn_mrf_amd import summary as S, synth  # noqa: E402
from joint_cnn_mrf_amd.engine import Engine  # noqa: E402

B = 14


def main():
    if len(sys.argv) < 2:
        sys.exit(__doc__)
    outdir = sys.argv[1]
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    calls = int(sys.argv[3]) if len(sys.argv) > 3 else 20
    os.makedirs(outdir, exist_ok=True)
    p = synth.make_pd_params(debug=False, bn='trained')
    p.update(synth.make_sm_params(synth.synthetic_priors(), kind='init'))
    eng = Engine(device=0).load_params(p)
    x = torch.as_tensor(synth.make_images(B, seed=5), device='cuda:0')
    y = torch.as_tensor(synth.make_targets(B, seed=6), device='cuda:0')
    flat, layout = S.flat_params(eng, p)
    res = {'device': torch.cuda.get_device_name(0), 'batch': B, 'rounds': rounds, 'calls': calls}

    def merged(act):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        s = S.merged_summary(eng, layout, x, y, True, 9, params_flat=flat, activations=act, n_towers=1)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, len(s)

    for act in (False, True):      # first use: filter spectra, workspace, PNG pool
        merged(act)
    t = {False: [], True: []}
    nbytes = {}
    for _ in range(rounds):
        for act in (False, True):
            ms, nbytes[act] = merged(act)
            t[act].append(ms)
    res['merged_summary_ms'] = {'without': t[False], 'with_activations': t[True], 'median_without': float(np.median(t[False])),
                                'median_with': float(np.median(t[True])), 'summary_bytes_without': nbytes[False], 'summary_bytes_with': nbytes[True]}

    z = eng.conv_layer_pre(x, 'conv1_fullres', 2, 64)
    res['act_summary_conv1_fullres'] = {}
    for n_groups in (1, 4):
        n_pics = min(3, B // n_groups)
        used = (B // n_groups) * n_groups
        moved = 2 * used * z[0].numel() * 4 + n_groups * n_pics * 240 * 360 * 4
        for _ in range(3):
            eng.act_summary(z, 'conv1_fullres', n_groups=n_groups, n_pics=n_pics)
        eng.set_profile(True)
        for _ in range(calls):
            eng.act_summary(z, 'conv1_fullres', n_groups=n_groups, n_pics=n_pics)
        total_ms, n = eng.profile_read('conv1_fullres/act_summary')
        eng.set_profile(False)
        res['act_summary_conv1_fullres']['n_groups=%d' % n_groups] = {'launch_pairs': n, 'mean_ms': total_ms / max(n, 1), 'bytes_moved': moved,
                                                                      'GB_per_s': moved / (total_ms / max(n, 1) * 1e-3) / 1e9}
    with open(os.path.join(outdir, 'activ_summary_time.json'), 'w') as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
