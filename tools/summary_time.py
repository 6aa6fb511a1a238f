"""Times the TensorBoard summaries on a full-width fp32 engine after one training step (batch 14, 480 x 720, spatial model on):
(i) jcm_tensor_stats over every trainable parameter (read in place) and over the clipped gradients, device events per call;
(ii) jcm_hm_overlay for 14 images x 3 sets; (iii) PNG encoding of those 420 pictures on the thread pool; (iv) the whole per-epoch
summary pass (merged_summary for the train and the test batch, written to two event files).  Writes <outdir>/summary_time.json.
    python tools/summary_time.py <outdir> [calls=50] [--kernels-only]
Kernel times come from a separate run under rocprofv3 --kernel-trace --stats with --kernels-only (parts (i) and (ii) only);
pass its results database (<dir>/s_results.db) as --stats DB to fold the per-kernel times into the JSON."""
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import joint_cnn_mrf_amd  # noqa: F401,E402
from joint_cnn_mrf_amd import summary as S, synth  # noqa: E402
from joint_cnn_mrf_amd.engine import Engine  # noqa: E402
from joint_cnn_mrf_amd.train import Trainer  # noqa: E402

B = 14
HBM_PEAK_TBPS = 8.0      # MI355X HBM3E


def event_times(fn, n):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(n + 1)]
    ev[0].record()
    for i in range(n):
        fn()
        ev[i + 1].record()
    torch.cuda.synchronize()
    return [ev[i].elapsed_time(ev[i + 1]) for i in range(n)]


def med(ms):
    a = np.asarray(ms)
    return {'n': int(a.size), 'median_ms': float(np.median(a)), 'min_ms': float(a.min())}


def main():
    args = [a for a in sys.argv[1:] if not a.startswith('--')]
    outdir = args[0]
    calls = int(args[1]) if len(args) > 1 else 50
    kernels_only = '--kernels-only' in sys.argv
    stats_db = sys.argv[sys.argv.index('--stats') + 1] if '--stats' in sys.argv else None
    os.makedirs(outdir, exist_ok=True)
    p = synth.make_pd_params(debug=False, bn='trained')
    p.update(synth.make_sm_params(synth.synthetic_priors(), kind='init'))
    eng = Engine(device=0).load_params(p)
    tr = Trainer(eng, use_sm=True)
    x = torch.as_tensor(synth.make_images(B, seed=1), device='cuda:0')
    y = torch.as_tensor(synth.make_targets(B, seed=2), device='cuda:0')
    tr.loss_and_grads(x, y)
    tr.apply()
    segs = [(o, c) for _, o, c in tr.layout]
    n_el = tr.n_elements
    hm = eng.eval_forward(x, y, use_sm=True, want_prob=True)
    sets = [y[..., :9].contiguous(), hm['pd_prob'], hm['sm_prob']]
    out = {'B': B, 'n_tensors': len(segs), 'n_elements': int(n_el), 'device': torch.cuda.get_device_name(0)}
    t_par = event_times(lambda: eng.tensor_stats(None, segs), calls)
    t_grd = event_times(lambda: eng.tensor_stats(tr.grads, segs, clip_norm=4.0), calls)
    t_ovl = event_times(lambda: [eng.hm_overlay(x, s, B) for s in sets], calls)
    if kernels_only:
        return
    for k, t in (('stats_params', t_par), ('stats_grads', t_grd)):
        out[k] = med(t)
        out[k]['note'] = 'whole call incl. chunk-table upload, stream synchronisation and the copy of the counts to the host'
    out['overlays_14x3'] = med(t_ovl)
    u8 = [eng.hm_overlay(x, s, B).cpu().numpy() for s in sets]
    t0 = time.perf_counter()
    futs = [S.png_pool().submit(S.encode_png, u[b, j]) for u in u8 for b in range(B) for j in range(10)]
    nbytes = sum(len(f.result()) for f in futs)
    out['png_420'] = {'seconds': time.perf_counter() - t0, 'pictures': len(futs), 'png_bytes': nbytes, 'threads': S.png_pool()._max_workers,
                      'zlib_level': S.PNG_LEVEL}
    d = tempfile.mkdtemp()
    writers = {k: S.FileWriter(os.path.join(d, k)) for k in ('train', 'test')}
    passes = []
    for _ in range(3):
        t0 = time.perf_counter()
        for k, w in writers.items():
            S.run_summary(w, S.merged_summary(eng, tr.layout, x, y, True, 9, grads=tr.grads), 1)
        passes.append(time.perf_counter() - t0)
    for w in writers.values():
        w.close()
    out['epoch_pass_two_writers'] = {'seconds_median': float(np.median(passes)), 'seconds': passes,
                                     'event_file_bytes': sum(os.path.getsize(w.path) for w in writers.values()) // 3}
    if stats_db:
        import sqlite3
        kern = {}
        for name, calls, avg in sqlite3.connect(stats_db).execute('select name, count(*), avg("end" - start) from kernels group by name'):
            for short in ('stats_chunk_kernel', 'stats_fold_kernel', 'ovl_xmax_kernel', 'ovl_contrast_kernel', 'ovl_minmax_kernel', 'img_scale_kernel',
                          'ovl_write_kernel'):
                if short + '(' in name:
                    kern[short] = {'calls': int(calls), 'avg_us': float(avg) / 1e3}
        out['kernels'] = kern
        if 'stats_chunk_kernel' in kern:
            # one call of each set per chunk pass: params and grads both read n_el floats
            per_set_us = kern['stats_chunk_kernel']['avg_us'] + kern.get('stats_fold_kernel', {'avg_us': 0})['avg_us']
            out['stats_kernels_per_set_us'] = per_set_us
            out['stats_kernels_both_sets_ms'] = 2 * per_set_us / 1e3
            out['stats_TBps'] = n_el * 4 / (per_set_us * 1e-6) / 1e12
            out['stats_share_of_hbm_peak'] = out['stats_TBps'] / HBM_PEAK_TBPS
    with open(os.path.join(outdir, 'summary_time.json'), 'w') as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out, indent=1))


if __name__ == '__main__':
    main()
