"""Times the smoother: jcm_seq_smooth beside jcm_seq_filter and jcm_seq_viterbi at the C ABI on the same heat maps of the tower's
geometry (60x90, K = 9, R = 5, sigma 1.5, rho 0.05) for one long clip (S = 1, T = 256) and for sixteen clips (S = 16, T = 64), one iteration of
predict.seq_fit's EM at radius 16 (one jcm_seq_smooth without the smoothed maps, its statistics read back and the M-step on the host) on the
sixteen clips, and the forward that makes such maps -- Engine.forward with the spatial model on 16 byte images of 480x720 -- alternated in one
run as tools/seq_time.py does.  The figures are per call (median over the blocks, minimum, 90th percentile) and, derived from the medians,
microseconds per frame, the ratio to the filter on the same maps and the ratio to the forward's time per frame.  The EM iteration's device-event
time leaves out its host part; its wall time is reported beside it.
Writes <outdir>/<name>.json.
    python tools/seq_smooth_time.py <outdir> [blocks=10] [inner=3] [--name seq_smooth_time]"""
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import joint_cnn_mrf_amd  # noqa: F401,E402
from joint_cnn_mrf_amd import _lib, predict, synth  # noqa: E402
from joint_cnn_mrf_amd.engine import Engine  # noqa: E402
from mirror_time import alternate  # noqa: E402

HH, WW, K, R, SIGMA, RHO = 60, 90, 9, 5, 1.5, 0.05
SHAPES = {'S1_T256': (1, 256), 'S16_T64': (16, 64)}
FORWARD_BATCH = 16
FIT_RADIUS = 16


def main():
    argv = sys.argv[1:]
    name = 'seq_smooth_time'
    if '--name' in argv:
        i = argv.index('--name')
        name = argv[i + 1]
        del argv[i:i + 2]
    if not argv or any(a.startswith('--') for a in argv):
        sys.exit(__doc__)
    outdir = argv[0]
    blocks = int(argv[1]) if len(argv) > 1 else 10
    inner = int(argv[2]) if len(argv) > 2 else 3
    os.makedirs(outdir, exist_ok=True)
    params = synth.make_pd_params(debug=False)
    params.update(synth.make_sm_params(synth.synthetic_priors(), kind='init'))
    eng = Engine(device=0).load_params(params)
    lib, h, p = eng._lib, eng._h, eng._p
    taps = predict.seq_taps(SIGMA, R, K)
    tp = taps.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    arms, keep = {}, []
    for tag, (S, T) in SHAPES.items():
        hm = torch.rand((S, T, HH, WW, K), device='cuda:0') ** 8
        hm /= hm.sum(dim=(2, 3), keepdim=True)
        maps = torch.empty_like(hm)
        coords = torch.empty((S, T, 2, K), dtype=torch.int32, device='cuda:0')
        conf = torch.empty((S, T, K), device='cuda:0')
        value, mass = (torch.empty((S, T, K), dtype=torch.float64, device='cuda:0') for _ in range(2))
        flag, cut = (torch.empty((S, T, K), dtype=torch.int32, device='cuda:0') for _ in range(2))
        trans = torch.empty((S, T, K, 3), dtype=torch.float64, device='cuda:0')
        state = torch.empty((S, K, HH, WW), dtype=torch.float64, device='cuda:0')
        keep.append((hm, maps, coords, conf, value, mass, flag, cut, trans, state))

        def run_filter(hm=hm, S=S, T=T, maps=maps, coords=coords, value=value, flag=flag, state=state):
            return lib.jcm_seq_filter(h, p(hm), S, T, HH, WW, K, tp, R, RHO, p(None), p(maps), p(coords), p(value), p(flag), p(state))

        def run_viterbi(hm=hm, S=S, T=T, coords=coords, value=value, flag=flag):
            return lib.jcm_seq_viterbi(h, p(hm), S, T, HH, WW, K, tp, R, RHO, p(coords), p(value), p(flag))

        def run_smooth(hm=hm, S=S, T=T, maps=maps, coords=coords, conf=conf, value=value, flag=flag, mass=mass, cut=cut, trans=trans):
            return lib.jcm_seq_smooth(h, p(hm), S, T, HH, WW, K, tp, R, RHO, p(maps), p(coords), p(conf), p(value), p(flag), p(mass), p(cut), p(trans))
        _lib.check(run_filter(), 'jcm_seq_filter')
        _lib.check(run_viterbi(), 'jcm_seq_viterbi')
        _lib.check(run_smooth(), 'jcm_seq_smooth')
        arms['seq_filter_' + tag], arms['seq_viterbi_' + tag], arms['seq_smooth_' + tag] = run_filter, run_viterbi, run_smooth
    fit_hm = keep[-1][0]
    wall = []

    def run_fit_iteration():
        t0 = time.perf_counter()
        r = eng.seq_smooth(fit_hm, SIGMA, RHO, radius=FIT_RADIUS, want_smoothed=False)
        predict.seq_m_step(r['trans'].cpu().numpy().reshape(-1, K, 3).sum(axis=0), np.full(K, SIGMA), RHO, FIT_RADIUS)
        wall.append(time.perf_counter() - t0)
    run_fit_iteration()
    arms['seq_fit_iteration_R16_S16_T64'] = run_fit_iteration
    x = torch.randint(0, 256, (FORWARD_BATCH, 480, 720, 3), dtype=torch.uint8, device='cuda:0')
    arms['forward_16_frames'] = lambda: eng.forward(x, 'infer', use_sm=True)
    torch.cuda.synchronize()
    del wall[:]
    t = alternate(arms, blocks, inner)
    fwd = t['forward_16_frames']['device_events']['median_us'] / FORWARD_BATCH
    per_frame = {'forward': fwd}
    for tag, (S, T) in SHAPES.items():
        for kind in ('seq_filter_', 'seq_viterbi_', 'seq_smooth_'):
            per_frame[kind + tag] = t[kind + tag]['device_events']['median_us'] / (S * T)
    S, T = SHAPES['S16_T64']
    per_frame['seq_fit_iteration_R16_S16_T64'] = t['seq_fit_iteration_R16_S16_T64']['device_events']['median_us'] / (S * T)
    res = {'device': torch.cuda.get_device_name(0), 'blocks': blocks, 'calls_per_block': inner, 'map': [HH, WW], 'K': K, 'R': R, 'sigma': SIGMA, 'rho': RHO,
           'shapes': {tag: {'S': S, 'T': T, 'work_groups': S * K} for tag, (S, T) in SHAPES.items()}, 'forward_batch': FORWARD_BATCH, 'kernels': t,
           'us_per_frame_at_median': per_frame, 'ratio_to_forward_per_frame': {k: v / fwd for k, v in per_frame.items() if k != 'forward'},
           'smooth_to_filter': {tag: per_frame['seq_smooth_' + tag] / per_frame['seq_filter_' + tag] for tag in SHAPES},
           'fit_iteration': {'radius': FIT_RADIUS, 'wall_ms_median': 1e3 * float(np.median(wall)), 'calls': len(wall)},
           'kernel_shape': {'threads': 1024, 'lds_bytes_forward': 2 * HH * WW * 8, 'lds_bytes_backward': 3 * HH * WW * 8,
                            'belief_bytes': {tag: S * K * T * HH * WW * 8 for tag, (S, T) in SHAPES.items()}}}
    eng.close()
    print(json.dumps(res), flush=True)
    with open(os.path.join(outdir, name + '.json'), 'w') as fh:
        json.dump(res, fh, indent=1)


if __name__ == '__main__':
    main()
