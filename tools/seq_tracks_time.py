"""Times the torso tracks: jcm_seq_tracks_viterbi and jcm_seq_tracks_filter at the C ABI at M = 4 on single-channel maps of the
tower's geometry (60x90, R = 5, sigma 1.5, rho 0.05, D = 4) for one long clip (S = 1, T = 256) and for sixteen clips (S = 16, T = 64).  The
comparison arm is what the four passes cost without the exclusion: FOUR back-to-back calls of jcm_seq_viterbi / jcm_seq_filter at K = 1 on the
same maps, in the same run, the arms alternating.  Every arm is warmed up, then timed in blocks of `inner` calls between two device events; the
figures are per call (median over the blocks, minimum, 90th percentile), the ratio of the medians, and the spread (p90 / median) of each
comparison arm, which is what the ratio is to be read against.
Writes <outdir>/<name>.json.
    python tools/seq_tracks_time.py <outdir> [blocks=10] [inner=3] [--name seq_tracks_time]"""
import ctypes
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import joint_cnn_mrf_amd  # noqa: F401,E402
from joint_cnn_mrf_amd import _lib, predict  # noqa: E402
from joint_cnn_mrf_amd.engine import Engine  # noqa: E402
from mirror_time import alternate  # noqa: E402

HH, WW, M, R, D, SIGMA, RHO = 60, 90, 4, 5, 4, 1.5, 0.05
SHAPES = {'S1_T256': (1, 256), 'S16_T64': (16, 64)}


def main():
    argv = sys.argv[1:]
    name = 'seq_tracks_time'
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
    eng = Engine(device=0)
    lib, h, p = eng._lib, eng._h, eng._p
    taps = predict.seq_taps(SIGMA, R, 1)
    tp = taps.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    arms, keep = {}, []
    for tag, (S, T) in SHAPES.items():
        hm = torch.rand((S, T, HH, WW), device='cuda:0') ** 8
        hm /= hm.sum(dim=(2, 3), keepdim=True)
        i32, f64 = dict(dtype=torch.int32, device='cuda:0'), dict(dtype=torch.float64, device='cuda:0')
        cells, num, flag, value = torch.empty((S, M, T, 2), **i32), torch.empty((S, M, T), **f64), torch.empty((S, M, T), **i32), torch.empty((S, M, T), device='cuda:0')
        state = torch.empty((S, M, HH * WW), **f64)
        keep.append((hm, cells, num, flag, value, state))

        def tracks_filter(hm=hm, S=S, T=T, cells=cells, num=num, flag=flag, value=value, state=state):
            return lib.jcm_seq_tracks_filter(h, p(hm), S, T, HH, WW, M, tp, R, RHO, D, p(None), p(None), p(cells), p(num), p(flag), p(state), p(value))

        def tracks_viterbi(hm=hm, S=S, T=T, cells=cells, num=num, flag=flag, value=value):
            return lib.jcm_seq_tracks_viterbi(h, p(hm), S, T, HH, WW, M, tp, R, RHO, D, p(cells), p(num), p(flag), p(value))

        def four_filters(hm=hm, S=S, T=T, cells=cells, num=num, flag=flag, state=state):
            rc = 0
            for _ in range(M):
                rc |= lib.jcm_seq_filter(h, p(hm), S, T, HH, WW, 1, tp, R, RHO, p(None), p(None), p(cells), p(num), p(flag), p(state))
            return rc

        def four_viterbis(hm=hm, S=S, T=T, cells=cells, num=num, flag=flag):
            rc = 0
            for _ in range(M):
                rc |= lib.jcm_seq_viterbi(h, p(hm), S, T, HH, WW, 1, tp, R, RHO, p(cells), p(num), p(flag))
            return rc
        for fn in (tracks_filter, tracks_viterbi, four_filters, four_viterbis):
            _lib.check(fn(), fn.__name__)
            arms['%s_%s' % (fn.__name__, tag)] = fn
    torch.cuda.synchronize()
    t = alternate(arms, blocks, inner)
    med = {k: v['device_events']['median_us'] for k, v in t.items()}
    ratio, spread = {}, {}
    for tag in SHAPES:
        for kind, base in (('tracks_filter_', 'four_filters_'), ('tracks_viterbi_', 'four_viterbis_')):
            ratio[kind + tag] = med[kind + tag] / med[base + tag]
            spread[base + tag] = t[base + tag]['device_events']['p90_us'] / med[base + tag]
    res = {'device': torch.cuda.get_device_name(0), 'blocks': blocks, 'calls_per_block': inner, 'map': [HH, WW], 'M': M, 'R': R, 'D': D, 'sigma': SIGMA, 'rho': RHO,
           'shapes': {tag: {'S': S, 'T': T, 'work_groups_per_pass': S} for tag, (S, T) in SHAPES.items()}, 'kernels': t,
           'ratio_of_medians_to_four_single_calls': ratio, 'p90_over_median_of_the_comparison_arm': spread}
    eng.close()
    print(json.dumps(res), flush=True)
    with open(os.path.join(outdir, name + '.json'), 'w') as fh:
        json.dump(res, fh, indent=1)


if __name__ == '__main__':
    main()
