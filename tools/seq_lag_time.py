"""Times the fixed-lag smoother on one clip of the tower's geometry (60x90, K = 9, R = 5, sigma 1.5, rho 0.05), device events, the
arms alternated in one process as tools/seq_smooth_time.py alternates them:
  one-frame pushes of jcm_seq_smooth_lag in the steady state (a window of L pending frames and one new one, one frame emitted) at L = 4, 8, 16,
    at the C ABI, and the same push through Engine.seq_smooth_lag, which also assembles and cuts the window with device copies;
  one-frame pushes of jcm_seq_filter with its carried state;
  the offline jcm_seq_filter and jcm_seq_smooth over the whole clip (S = 1, T = 256), per frame;
  one flushed jcm_seq_smooth_lag call over the 256 frames at L = 8, where 9 * 256 work groups run the backward pass.
For each L the yardstick is filter + L * (smooth - filter) per frame from the OFFLINE entries of the same run -- a forward step and L backward
steps at the cost they have inside the one-group-per-joint kernels -- and the ratio of the push to it is reported.
Writes <outdir>/<name>.json.
    python tools/seq_lag_time.py <outdir> [blocks=10] [inner=3] [--name seq_lag_time]"""
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

HH, WW, K, R, SIGMA, RHO = 60, 90, 9, 5, 1.5, 0.05
T = 256
LAGS = (4, 8, 16)
FLUSH_LAG = 8


def main():
    argv = sys.argv[1:]
    name = 'seq_lag_time'
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
    taps = predict.seq_taps(SIGMA, R, K)
    tp = taps.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    new = lambda shape, dtype=torch.float32: torch.empty(shape, dtype=dtype, device='cuda:0')
    hm = torch.rand((1, T, HH, WW, K), device='cuda:0') ** 8
    hm /= hm.sum(dim=(2, 3), keepdim=True)
    maps, coords, conf = new((1, T, HH, WW, K)), new((1, T, 2, K), torch.int32), new((1, T, K))
    value, mass = new((1, T, K), torch.float64), new((1, T, K), torch.float64)
    flag, cut = new((1, T, K), torch.int32), new((1, T, K), torch.int32)
    state = new((1, K, HH, WW), torch.float64)
    belief = new((K, T, HH * WW), torch.float64)
    arms = {}

    def run_filter():
        return lib.jcm_seq_filter(h, p(hm), 1, T, HH, WW, K, tp, R, RHO, p(None), p(maps), p(coords), p(value), p(flag), p(state))

    def run_smooth():
        return lib.jcm_seq_smooth(h, p(hm), 1, T, HH, WW, K, tp, R, RHO, p(maps), p(coords), p(conf), p(value), p(flag), p(mass), p(cut), p(None))

    def run_filter_push():      # frame 1 from the state frame 0 left
        return lib.jcm_seq_filter(h, p(hm[:, 1:2]), 1, 1, HH, WW, K, tp, R, RHO, p(state), p(maps), p(coords), p(value), p(flag), p(state2))

    def run_flush():
        return lib.jcm_seq_smooth_lag(h, p(hm), 1, T, 0, HH, WW, K, tp, R, RHO, FLUSH_LAG, 1, p(belief), p(value), p(flag), p(maps), p(coords), p(conf), p(mass),
                                      p(cut))
    state2 = torch.empty_like(state)
    _lib.check(lib.jcm_seq_filter(h, p(hm), 1, 1, HH, WW, K, tp, R, RHO, p(None), p(maps), p(coords), p(value), p(flag), p(state)), 'jcm_seq_filter')
    _lib.check(run_filter_push(), 'jcm_seq_filter')
    arms['seq_filter_push'] = run_filter_push
    keep = []
    for L in LAGS:
        W = L + 1
        win = (hm[:, :W].contiguous(), new((K, W, HH * WW), torch.float64), new((1, W, K), torch.float64), new((1, W, K), torch.int32))
        out = (new((1, 1, HH, WW, K)), new((1, 1, 2, K), torch.int32), new((1, 1, K)), new((1, 1, K), torch.float64), new((1, 1, K), torch.int32))
        keep.append((win, out))

        def run_push(P=L, L=L, W=W, win=win, out=out):      # P = L: the steady state; P = 0 fills the window first
            return lib.jcm_seq_smooth_lag(h, p(win[0]), 1, W, P, HH, WW, K, tp, R, RHO, L, 0, p(win[1]), p(win[2]), p(win[3]), *(p(o) for o in out))
        _lib.check(run_push(P=0), 'jcm_seq_smooth_lag')
        _lib.check(run_push(), 'jcm_seq_smooth_lag')
        arms['seq_lag_push_L%d' % L] = run_push
        st = eng.seq_smooth_lag(hm[:, :L].contiguous(), SIGMA, RHO, L, radius=R)['state']
        frame = hm[:, L:W].contiguous()
        arms['engine_push_L%d' % L] = lambda st=st, frame=frame, L=L: eng.seq_smooth_lag(frame, SIGMA, RHO, L, radius=R, state=st, want_smoothed=True)
    _lib.check(run_filter(), 'jcm_seq_filter')
    _lib.check(run_smooth(), 'jcm_seq_smooth')
    _lib.check(run_flush(), 'jcm_seq_smooth_lag')
    arms['seq_filter_S1_T256'], arms['seq_smooth_S1_T256'], arms['seq_lag_flush_T256_L%d' % FLUSH_LAG] = run_filter, run_smooth, run_flush
    torch.cuda.synchronize()
    t = alternate(arms, blocks, inner)
    med = {k: v['device_events']['median_us'] for k, v in t.items()}
    flt, smo = med['seq_filter_S1_T256'] / T, med['seq_smooth_S1_T256'] / T
    pushes = {}
    for L in LAGS:
        yard = flt + L * (smo - flt)
        pushes['L%d' % L] = {'push_us': med['seq_lag_push_L%d' % L], 'engine_push_us': med['engine_push_L%d' % L], 'yardstick_us': yard,
                             'push_to_yardstick': med['seq_lag_push_L%d' % L] / yard, 'engine_push_to_yardstick': med['engine_push_L%d' % L] / yard,
                             'push_to_filter_push': med['seq_lag_push_L%d' % L] / med['seq_filter_push'], 'backward_work_groups': K,
                             'window_bytes': (L + 1) * HH * WW * K * (4 + 8)}
    flush_pf = med['seq_lag_flush_T256_L%d' % FLUSH_LAG] / T
    yard = flt + FLUSH_LAG * (smo - flt)
    res = {'device': torch.cuda.get_device_name(0), 'blocks': blocks, 'calls_per_block': inner, 'map': [HH, WW], 'K': K, 'R': R, 'sigma': SIGMA, 'rho': RHO, 'T': T,
           'kernels': t, 'us_per_frame_at_median': {'seq_filter_offline': flt, 'seq_smooth_offline': smo, 'seq_filter_push': med['seq_filter_push'],
                                                    'seq_lag_flush_T256_L%d' % FLUSH_LAG: flush_pf},
           'pushes': pushes, 'flush': {'L': FLUSH_LAG, 'E': T, 'backward_work_groups': K * T, 'us_per_frame': flush_pf, 'yardstick_us': yard,
                                       'flush_to_yardstick': flush_pf / yard, 'flush_to_smooth_offline': flush_pf / smo},
           'kernel_shape': {'threads': 1024, 'lds_bytes_forward': 2 * HH * WW * 8, 'lds_bytes_backward': 3 * HH * WW * 8, 'groups_per_cu': 1}}
    eng.close()
    print(json.dumps(res), flush=True)
    with open(os.path.join(outdir, name + '.json'), 'w') as fh:
        json.dump(res, fh, indent=1)


if __name__ == '__main__':
    main()
