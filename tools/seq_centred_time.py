"""Times the flow-centred sequence stages: jcm_seq_filter_centred and jcm_seq_viterbi_centred beside jcm_seq_filter_moving and
jcm_seq_viterbi_moving at the C ABI, in the same run and on the same maps -- the tower's geometry (60x90, K = 9, R = 5, sigma 1.5, rho 0.05), one
clip of 256 frames (nine work groups) and sixteen clips of 64 frames (144 work groups).  The table holds one shift per block of 10 x 10 cells, drawn
from {-2 .. 2} cells per axis; the `_uniform` arms run the centred entries on a table that carries the moving arm's per-frame shift in every cell,
which separates the cost of the larger window -- (2R+1)^2 reads of the belief plane per cell against 2 (2R+1) -- from that of lanes whose LDS
addresses diverge.  Beside them the forward that produces such maps (Engine.forward with the spatial model on 16 byte images, full-width synthetic
parameters), so that every figure can be read against a forward's time per frame from the same run.  The arms are alternated block by block; every
arm is warmed up, then timed in blocks of `inner` calls between two device events; the figures are per call (median over the blocks, minimum,
90th percentile) and, derived from the medians, microseconds per frame and the ratio to the moving entry.  Writes <outdir>/<name>.json.
    python tools/seq_centred_time.py <outdir> [blocks=10] [inner=3] [--name seq_centred_time]"""
import ctypes
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import joint_cnn_mrf_amd  # noqa: F401,E402
from joint_cnn_mrf_amd import _lib, predict, synth  # noqa: E402
from joint_cnn_mrf_amd.engine import Engine  # noqa: E402
from mirror_time import alternate  # noqa: E402

HH, WW, K, R, SIGMA, RHO = 60, 90, 9, 5, 1.5, 0.05
SHAPES = ((1, 256), (16, 64))      # (S, T)
SHIFT_MAX, BLOCK, FORWARD_BATCH = 2, 10, 16


def main():
    argv = sys.argv[1:]
    name = 'seq_centred_time'
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
    rs = np.random.RandomState(5)
    arms, keep, frames_of = {}, [], {}
    for S, T in SHAPES:
        tag = 'S%d_T%d' % (S, T)
        sh = rs.randint(-SHIFT_MAX, SHIFT_MAX + 1, (S, T, 2))
        sh[(sh == 0).all(axis=2)] = (SHIFT_MAX, -SHIFT_MAX)
        coarse = rs.randint(-SHIFT_MAX, SHIFT_MAX + 1, (S, T, HH // BLOCK, WW // BLOCK, 2))
        table = np.repeat(np.repeat(coarse, BLOCK, axis=2), BLOCK, axis=3)
        shift = torch.as_tensor(sh.astype(np.int32), device='cuda:0')
        centre = torch.as_tensor(table.astype(np.int32), device='cuda:0')
        uniform = shift[:, :, None, None, :].expand(S, T, HH, WW, 2).contiguous()
        hm = torch.rand((S, T, HH, WW, K), device='cuda:0') ** 8
        hm /= hm.sum(dim=(2, 3), keepdim=True)
        filtered = torch.empty_like(hm)
        coords = torch.empty((S, T, 2, K), dtype=torch.int32, device='cuda:0')
        value = torch.empty((S, T, K), dtype=torch.float64, device='cuda:0')
        flag = torch.empty((S, T, K), dtype=torch.int32, device='cuda:0')
        state = torch.empty((S, K, HH, WW), dtype=torch.float64, device='cuda:0')
        keep.append((shift, centre, uniform, hm, filtered, coords, value, flag, state))

        def filter_moving(S=S, T=T, hm=hm, shift=shift, filtered=filtered, coords=coords, value=value, flag=flag, state=state):
            return lib.jcm_seq_filter_moving(h, p(hm), S, T, HH, WW, K, tp, R, RHO, p(shift), p(None), p(filtered), p(coords), p(value), p(flag), p(state))

        def filter_centred(table=centre, S=S, T=T, hm=hm, filtered=filtered, coords=coords, value=value, flag=flag, state=state):
            return lib.jcm_seq_filter_centred(h, p(hm), S, T, HH, WW, K, tp, R, RHO, p(table), p(None), p(filtered), p(coords), p(value), p(flag), p(state))

        def viterbi_moving(S=S, T=T, hm=hm, shift=shift, coords=coords, value=value, flag=flag):
            return lib.jcm_seq_viterbi_moving(h, p(hm), S, T, HH, WW, K, tp, R, RHO, p(shift), p(coords), p(value), p(flag))

        def viterbi_centred(table=centre, S=S, T=T, hm=hm, coords=coords, value=value, flag=flag):
            return lib.jcm_seq_viterbi_centred(h, p(hm), S, T, HH, WW, K, tp, R, RHO, p(table), p(coords), p(value), p(flag))
        # the timed calls do the work: on the uniform table the centred entries give the bits of the moving ones
        _lib.check(filter_moving(), 'jcm_seq_filter_moving')
        want = (filtered.clone(), coords.clone(), value.clone())
        _lib.check(filter_centred(uniform), 'jcm_seq_filter_centred')
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(want, (filtered, coords, value))), tag
        _lib.check(viterbi_moving(), 'jcm_seq_viterbi_moving')
        want = (coords.clone(), value.clone())
        _lib.check(viterbi_centred(uniform), 'jcm_seq_viterbi_centred')
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(want, (coords, value))), tag
        _lib.check(filter_centred(), 'jcm_seq_filter_centred')
        _lib.check(viterbi_centred(), 'jcm_seq_viterbi_centred')
        arms.update({'seq_filter_moving_' + tag: filter_moving, 'seq_filter_centred_' + tag: filter_centred,
                     'seq_filter_centred_uniform_' + tag: lambda f=filter_centred, u=uniform: f(u),
                     'seq_viterbi_moving_' + tag: viterbi_moving, 'seq_viterbi_centred_' + tag: viterbi_centred,
                     'seq_viterbi_centred_uniform_' + tag: lambda f=viterbi_centred, u=uniform: f(u)})
        frames_of[tag] = S * T
    xf = torch.randint(0, 256, (FORWARD_BATCH, 480, 720, 3), dtype=torch.uint8, device='cuda:0')
    arms['forward_16_frames'] = lambda: eng.forward(xf, 'infer', use_sm=True)
    torch.cuda.synchronize()
    t = alternate(arms, blocks, inner)
    fwd = t['forward_16_frames']['device_events']['median_us'] / FORWARD_BATCH
    per_frame = {'forward': fwd}
    per_frame.update({arm: t[arm]['device_events']['median_us'] / frames_of[arm[arm.index('_S') + 1:]] for arm in arms if arm != 'forward_16_frames'})
    ratio = {arm: per_frame[arm] / per_frame[arm.replace('_centred_uniform', '_moving').replace('_centred', '_moving')] for arm in per_frame if '_centred' in arm}
    res = {'device': torch.cuda.get_device_name(0), 'blocks': blocks, 'calls_per_block': inner, 'map': [HH, WW], 'K': K, 'R': R, 'sigma': SIGMA, 'rho': RHO,
           'shapes_S_T': [list(s) for s in SHAPES], 'shift_cells': [-SHIFT_MAX, SHIFT_MAX], 'table_block_cells': BLOCK, 'forward_batch': FORWARD_BATCH,
           'lds_reads_of_the_belief_plane_per_cell': {'moving': 2 * (2 * R + 1), 'centred': (2 * R + 1) ** 2}, 'kernels': t,
           'us_per_frame_at_median': per_frame, 'ratio_to_moving_per_frame': ratio,
           'ratio_to_forward_per_frame': {k: v / fwd for k, v in per_frame.items() if k != 'forward'}}
    eng.close()
    print(json.dumps({k: res[k] for k in ('us_per_frame_at_median', 'ratio_to_moving_per_frame')}), flush=True)
    with open(os.path.join(outdir, name + '.json'), 'w') as fh:
        json.dump(res, fh, indent=1)


if __name__ == '__main__':
    main()
