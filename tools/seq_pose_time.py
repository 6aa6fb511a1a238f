"""Times the clip decode: jcm_seq_pose_viterbi at the C ABI at P = 2, 3 and 4 candidates per joint, on one clip of 256 frames (one
work group) and on sixteen clips of 64 frames (sixteen work groups), random tables with every count P and a finite tau (no break: every frame runs
its nine passes).  Beside it, alternated in the same run: jcm_pose_decode on the same number of frames (random 60x90x10 maps, random candidate
cells), jcm_seq_viterbi on 60x90x9 maps of the same clip shapes (R = 5, sigma 1.5, rho 0.05), and the forward that produces such maps
(Engine.forward with the spatial model on 16 byte images, full-width synthetic parameters).  Every arm is warmed up, then timed in blocks of `inner`
calls between two device events; the figures are per call (median over the blocks, minimum, 90th percentile) and, derived from the medians,
microseconds per frame; the workspace bytes per frame of the clip decode are stated beside them.  Writes <outdir>/<name>.json.
    python tools/seq_pose_time.py <outdir> [blocks=5] [inner=2] [--name seq_pose_time]"""
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
PEAKS = (2, 3, 4)
FORWARD_BATCH = 16


def main():
    argv = sys.argv[1:]
    name = 'seq_pose_time'
    if '--name' in argv:
        i = argv.index('--name')
        name = argv[i + 1]
        del argv[i:i + 2]
    if not argv or any(a.startswith('--') for a in argv):
        sys.exit(__doc__)
    outdir = argv[0]
    blocks = int(argv[1]) if len(argv) > 1 else 5
    inner = int(argv[2]) if len(argv) > 2 else 2
    os.makedirs(outdir, exist_ok=True)
    params = synth.make_pd_params(debug=False)
    params.update(synth.make_sm_params(synth.synthetic_priors(), kind='init'))
    eng = Engine(device=0).load_params(params)
    lib, h, p = eng._lib, eng._h, eng._p
    taps = predict.seq_taps(SIGMA, R, K)
    tp = taps.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    rs = np.random.RandomState(5)
    dev = lambda a: torch.as_tensor(np.ascontiguousarray(a), device='cuda:0')
    arms, keep, frames_of = {}, [], {}
    for S, T in SHAPES:
        tag = 'S%d_T%d' % (S, T)
        hm = torch.rand((S, T, HH, WW, K), device='cuda:0') ** 8
        hm /= hm.sum(dim=(2, 3), keepdim=True)
        hm10 = torch.cat([hm, torch.rand((S, T, HH, WW, 1), device='cuda:0')], dim=4).view(S * T, HH, WW, K + 1).contiguous()
        path = torch.empty((S, T, 2, K), dtype=torch.int32, device='cuda:0')
        value = torch.empty((S, T, K), dtype=torch.float64, device='cuda:0')
        flag = torch.empty((S, T, K), dtype=torch.int32, device='cuda:0')
        keep.append((hm, hm10, path, value, flag))

        def viterbi(S=S, T=T, hm=hm, path=path, value=value, flag=flag):
            return lib.jcm_seq_viterbi(h, p(hm), S, T, HH, WW, K, tp, R, RHO, p(path), p(value), p(flag))
        _lib.check(viterbi(), 'jcm_seq_viterbi')
        arms['seq_viterbi_' + tag] = viterbi
        frames_of['seq_viterbi_' + tag] = S * T
        for P in PEAKS:
            B = S * T
            flat = np.stack([rs.choice(HH * WW, P, replace=False) for _ in range(B * K)]).reshape(B, K, P)
            cells = dev(np.stack([flat // WW, flat % WW], axis=3).astype(np.int32))
            count = dev(np.full((B, K), P, np.int32))
            V = torch.empty((B, K, P), device='cuda:0')
            M = torch.empty((B, 36, P, P), device='cuda:0')
            tau = dev(rs.standard_normal((B, K, P, P)))
            index = torch.empty((B, K), dtype=torch.int32, device='cuda:0')
            coords = torch.empty((B, 2, K), dtype=torch.int32, device='cuda:0')
            score = torch.empty((B,), device='cuda:0')
            score0 = torch.empty((B,), device='cuda:0')
            maxes = torch.empty((B,), dtype=torch.float64, device='cuda:0')
            breaks = torch.empty((B,), dtype=torch.int32, device='cuda:0')
            keep.append((cells, count, V, M, tau, index, coords, score, score0, maxes, breaks))

            def decode(hm10=hm10, B=B, P=P, cells=cells, count=count, V=V, M=M, index=index, coords=coords, score=score, score0=score0):
                return lib.jcm_pose_decode(h, p(hm10), B, p(cells), p(count), P, p(index), p(coords), p(score), p(score0), p(V), p(M))

            def clip(S=S, T=T, P=P, cells=cells, count=count, V=V, M=M, tau=tau, index=index, coords=coords, score=score, maxes=maxes, breaks=breaks):
                return lib.jcm_seq_pose_viterbi(h, p(V), p(M), p(count), p(cells), p(tau), S, T, P, p(index), p(coords), p(score), p(maxes), p(breaks))
            _lib.check(decode(), 'jcm_pose_decode')      # fills V and M for the clip decode
            _lib.check(clip(), 'jcm_seq_pose_viterbi')
            torch.cuda.synchronize()
            assert int(breaks.max()) == 0 and int(index.min()) >= 0, (tag, P)
            for arm, fn in (('pose_decode_P%d_%s' % (P, tag), decode), ('seq_pose_viterbi_P%d_%s' % (P, tag), clip)):
                arms[arm] = fn
                frames_of[arm] = B
    xf = torch.randint(0, 256, (FORWARD_BATCH, 480, 720, 3), dtype=torch.uint8, device='cuda:0')
    arms['forward_16_frames'] = lambda: eng.forward(xf, 'infer', use_sm=True)
    frames_of['forward_16_frames'] = FORWARD_BATCH
    torch.cuda.synchronize()
    t = alternate(arms, blocks, inner)
    per_frame = {arm: t[arm]['device_events']['median_us'] / frames_of[arm] for arm in arms}
    res = {'device': torch.cuda.get_device_name(0), 'blocks': blocks, 'calls_per_block': inner, 'map': [HH, WW], 'K': K, 'R': R, 'sigma': SIGMA, 'rho': RHO,
           'shapes_S_T': [list(s) for s in SHAPES], 'peaks': list(PEAKS), 'forward_batch': FORWARD_BATCH,
           'workspace_bytes_per_frame': {'P%d' % P: 3 * P ** 9 + 8 for P in PEAKS}, 'workspace_bytes_per_clip': {'P%d' % P: 8 * P ** 9 for P in PEAKS},
           'kernels': t, 'us_per_frame_at_median': per_frame}
    eng.close()
    print(json.dumps(res['us_per_frame_at_median']), flush=True)
    with open(os.path.join(outdir, name + '.json'), 'w') as fh:
        json.dump(res, fh, indent=1)


if __name__ == '__main__':
    main()
