"""Times the local motion: jcm_frame_flow and jcm_hm_flow_pool at the C ABI on 16 and on 256 byte frames of 480x720 (the whole
frame as the content rectangle, D = 8, N = 2: four reference frames a frame, motion.flow_refs), beside jcm_frame_shift on the same frames, a device
copy of the same bytes and the forward that reads such frames -- Engine.forward with the spatial model on 16 byte images, full-width synthetic
parameters -- in the same run, the arms alternated.  The frames are crops of one box-filtered canvas that pans by a few pixels a frame, so the
search does the work it does on a clip; the maps are random.  Every arm is warmed up, then timed in blocks of `inner` calls between two device
events; the figures are per call (median over the blocks, minimum, 90th percentile) and, derived from the medians, microseconds per frame and the
ratio to the forward's time per frame.  Writes <outdir>/<name>.json.
    python tools/frame_flow_time.py <outdir> [blocks=10] [inner=3] [--name frame_flow_time]"""
import ctypes
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import joint_cnn_mrf_amd  # noqa: F401,E402
from joint_cnn_mrf_amd import _lib, motion, synth  # noqa: E402
from joint_cnn_mrf_amd.engine import Engine  # noqa: E402
from frame_shift_time import panned  # noqa: E402
from mirror_time import alternate  # noqa: E402

H, W, D, N, K = 480, 720, 8, 2, 9
SHAPES = (16, 256)
FORWARD_BATCH = 16


def main():
    argv = sys.argv[1:]
    name = 'frame_flow_time'
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
    HH, WW = H // 8, W // 8
    w = (ctypes.c_double * (N + 1))(*motion.flow_weights(N))
    arms, keep, checked = {}, [], {}
    for T in SHAPES:
        frames, true = panned(T, eng.device)
        x, prev = frames[1:], frames[0]
        ref = torch.as_tensor(motion.flow_refs(T, N), device=eng.device)
        flow = torch.empty((T, 2 * N, HH, WW, 2), dtype=torch.int32, device=eng.device)
        sad = torch.empty_like(flow)
        hm = torch.rand((T, HH, WW, K), device=eng.device)
        out = torch.empty_like(hm)
        disp = torch.empty((T, 2), dtype=torch.int32, device=eng.device)
        sad64 = torch.empty((T, 2), dtype=torch.int64, device=eng.device)
        dst = torch.empty_like(x)
        keep.append((frames, ref, flow, sad, hm, out, disp, sad64, dst))

        def run_flow(x=x, T=T, ref=ref, flow=flow, sad=sad):
            return lib.jcm_frame_flow(h, p(x), T, H, W, 0, 0, H, W, D, p(ref), 2 * N, p(flow), p(sad))

        def run_pool(hm=hm, T=T, flow=flow, out=out):
            return lib.jcm_hm_flow_pool(h, p(hm), T, HH, WW, K, p(flow), N, w, p(out))

        def run_shift(x=x, prev=prev, T=T, disp=disp, sad64=sad64):
            return lib.jcm_frame_shift(h, p(x), T, H, W, 0, 0, H, W, D, p(prev), p(disp), p(sad64))
        _lib.check(run_flow(), 'jcm_frame_flow')
        _lib.check(run_pool(), 'jcm_hm_flow_pool')
        _lib.check(run_shift(), 'jcm_frame_shift')
        torch.cuda.synchronize()
        # the timed call does the work: away from the border, the cells of frame t find the pan of frame t against frame t-1 (slot 0 of frames >= 1)
        small = np.abs(true[1:]).max(axis=1) <= D
        got = flow[1:, 0, 8:-8, 8:-8].cpu().numpy()
        checked['T%d' % T] = float((got == true[1:, None, None, :])[small].all(axis=-1).mean())
        arms['frame_flow_T%d' % T] = run_flow
        arms['hm_flow_pool_T%d' % T] = run_pool
        arms['frame_shift_T%d' % T] = run_shift
        arms['copy_T%d' % T] = lambda x=x, dst=dst: dst.copy_(x)
    xf = torch.randint(0, 256, (FORWARD_BATCH, H, W, 3), dtype=torch.uint8, device=eng.device)
    arms['forward_16_frames'] = lambda: eng.forward(xf, 'infer', use_sm=True)
    torch.cuda.synchronize()
    t = alternate(arms, blocks, inner)
    fwd = t['forward_16_frames']['device_events']['median_us'] / FORWARD_BATCH
    per_frame = {'forward': fwd}
    for T in SHAPES:
        for kind in ('frame_flow_T%d', 'hm_flow_pool_T%d', 'frame_shift_T%d', 'copy_T%d'):
            per_frame[kind % T] = t[kind % T]['device_events']['median_us'] / T
    res = {'device': torch.cuda.get_device_name(0), 'blocks': blocks, 'calls_per_block': inner, 'frame': [H, W], 'D': D, 'N': N, 'K': K, 'frames': list(SHAPES),
           'forward_batch': FORWARD_BATCH, 'cells_that_find_the_pan': checked, 'kernels': t, 'us_per_frame_at_median': per_frame,
           'ratio_to_forward_per_frame': {k: v / fwd for k, v in per_frame.items() if k != 'forward'},
           'bytes_read_per_frame': H * W * 3, 'workspace_bytes_per_frame': H * W * 2}
    eng.close()
    print(json.dumps(res), flush=True)
    with open(os.path.join(outdir, name + '.json'), 'w') as fh:
        json.dump(res, fh, indent=1)


if __name__ == '__main__':
    main()
