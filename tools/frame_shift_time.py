"""Times the camera estimate: jcm_frame_shift at the C ABI on 16 and on 256 byte frames of 480x720 (the whole frame as the content
rectangle, D = 8, prev given, so T pairs), beside a device copy of the same bytes and beside the forward that reads such frames -- Engine.forward
with the spatial model on 16 byte images, full-width synthetic parameters -- in the same run.  The frames are crops of one box-filtered canvas that
pans by a few pixels a frame, so the search does the work it does on a clip.  Every arm is warmed up, then timed in blocks of `inner` calls between
two device events; the figures are per call (median over the blocks, minimum, 90th percentile) and, derived from the medians, microseconds per
frame and the ratio to the forward's time per frame.  Writes <outdir>/<name>.json.
    python tools/frame_shift_time.py <outdir> [blocks=10] [inner=3] [--name frame_shift_time]"""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import joint_cnn_mrf_amd  # noqa: F401,E402
from joint_cnn_mrf_amd import _lib, synth  # noqa: E402
from joint_cnn_mrf_amd.engine import Engine  # noqa: E402
from mirror_time import alternate  # noqa: E402

H, W, D = 480, 720, 8
SHAPES = (16, 256)
FORWARD_BATCH = 16


def panned(T, device):
    """T + 1 crops [H,W,3] of one smooth random canvas, each a few pixels from the one before (a device box filter: the content does not matter
    to the time, only that a best match exists where a clip has one)."""
    g = torch.Generator(device='cpu').manual_seed(T)
    raw = torch.randint(0, 256, (1, 3, H + 72, W + 72), generator=g).float()
    canvas = torch.nn.functional.avg_pool2d(raw, 9, stride=1).round().clamp(0, 255).to(torch.uint8)[0].permute(1, 2, 0).contiguous().to(device)
    rs = np.random.RandomState(T)
    o = np.clip(np.cumsum(rs.randint(-6, 7, size=(T + 1, 2)), axis=0) + 32, 0, 63)
    return torch.stack([canvas[int(y):int(y) + H, int(x):int(x) + W] for y, x in o]).contiguous(), np.diff(o, axis=0)


def main():
    argv = sys.argv[1:]
    name = 'frame_shift_time'
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
    arms, keep, checked = {}, [], {}
    for T in SHAPES:
        frames, true = panned(T, eng.device)
        x, prev = frames[1:], frames[0]
        disp = torch.empty((T, 2), dtype=torch.int32, device=eng.device)
        sad = torch.empty((T, 2), dtype=torch.int64, device=eng.device)
        dst = torch.empty_like(x)
        keep.append((frames, disp, sad, dst))

        def run(x=x, prev=prev, T=T, disp=disp, sad=sad):
            return lib.jcm_frame_shift(h, p(x), T, H, W, 0, 0, H, W, D, p(prev), p(disp), p(sad))
        _lib.check(run(), 'jcm_frame_shift')
        torch.cuda.synchronize()
        checked['T%d' % T] = bool((disp.cpu().numpy() == true).all())      # the timed call does the work: it finds the pans
        arms['frame_shift_T%d' % T] = run
        arms['copy_T%d' % T] = lambda x=x, dst=dst: dst.copy_(x)
    xf = torch.randint(0, 256, (FORWARD_BATCH, H, W, 3), dtype=torch.uint8, device=eng.device)
    arms['forward_16_frames'] = lambda: eng.forward(xf, 'infer', use_sm=True)
    torch.cuda.synchronize()
    t = alternate(arms, blocks, inner)
    fwd = t['forward_16_frames']['device_events']['median_us'] / FORWARD_BATCH
    per_frame = {'forward': fwd}
    for T in SHAPES:
        for kind in ('frame_shift_T%d', 'copy_T%d'):
            per_frame[kind % T] = t[kind % T]['device_events']['median_us'] / T
    res = {'device': torch.cuda.get_device_name(0), 'blocks': blocks, 'calls_per_block': inner, 'frame': [H, W], 'D': D, 'frames': list(SHAPES),
           'forward_batch': FORWARD_BATCH, 'finds_the_pans': checked, 'kernels': t, 'us_per_frame_at_median': per_frame,
           'ratio_to_forward_per_frame': {k: v / fwd for k, v in per_frame.items() if k != 'forward'},
           'bytes_read_per_frame': H * W * 3, 'workspace_bytes_per_frame': H * W * 2 + (H // 4) * (W // 4) * 2}
    eng.close()
    print(json.dumps(res), flush=True)
    with open(os.path.join(outdir, name + '.json'), 'w') as fh:
        json.dump(res, fh, indent=1)


if __name__ == '__main__':
    main()
