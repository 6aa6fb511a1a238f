"""Times the fit of windows beside the letterbox fit it shares its kernel with, at the C ABI on packed device buffers and a
preallocated 64 x 480 x 720 x 3 byte output, the two arms of a pair alternating block by block on the same device (tools/mirror_time.py:
alternate -- warm-up, then blocks of `inner` calls between two device events; per call: median, minimum, 90th percentile):
  windows_in_1080x1920   jcm_fit_windows: 64 windows of 400 x 600, one in each of 64 sources of 1080 x 1920 (at varying, odd positions inside)
                         against jcm_fit_images on 64 sources of 400 x 600 holding the same pixels -- the same filter work; the windows' rows lie
                         1920 pixels apart in memory instead of 600
  whole_image_windows    jcm_fit_windows with the window (0, 0, h, w) of each of 64 sources of 1080 x 1920 against jcm_fit_images on those
                         sources -- the same bytes read and the same bytes written
Before timing, each pair's two outputs are compared: they must be equal, so the timed calls do the same work.  Writes <outdir>/<name>.json.
    python tools/fit_windows_time.py <outdir> [blocks=20] [inner=10] [--name fit_windows_time]"""
import ctypes
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import joint_cnn_mrf_amd  # noqa: F401,E402
from joint_cnn_mrf_amd import _lib  # noqa: E402
from joint_cnn_mrf_amd.engine import Engine  # noqa: E402
from mirror_time import alternate  # noqa: E402

OH, OW, N = 480, 720, 64


def _i64(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))


def pair(eng, name, src, desc7, ref_src, desc3, blocks, inner, out):
    """jcm_fit_windows(src, desc7) against jcm_fit_images(ref_src, desc3): equal outputs, then alternating timing."""
    lib, h, p = eng._lib, eng._h, eng._p
    dst_w = torch.empty((N, OH, OW, 3), dtype=torch.uint8, device='cuda:0')
    dst_i = torch.empty_like(dst_w)

    def windows():
        return lib.jcm_fit_windows(h, p(src), src.numel(), _i64(desc7), N, 3, OH, OW, 0, 0, p(dst_w), None)

    def images():
        return lib.jcm_fit_images(h, p(ref_src), ref_src.numel(), _i64(desc3), N, 3, OH, OW, 0, 0, p(dst_i), None)
    _lib.check(windows(), 'jcm_fit_windows')
    _lib.check(images(), 'jcm_fit_images')
    torch.cuda.synchronize()
    assert torch.equal(dst_w, dst_i), name
    r = alternate({'fit_windows': windows, 'fit_images': images}, blocks, inner)
    mw, mi = r['fit_windows']['device_events']['median_us'], r['fit_images']['device_events']['median_us']
    r.update(windows=N, outputs_equal=True, fit_windows_over_fit_images_at_median=mw / mi)
    out[name] = r
    print('%s: %s' % (name, json.dumps(r)), flush=True)


def main():
    argv = sys.argv[1:]
    name = 'fit_windows_time'
    if '--name' in argv:
        i = argv.index('--name')
        name = argv[i + 1]
        del argv[i:i + 2]
    if not argv or any(a.startswith('--') for a in argv):
        sys.exit(__doc__)
    outdir = argv[0]
    blocks = int(argv[1]) if len(argv) > 1 else 20
    inner = int(argv[2]) if len(argv) > 2 else 10
    os.makedirs(outdir, exist_ok=True)
    res = {'device': torch.cuda.get_device_name(0), 'blocks': blocks, 'calls_per_block': inner, 'frame': [OH, OW], 'pairs': {}}
    eng = Engine(device=0)
    H, W, wh, ww = 1080, 1920, 400, 600
    big = torch.randint(0, 256, (N, H, W, 3), dtype=torch.uint8, device='cuda:0')
    desc_big = np.array([(i * H * W * 3, H, W) for i in range(N)], np.int64)
    rs = np.random.RandomState(0)
    pos = np.stack([rs.randint(0, H - wh + 1, N), rs.randint(0, W - ww + 1, N) | 1], axis=1)
    pos[:, 1] = np.minimum(pos[:, 1], W - ww - 1)
    desc7 = np.ascontiguousarray(np.concatenate([desc_big, pos, np.full((N, 2), (wh, ww))], axis=1).astype(np.int64))
    crops = torch.stack([big[i, y:y + wh, x:x + ww] for i, (y, x) in enumerate(pos)]).contiguous()
    desc_crop = np.array([(i * wh * ww * 3, wh, ww) for i in range(N)], np.int64)
    pair(eng, 'windows_in_1080x1920', big.view(-1), desc7, crops.view(-1), desc_crop, blocks, inner, res['pairs'])
    whole = np.ascontiguousarray(np.concatenate([desc_big, np.zeros((N, 2), np.int64), np.full((N, 2), (H, W))], axis=1).astype(np.int64))
    pair(eng, 'whole_image_windows', big.view(-1), whole, big.view(-1), desc_big, blocks, inner, res['pairs'])
    eng.close()
    with open(os.path.join(outdir, name + '.json'), 'w') as fh:
        json.dump(res, fh, indent=1)


if __name__ == '__main__':
    main()
