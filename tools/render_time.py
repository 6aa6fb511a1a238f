"""Times the pose renderer: jcm_render_poses on 64 byte images of 1080x1920 with one skeleton each (17 or 18 capsules, what
predict.skeleton_primitives makes of nine joints spread over the image), at the C ABI on a packed device buffer: into a second buffer and in
place, without and with the heat tint (nine 60x90 maps per image, the letterbox geometry of 1080x1920 in 480x720); without any primitive (the
copy path); beside a device-to-device copy (torch's copy_, same stream) of the same buffer and jcm_fit_images on the same sources, in the same
run.  Every arm is warmed up, then timed in blocks of `inner` calls between two device events; the figures are per call: the median over the
blocks, the minimum and the 90th percentile.  Writes <outdir>/<name>.json.
    python tools/render_time.py <outdir> [blocks=20] [inner=10] [--name render_time]"""
import ctypes
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import joint_cnn_mrf_amd  # noqa: F401,E402
from joint_cnn_mrf_amd import _lib, predict  # noqa: E402
from joint_cnn_mrf_amd.engine import Engine  # noqa: E402
from joint_cnn_mrf_amd.evaluation import fit_geometry  # noqa: E402
from mirror_time import alternate  # noqa: E402

H, W, B = 1080, 1920, 64
OH, OW = 480, 720


def skeletons(rs):
    """One person per image, of about half the image's height, somewhere in it."""
    shape = np.array([(0.25, 0.62), (0.45, 0.68), (0.62, 0.72), (0.25, 0.38), (0.45, 0.32), (0.62, 0.28), (0.70, 0.58), (0.70, 0.42), (0.10, 0.50)])
    results = []
    for _ in range(B):
        size = rs.uniform(0.5, 0.9) * H
        origin = np.array([rs.uniform(0, H - size), rs.uniform(0, W - size)])
        results.append({'size': (H, W), 'sm': origin + shape * size + rs.uniform(-10, 10, (9, 2)), 'sm_inside': np.ones(9, bool)})
    return predict.skeleton_primitives(results)


def main():
    argv = sys.argv[1:]
    name = 'render_time'
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
    eng = Engine(device=0)
    lib, h, p = eng._lib, eng._h, eng._p
    rs = np.random.RandomState(0)
    desc = np.array([(b * H * W * 3, H, W) for b in range(B)], np.int64)
    off = B * H * W * 3
    dp = desc.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))
    src = torch.randint(0, 256, (off,), dtype=torch.uint8, device='cuda:0')
    dst, own = torch.empty_like(src), src.clone()
    fitted = torch.empty((B, OH, OW, 3), dtype=torch.uint8, device='cuda:0')
    prims = np.ascontiguousarray(skeletons(rs), np.int32)
    pp = prims.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
    hm = torch.rand((B, 60, 90, 9), device='cuda:0') ** 8
    geom = np.ascontiguousarray(np.tile(np.array(fit_geometry(H, W, OH, OW), np.int32), (B, 1)))
    gp = geom.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
    mask = np.array(predict.HEAT_MASK, np.uint8)
    mp = mask.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))

    def render(out, n, heat):
        return lib.jcm_render_poses(h, p(src if out is not own else own), off, dp, B, p(out), pp if n else None, n,
                                    p(hm) if heat else None, 60, 90, 9, 8, gp if heat else None, mp if heat else None, 255)
    for out, n, heat in ((dst, len(prims), False), (dst, len(prims), True), (own, len(prims), False), (dst, 0, False)):
        _lib.check(render(out, n, heat), 'jcm_render_poses')
    torch.cuda.synchronize()
    arms = {'render_skeletons': lambda: render(dst, len(prims), False),
            'render_skeletons_in_place': lambda: render(own, len(prims), False),
            'render_no_primitives': lambda: render(dst, 0, False),
            'render_skeletons_and_tint': lambda: render(dst, len(prims), True),
            'copy_source': lambda: dst.copy_(src),
            'fit_images_u8': lambda: lib.jcm_fit_images(h, p(src), off, dp, B, 3, OH, OW, 0, 0, p(fitted), None)}
    t = alternate(arms, blocks, inner)
    copy = t['copy_source']['device_events']['median_us']
    res = {'device': torch.cuda.get_device_name(0), 'blocks': blocks, 'calls_per_block': inner, 'images': B, 'image': [H, W], 'source_bytes': int(off),
           'primitives': int(len(prims)), 'upload_launches_per_call': -(-len(prims) // 120), 'kernels': t,
           'ratio_to_copy_at_median': {k: v['device_events']['median_us'] / copy for k, v in t.items() if k.startswith('render')},
           'kernel_shape': {'threads': 256, 'tile_pixels': 8192, 'lds_bytes': 8192 * 3 + 16 + 256 * 48 + 16, 'work_groups': B * -(-H * W // 8192)}}
    eng.close()
    print(json.dumps(res), flush=True)
    with open(os.path.join(outdir, name + '.json'), 'w') as fh:
        json.dump(res, fh, indent=1)


if __name__ == '__main__':
    main()
