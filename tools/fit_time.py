"""Times the letterbox fit: jcm_fit_images on 64 byte images of 1080x1920 -> 480x720 (uint8 out; and float32 out), at the C ABI
on a packed device buffer and a preallocated output, beside a device-to-device copy (torch's copy_, same stream) of the source buffer.  Every arm
is warmed up, then timed in blocks of `inner` calls between two device events; the figures are per call: the median over the blocks, the minimum
and the 90th percentile.  Bytes per second are the ALGORITHMIC bytes -- the source bytes once plus the output bytes once -- over the median time.
A second case packs 64 images of mixed sizes (portrait, landscape, small, equal-size) to show the ragged grid.
With --forward: Engine.forward(x_u8, torso='infer') on the 64 fitted images, full-width fp32 engine, want_prob=False -- what the fit is a cost on
top of.  Writes <outdir>/<name>.json.
    python tools/fit_time.py <outdir> [blocks=20] [inner=10] [--forward] [--name fit_time]"""
import ctypes
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

OH, OW = 480, 720


def case(eng, name, sizes, blocks, inner, out):
    lib, h, p = eng._lib, eng._h, eng._p
    B = len(sizes)
    desc = np.empty((B, 3), np.int64)
    off = 0
    for i, (hh, ww) in enumerate(sizes):
        desc[i] = (off, hh, ww)
        off += hh * ww * 3
    src = torch.randint(0, 256, (off,), dtype=torch.uint8, device='cuda:0')
    src2 = torch.empty_like(src)
    dp = desc.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))
    r = {}
    for f32 in (0, 1):
        dst = torch.empty((B, OH, OW, 3), dtype=torch.float32 if f32 else torch.uint8, device='cuda:0')
        _lib.check(lib.jcm_fit_images(h, p(src), off, dp, B, 3, OH, OW, 0, f32, p(dst), None), 'jcm_fit_images')
        torch.cuda.synchronize()
        key = 'fit_f32' if f32 else 'fit_u8'
        t = alternate({key: lambda: lib.jcm_fit_images(h, p(src), off, dp, B, 3, OH, OW, 0, f32, p(dst), None), 'copy_source': lambda: src2.copy_(src)}, blocks, inner)
        n = off + dst.numel() * dst.element_size()
        r[key] = t[key]
        r[key + '_algorithmic_bytes'] = int(n)
        r[key + '_GBps_at_median'] = n / (t[key]['device_events']['median_us'] * 1e-6) / 1e9
        r['copy_source'] = t['copy_source']
        r['copy_source_GBps_at_median'] = 2 * off / (t['copy_source']['device_events']['median_us'] * 1e-6) / 1e9
    r.update(images=B, source_bytes=int(off))
    out[name] = r
    print('%s: %s' % (name, json.dumps(r)), flush=True)


def forward(blocks):
    params = synth.make_pd_params(debug=False)
    params.update(synth.make_sm_params(synth.synthetic_priors(), kind='init'))
    eng = Engine(device=0, precision='fp32').load_params(params)
    images = [torch.randint(0, 256, (1080, 1920, 3), dtype=torch.uint8, device='cuda:0') for _ in range(64)]
    x, _ = eng.fit_images(images)
    r = alternate({'forward_infer_64_u8': lambda: eng.forward(x, 'infer', use_sm=True, want_prob=False),
                   'fit_images_64_engine_call': lambda: eng.fit_images(images, out=x)}, blocks, 1)
    eng.close()
    print('forward: %s' % json.dumps(r), flush=True)
    return r


def main():
    argv = sys.argv[1:]
    name = 'fit_time'
    if '--name' in argv:
        i = argv.index('--name')
        name = argv[i + 1]
        del argv[i:i + 2]
    flags = [a for a in argv if a.startswith('--')]
    argv = [a for a in argv if not a.startswith('--')]
    if not argv or set(flags) - {'--forward'}:
        sys.exit(__doc__)
    outdir = argv[0]
    blocks = int(argv[1]) if len(argv) > 1 else 20
    inner = int(argv[2]) if len(argv) > 2 else 10
    os.makedirs(outdir, exist_ok=True)
    res = {'device': torch.cuda.get_device_name(0), 'blocks': blocks, 'calls_per_block': inner, 'frame': [OH, OW], 'kernels': {}}
    eng = Engine(device=0)
    case(eng, 'fit_64x1080x1920', [(1080, 1920)] * 64, blocks, inner, res['kernels'])
    mixed = [(1080, 1920), (1920, 1080), (480, 640), (480, 720), (3000, 4000), (240, 320), (1000, 700), (211, 317)] * 8
    case(eng, 'fit_64_mixed_sizes', mixed, blocks, inner, res['kernels'])
    eng.close()
    if '--forward' in flags:
        res['forward_fp32'] = forward(min(blocks, 20))
    with open(os.path.join(outdir, name + '.json'), 'w') as fh:
        json.dump(res, fh, indent=1)


if __name__ == '__main__':
    main()
