"""Times the mirrored test-time evaluation at the shapes Engine.forward(flip_test=True) uses for 32 fp32 images:
  mirror_pairs on the images [32,480,720,3] and on the torso maps [32,60,90,1], mirror_merge on the maps [64,60,90,9] (group 2), each beside a
  device-to-device copy (torch's copy_, on the same stream) of a buffer of the kernel's OUTPUT size for mirror_pairs and of its INPUT size for
  mirror_merge, the two arms alternated block by block in one process.  Bytes per second are (bytes read + bytes written) / time for both arms:
  mirror_pairs reads n and writes 2n, mirror_merge reads 2n and writes n, a copy of m bytes reads m and writes m.
  With --forward: Engine.forward(flip_test=True) on 32 images beside Engine.forward on 64 images, full-width fp32 engine, spatial model on,
  want_prob=False, alternated call by call.  With --forward64 INSTEAD: only Engine.forward on 64 images, through calls that every earlier commit
  has -- copy this file into another checkout's tools/ to time that commit's forward on the same machine, in the same job.
The kernels are called at the C ABI on preallocated outputs.  Each arm is warmed up, then timed in blocks of `inner` calls between two device
events; the figures are per call: the median over the blocks, the minimum and the 90th percentile.  Writes <outdir>/<name>.json.
    python tools/mirror_time.py <outdir> [blocks=40] [inner=20] [--forward | --forward64] [--name mirror_time]"""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import joint_cnn_mrf_amd  # noqa: F401,E402
from joint_cnn_mrf_amd import _lib, synth  # noqa: E402
from joint_cnn_mrf_amd.engine import Engine  # noqa: E402


def block(fn, inner):
    """(device ms, host ms) of `inner` consecutive calls."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    e0.record()
    for _ in range(inner):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), (time.perf_counter() - t0) * 1e3


def stats(ms_per_call):
    a = np.sort(np.asarray(ms_per_call))
    return {'blocks': int(a.size), 'median_us': float(np.median(a) * 1e3), 'min_us': float(a[0] * 1e3), 'p90_us': float(a[int(0.9 * (a.size - 1))] * 1e3)}


def alternate(arms, blocks, inner):
    for fn in arms.values():                                        # warm-up: code objects, torch's allocator
        block(fn, inner)
    t = {name: ([], []) for name in arms}
    for _ in range(blocks):
        for name, fn in arms.items():
            dev, host = block(fn, inner)
            t[name][0].append(dev / inner)
            t[name][1].append(host / inner)
    return {name: {'device_events': stats(t[name][0]), 'host_clock': stats(t[name][1])} for name in t}


def kernels(eng, blocks, inner):
    lib, h, p = eng._lib, eng._h, eng._p
    out = {}

    def pairs_case(name, x):
        B, H, W, C = x.shape
        dst = torch.empty((2 * B, H, W, C), dtype=x.dtype, device=x.device)
        src2, dst2 = torch.empty_like(dst), torch.empty_like(dst)      # the copy of the output's size
        u8 = int(x.dtype == torch.uint8)

        def kernel():
            lib.jcm_mirror_pairs(h, p(x), u8, B, H, W, C, p(dst))
        _lib.check(lib.jcm_mirror_pairs(h, p(x), u8, B, H, W, C, p(dst)), 'jcm_mirror_pairs')
        torch.cuda.synchronize()
        assert torch.equal(dst[0::2], x) and torch.equal(dst[1::2], torch.flip(x, dims=[2]))      # the timed call does the work
        r = alternate({'mirror_pairs': kernel, 'copy': lambda: dst2.copy_(src2)}, blocks, inner)
        n = x.numel() * x.element_size()
        r.update(bytes_moved_kernel=3 * n, bytes_moved_copy=4 * n)
        finish(name, r)

    def merge_case(name, hm):
        N, HH, WW, K = hm.shape
        dst = torch.empty((N // 2, HH, WW, K), device=hm.device)
        dst2 = torch.empty_like(hm)

        def kernel():
            lib.jcm_mirror_merge(h, p(hm), N // 2, 2, HH, WW, K, None, p(dst))
        _lib.check(lib.jcm_mirror_merge(h, p(hm), N // 2, 2, HH, WW, K, None, p(dst)), 'jcm_mirror_merge')
        torch.cuda.synchronize()
        perm = list(_lib.HM_FLIP_PERM[:K])
        assert torch.equal(dst, ((hm[0::2].double() + torch.flip(hm[1::2], dims=[2])[..., perm].double()) / 2).float())
        r = alternate({'mirror_merge': kernel, 'copy': lambda: dst2.copy_(hm)}, blocks, inner)
        n = dst.numel() * 4
        r.update(bytes_moved_kernel=3 * n, bytes_moved_copy=4 * n)
        finish(name, r)

    def finish(name, r):
        kern = 'mirror_merge' if 'mirror_merge' in r else 'mirror_pairs'
        r['kernel_GBps_at_median'] = r['bytes_moved_kernel'] / (r[kern]['device_events']['median_us'] * 1e-6) / 1e9
        r['copy_GBps_at_median'] = r['bytes_moved_copy'] / (r['copy']['device_events']['median_us'] * 1e-6) / 1e9
        r['kernel_rate_over_copy_rate'] = r['kernel_GBps_at_median'] / r['copy_GBps_at_median']
        out[name] = r
        print('%s: %s' % (name, json.dumps(r)), flush=True)

    pairs_case('mirror_pairs_images_32x480x720x3_f32', torch.rand(32, 480, 720, 3, device='cuda:0'))
    pairs_case('mirror_pairs_images_32x480x720x3_u8', torch.randint(0, 256, (32, 480, 720, 3), dtype=torch.uint8, device='cuda:0'))
    pairs_case('mirror_pairs_torso_32x60x90x1_f32', torch.rand(32, 60, 90, 1, device='cuda:0'))
    merge_case('mirror_merge_64x60x90x9_group2', torch.rand(64, 60, 90, 9, device='cuda:0'))
    return out


def forward(blocks, only64):
    params = synth.make_pd_params(debug=False)
    params.update(synth.make_sm_params(synth.synthetic_priors(), kind='init'))
    eng = Engine(device=0, precision='fp32').load_params(params)
    x = torch.as_tensor(np.concatenate([synth.make_images(16, seed=5)] * 4), device='cuda:0')
    torso = torch.as_tensor(synth.make_torso(64, seed=3), device='cuda:0')
    arms = {'forward_64': lambda: eng.forward(x, torso, use_sm=True, want_prob=False)}
    if not only64:
        x32, t32 = x[:32].contiguous(), torso[:32].contiguous()
        arms['forward_flip_test_32'] = lambda: eng.forward(x32, t32, use_sm=True, want_prob=False, flip_test=True)
    r = alternate(arms, blocks, 1)
    if not only64:
        r['flip_test_cost_us_device_median'] = r['forward_flip_test_32']['device_events']['median_us'] - r['forward_64']['device_events']['median_us']
        r['flip_test_cost_percent'] = 100 * r['flip_test_cost_us_device_median'] / r['forward_64']['device_events']['median_us']
    eng.close()
    print('forward: %s' % json.dumps(r), flush=True)
    return r


def main():
    argv = sys.argv[1:]
    name = 'mirror_time'
    if '--name' in argv:
        i = argv.index('--name')
        name = argv[i + 1]
        del argv[i:i + 2]
    flags = [a for a in argv if a.startswith('--')]
    argv = [a for a in argv if not a.startswith('--')]
    if not argv or set(flags) - {'--forward', '--forward64'}:
        sys.exit(__doc__)
    outdir = argv[0]
    blocks = int(argv[1]) if len(argv) > 1 else 40
    inner = int(argv[2]) if len(argv) > 2 else 20
    os.makedirs(outdir, exist_ok=True)
    res = {'device': torch.cuda.get_device_name(0), 'blocks': blocks, 'calls_per_block': inner}
    if '--forward64' in flags:
        res['forward_fp32'] = forward(min(blocks, 30), True)
    else:
        eng = Engine(device=0)
        res['kernels'] = kernels(eng, blocks, inner)
        eng.close()
        if '--forward' in flags:
            res['forward_fp32'] = forward(min(blocks, 30), False)
    with open(os.path.join(outdir, name + '.json'), 'w') as fh:
        json.dump(res, fh, indent=1)


if __name__ == '__main__':
    main()
