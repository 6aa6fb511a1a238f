"""Times the feeding of the forward pass on full-width towers at 480 x 720: the fp32 handle at B = 64 and the bf16 handle
at B = 256, images/s of
  (a) Engine.forward on a device-resident float32 batch;
  (b) the same on a device-resident uint8 batch;
  (c) stream.forward_stream from host float32 batches;
  (d) stream.forward_stream from host uint8 batches;
  (e) the evaluation CLI's pattern before --u8_images: a pageable float32 array, copied synchronously, then Towers.forward's body;
plus the bare pinned host-to-device copy rate, and the DeviceDataset upload (seconds, bytes) of N synthetic images in both storages.
The five arms are alternated in one process after a warm-up, three rounds, medians reported (every round is kept in the JSON); an arm is
timed on the host from its first call to the end of its device work, over `nb` batches.
    timeout -k 10 1100 python tools/feed_time.py <outdir> [nb=6] [N=3987]
Writes <outdir>/feed_time.json."""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import joint_cnn_mrf_amd  # noqa: F401,E402
from joint_cnn_mrf_amd import synth  # noqa: E402
from joint_cnn_mrf_amd.dataset import DeviceDataset  # noqa: E402
from joint_cnn_mrf_amd.engine import Engine  # noqa: E402
from joint_cnn_mrf_amd.main import byte_grid  # noqa: E402
from joint_cnn_mrf_amd.stream import ForwardStream  # noqa: E402

H, W, h, w = 480, 720, 60, 90
ROUNDS = 3
IMAGE_BYTES_F32, IMAGE_BYTES_U8 = H * W * 3 * 4, H * W * 3


def byte_batch(B, seed):
    """B byte images: 16 generated ones, repeated (the forward's time does not depend on the values; the link's does not either)."""
    k = byte_grid(synth.make_images(16, seed=seed))
    return np.ascontiguousarray(np.concatenate([k] * (B // 16 + 1))[:B])


def copy_rate(nbytes=1 << 30, reps=5):
    src = torch.empty(nbytes, dtype=torch.uint8).pin_memory()
    dst = torch.empty(nbytes, dtype=torch.uint8, device='cuda:0')
    rates = []
    for i in range(reps + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        dst.copy_(src, non_blocking=True)
        e1.record()
        e1.synchronize()
        if i:
            rates.append(nbytes / (e0.elapsed_time(e1) * 1e-3) / 1e9)
    return {'bytes': nbytes, 'GBps': rates, 'GBps_median': float(np.median(rates))}


def time_handle(precision, B, nb, link_GBps):
    params = synth.make_pd_params(debug=False)
    params.update(synth.make_sm_params(synth.synthetic_priors(), kind='init'))
    eng = Engine(device=0, precision=precision).load_params(params)
    ks = [byte_batch(B, 1), byte_batch(B, 2)]
    fs = [k.astype(np.float32) / np.float32(255) for k in ks]          # pageable
    torso = synth.make_torso(B, seed=3)
    d_torso = torch.as_tensor(torso, device='cuda:0')
    d_k, d_f = torch.as_tensor(ks[0], device='cuda:0'), torch.as_tensor(fs[0], device='cuda:0')
    st_f, st_k = ForwardStream(eng, use_sm=True), ForwardStream(eng, use_sm=True)

    def resident(x):
        for _ in range(nb):
            r = eng.forward(x, d_torso, use_sm=True, want_prob=False)
        return r['sm_coords'].cpu()

    def streamed(st, pool):
        return [r for r in st.run((pool[i % 2], torso) for i in range(nb))]

    def pageable():
        for i in range(nb):
            x = torch.as_tensor(fs[i % 2]).to('cuda:0', non_blocking=True).contiguous()
            t = torch.as_tensor(torso).to('cuda:0', non_blocking=True).contiguous()
            r = eng.forward(x, t, use_sm=True, want_prob=False)
        return r['sm_coords'].cpu()
    arms = [('a_resident_f32', lambda: resident(d_f)), ('b_resident_u8', lambda: resident(d_k)), ('c_stream_f32', lambda: streamed(st_f, fs)),
            ('d_stream_u8', lambda: streamed(st_k, ks)), ('e_pageable_f32_sync', pageable)]
    for _name, fn in arms:                                             # warm-up: filter spectra, workspace, pinned buffers
        fn()
    rounds = {name: [] for name, _ in arms}
    for _ in range(ROUNDS):
        for name, fn in arms:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            rounds[name].append(nb * B / (time.perf_counter() - t0))
    res = {'precision': precision, 'B': B, 'batches_per_round': nb,
           'images_per_s': {k: {'rounds': v, 'median': float(np.median(v)), 'spread': float(max(v) - min(v))} for k, v in rounds.items()}}
    ips = {k: v['median'] for k, v in res['images_per_s'].items()}
    res['byte_forward_vs_float_forward'] = {'b_over_a': ips['b_resident_u8'] / ips['a_resident_f32'],
                                            'spread_of_a_relative': res['images_per_s']['a_resident_f32']['spread'] / ips['a_resident_f32']}
    for tag, nbytes, arm in (('f32', IMAGE_BYTES_F32 + h * w * 4, 'c_stream_f32'), ('u8', IMAGE_BYTES_U8 + h * w * 4, 'd_stream_u8')):
        need = nbytes * ips['b_resident_u8'] / 1e9
        res['link_' + tag] = {'bytes_per_image': nbytes, 'GBps_needed_at_resident_rate': need, 'GBps_measured_copy': link_GBps,
                              'achieved_fraction_of_resident_rate': ips[arm] / ips['b_resident_u8'], 'bound_by': 'link' if need > link_GBps else 'compute'}
    eng.close()
    return res


def upload_times(N):
    k = np.concatenate([byte_grid(synth.make_images(16, seed=5))] * (N // 16 + 1))[:N]
    y = np.zeros((N, h, w, 10), np.float32)
    out = {}
    for name, src, kind in (('uint8_from_bytes', k, 'uint8'), ('uint8_from_floats', None, 'uint8'), ('float32', None, 'float32')):
        if src is None:
            src = k.astype(np.float32) / np.float32(255)
        ds = DeviceDataset(src, y, device=0, image_dtype=kind)
        out[name] = {'bytes': ds.nbytes, 'seconds': ds.upload_seconds, 'GBps': ds.nbytes / ds.upload_seconds / 1e9}
        del ds, src
        torch.cuda.empty_cache()
        print('upload %-18s %s' % (name, out[name]), flush=True)
    return out


def main():
    args = [a for a in sys.argv[1:] if not a.startswith('--')]
    if not args:
        sys.exit(__doc__)
    outdir = args[0]
    nb = int(args[1]) if len(args) > 1 else 6
    N = int(args[2]) if len(args) > 2 else 3987
    os.makedirs(outdir, exist_ok=True)
    res = {'H': H, 'W': W, 'device': torch.cuda.get_device_name(0), 'rounds': ROUNDS, 'pinned_copy': copy_rate()}
    print('pinned copy: %s' % res['pinned_copy'], flush=True)

    def save():
        with open(os.path.join(outdir, 'feed_time.json'), 'w') as fh:
            json.dump(res, fh, indent=1)
    for precision, B in (('fp32', 64), ('bf16', 256)):
        res[precision] = time_handle(precision, B, nb, res['pinned_copy']['GBps_median'])
        print(json.dumps(res[precision]), flush=True)
        save()
    res['upload'] = dict(upload_times(N), N=N)
    save()


if __name__ == '__main__':
    main()
