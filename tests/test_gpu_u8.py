"""Byte images on the GPU.  A byte k stands for float32(k) / float32(255), the value data.load_image makes of it, so every
result on byte images must equal the result on that float image BIT FOR BIT: there is no tolerance anywhere in this file.  The float
references are always made on the host with numpy (`as_float`) and uploaded, never by a division on the device under test."""
import json
import os

import numpy as np
import pytest
import torch

from cli_util import run_cli
import joint_cnn_mrf_amd  # noqa: F401
from joint_cnn_mrf_amd import synth
from joint_cnn_mrf_amd import main as M
from joint_cnn_mrf_amd.dataset import DeviceDataset, NotByteExact
from test_gpu_augment import edge_params          # the parameter set of the augmentation's own tests

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
SENTINEL = -7.25


def as_float(k):
    return np.asarray(k, np.uint8).astype(f32) / f32(255)


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), device='cuda:0')


def engine(**kw):
    from joint_cnn_mrf_amd.engine import Engine
    return Engine(device=0, **kw)


def byte_images(B, H, W, seed=0):
    """Image 0 all 0, image 1 all 255, image 2 a full ramp (every byte value, at every alignment of the 3-byte pixels), the rest random."""
    k = np.random.RandomState(seed).randint(0, 256, (B, H, W, 3)).astype(np.uint8)
    k[0] = 0
    if B > 1:
        k[1] = 255
    if B > 2:
        k[2] = (np.arange(H * W * 3) % 256).reshape(H, W, 3).astype(np.uint8)
    return k


def params(debug=True):
    p = synth.make_pd_params(debug=debug, bn='trained', conv6_gain=8.0)
    p.update(synth.make_sm_params(synth.synthetic_priors(), kind='trained'))
    return p


def unaligned(a, off):
    """The device copy of the byte array `a` starting `off` bytes behind a 256-byte aligned allocation."""
    buf = torch.empty(a.size + off, dtype=torch.uint8, device='cuda:0')
    v = buf[off:off + a.size].view(a.shape)
    v.copy_(torch.as_tensor(np.ascontiguousarray(a)))
    assert v.data_ptr() % 4 == off % 4 and v.is_contiguous()
    return v


# ------------------------------------------------------------------ the conversion itself
@pytest.mark.parametrize('shape', [(1, 8, 32, 3), (2, 7, 11, 3), (3, 16, 16, 3)], ids=['wide', 'narrow_231_bytes', 'wide_three_ramps'])
@pytest.mark.parametrize('off', [0, 1])
def test_all_256_values_through_the_device_conversion_equal_numpy(shape, off):
    """u8_to_f32 (csrc/u8.h) by way of the converting gather: the full ramp, on the dword route and on the byte route."""
    n = int(np.prod(shape))
    k = (np.arange(n) % 256).astype(np.uint8).reshape(shape)
    assert n >= 256 and set(k.reshape(-1).tolist()) == set(range(256))
    y = dev(np.zeros((shape[0], 2, 2, 10), f32))
    eng = engine()
    idx = np.arange(shape[0])[::-1].copy()
    xo, _ = eng.gather_batch(unaligned(k, off), y, idx)
    torch.cuda.synchronize()
    got = xo.cpu().numpy()
    assert got.dtype == f32 and np.array_equal(got.view(np.uint32), as_float(k)[idx].view(np.uint32))
    eng.close()


# ------------------------------------------------------------------ the forward
FORWARD_CASES = {
    'fp32_default': (dict(), True, 4),
    'fp32_exact_mfma': (dict(conv9_fft=False), True, 4),
    'fp32_split16': (dict(f32_conv='split16'), True, 4),
    'fp32_micro_batch_2': (dict(micro_batch=2), True, 5),          # slices of 2, 2, 1 images
    'bf16_micro_batch_3_full_width': (dict(precision='bf16', micro_batch=3), False, 5),      # (bf16 handles exist at full width only: Cin % 32)
    'fp32_full_width': (dict(), False, 3),
    'fp32_micro_batch_2_full_width': (dict(micro_batch=2), False, 5),      # the slice pointer b0 * H * W * 3 bytes on the split kernel
    'fp32_exact_mfma_full_width': (dict(conv9_fft=False), False, 3),
    'bf16_full_width': (dict(precision='bf16'), False, 3),
}
# the conv1 route of each case: the debug-width network (16 filters) takes the generic kernel on every handle, the full-width one the three MFMA kernels
CONV1_KERNEL = {'fp32_full_width': 'conv1_mfma_pool_split_kernel', 'fp32_micro_batch_2_full_width': 'conv1_mfma_pool_split_kernel',
                'fp32_exact_mfma_full_width': 'conv1_mfma_pool_f32_kernel',
                'bf16_full_width': 'conv1_mfma_pool_kernel', 'bf16_micro_batch_3_full_width': 'conv1_mfma_pool_kernel'}


@pytest.mark.parametrize('case', sorted(FORWARD_CASES))
def test_forward_and_eval_forward_on_bytes_equal_the_float_calls(case):
    kw, debug, B = FORWARD_CASES[case]
    k = byte_images(B, 480, 720, seed=len(case))
    y = synth.make_targets(B, seed=7)
    xb, xf, yd = dev(k), dev(as_float(k)), dev(y)
    torso = yd[..., 9:].contiguous()
    eng = engine(**kw).load_params(params(debug))
    assert eng.conv_kernel_name('conv1_fullres', B, 480, 720) == CONV1_KERNEL.get(case, 'conv1_5x5s2_kernel')      # the route the case is here for
    for use_sm in (True, False):
        want = eng.forward(xf, torso, use_sm=use_sm)
        got = eng.forward(xb, torso, use_sm=use_sm)
        assert sorted(got) == sorted(want)
        for key in want:
            assert got[key].dtype == want[key].dtype and torch.equal(got[key], want[key]), (case, use_sm, key)
        want = eng.eval_forward(xf, yd, use_sm=use_sm)
        got = eng.eval_forward(xb, yd, use_sm=use_sm)
        for key in want:
            assert torch.equal(got[key], want[key]), (case, use_sm, key)
        assert bool(torch.isfinite(got['losses']).all())
    # every other dtype is refused as before
    for bad in (xf.double(), xf.half(), xb.to(torch.int8), xb.to(torch.int32)):
        with pytest.raises(TypeError, match='x must be torch.float32'):
            eng.forward(bad, torso)
    eng.close()


@pytest.mark.parametrize('precision', ['fp32', 'bf16'])
@pytest.mark.parametrize('hw', [(244, 364), (200, 296), (250, 366)])
def test_model_on_bytes_at_odd_geometries(hw, precision):
    """jcm_pd_forward_u8 where the sub-sampled extents are odd: 244x364 (half and quarter branches on the generic conv1 kernel, 61x91
    with asymmetric padding), 200x296 (quarter branch generic, 50x74) and 250x366, whose quarter branch is a real bilinear resize (the
    byte batch is widened once, in front of the branches, for the resize kernel)."""
    H, W = hw
    k = byte_images(3, H, W, seed=H)
    eng = engine(precision=precision).load_params(params(precision != 'bf16'))      # debug width; bf16 handles exist at full width only
    want = eng.model(dev(as_float(k)))
    got = eng.model(dev(k))
    assert got.shape == want.shape and torch.equal(got, want)
    assert bool(torch.isfinite(got).all()) and float(got.std()) > 0
    got1 = eng.model(unaligned(k, 1))                    # a byte batch that starts at an odd address
    assert torch.equal(got1, want)
    eng.close()


# ------------------------------------------------------------------ gather and indexed augmentation from a byte set
@pytest.mark.parametrize('off', [0, 1, 2], ids=['aligned', 'off1', 'off2'])
@pytest.mark.parametrize('shape', [(480, 720, 60, 90), (37, 53, 7, 11), (7, 11, 2, 2)], ids=['480x720', '37x53', '7x11'])
def test_gather_and_indexed_augmentation_from_bytes_equal_those_from_floats(shape, off):
    H, W, h, w = shape
    N, idx = 9, np.asarray([8, 2, 2, 0, 5, 7, 1], np.int32)
    k = byte_images(N, H, W, seed=H + off)
    y = dev(np.random.RandomState(H).random_sample((N, h, w, 10)).astype(f32))
    xb, xf = unaligned(k, off), dev(as_float(k))
    p = dev(edge_params(len(idx), seed=11))
    eng = engine()
    wx, wy = eng.gather_batch(xf, y, idx)
    gx, gy = eng.gather_batch(xb, y, idx)
    assert gx.dtype == torch.float32 and torch.equal(gx, wx) and torch.equal(gy, wy)
    # into given buffers, and an output that does not start 16-byte aligned (the byte route of the stores)
    flat = torch.full((gx.numel() + 1,), SENTINEL, device='cuda:0')
    xo = flat[1:].view(gx.shape)
    r = eng.gather_batch(xb, y, idx, xo, torch.empty_like(gy))
    assert r[0] is xo and torch.equal(xo, wx) and float(flat[0]) == SENTINEL
    wx, wy = eng.augment_train_indexed(xf, y, idx, p)
    gx, gy = eng.augment_train_indexed(xb, y, idx, p)
    assert torch.equal(gx, wx) and torch.equal(gy, wy)
    assert not torch.equal(gx, xf[torch.as_tensor(idx.astype(np.int64), device='cuda:0')])       # it did augment
    eng.close()


def test_bad_indices_into_a_byte_set_are_refused_before_any_launch():
    N = 5
    k = byte_images(N, 37, 53, seed=3)
    xb, y = dev(k), dev(np.random.RandomState(3).random_sample((N, 7, 11, 10)).astype(f32))
    p = dev(edge_params(4))
    eng = engine()
    for bad, pos in (([0, 1, -1, 2], 2), ([0, N, 1, 2], 1), ([1, 2, 3, 2 ** 31 - 1], 3), ([-2 ** 31, 0, 0, 0], 0)):
        for call in (lambda xo, yo: eng.gather_batch(xb, y, np.asarray(bad, np.int32), xo, yo),
                     lambda xo, yo: eng.augment_train_indexed(xb, y, np.asarray(bad, np.int32), p, xo, yo)):
            xo, yo = torch.full((4, 37, 53, 3), SENTINEL, device='cuda:0'), torch.full((4, 7, 11, 10), SENTINEL, device='cuda:0')
            with pytest.raises(RuntimeError) as ei:
                call(xo, yo)
            assert 'status 1' in str(ei.value) and 'idx[%d]' % pos in str(ei.value), str(ei.value)
            torch.cuda.synchronize()
            assert bool((xo == SENTINEL).all()) and bool((yo == SENTINEL).all())
    with pytest.raises(TypeError):                        # outputs stay float32
        eng.gather_batch(xb, y, [0], torch.empty((1, 37, 53, 3), dtype=torch.uint8, device='cuda:0'))
    eng.close()


# ------------------------------------------------------------------ DeviceDataset and the training run
def test_byte_device_dataset_uploads_bytes_and_converts_floats_chunk_by_chunk(tmp_path):
    k = byte_images(7, 16, 24, seed=5)
    y = np.random.RandomState(5).random_sample((7, 2, 3, 10)).astype(f32)
    px = str(tmp_path / 'x.npy')
    np.save(px, as_float(k))
    for src in (k, as_float(k), px):                       # bytes as they are; floats (array, memory-mapped file) through to_u8_exact
        ds = DeviceDataset(src, y, device=0, chunk_rows=3, image_dtype='uint8', rows=[6, 0, 3, 3, 5])
        assert ds.x.dtype == torch.uint8 and ds.y.dtype == torch.float32 and ds.nbytes == 5 * 16 * 24 * 3 + 5 * 2 * 3 * 10 * 4
        assert np.array_equal(ds.x.cpu().numpy(), k[[6, 0, 3, 3, 5]]) and np.array_equal(ds.y.cpu().numpy(), y[[6, 0, 3, 3, 5]])
    bad = as_float(k)
    bad[4, 3, 2, 1] = 0.5
    with pytest.raises(NotByteExact) as ei:
        DeviceDataset(bad, y, device=0, chunk_rows=3, image_dtype='uint8')
    assert ei.value.index == (4, 3, 2, 1) and ei.value.value == 0.5
    assert DeviceDataset(bad, y, device=0).x.dtype == torch.float32       # the default is unchanged


@pytest.fixture(scope='module')
def train_case():
    p = synth.make_pd_params(debug=True, bn='trained')
    p.update(synth.make_sm_params(synth.synthetic_priors(), kind='trained'))
    return p, M.byte_grid(synth.make_images(12, seed=71)), synth.make_targets(12, seed=72)


def run_training(p, x, y, gpus, augment, image_dtype):
    """Three steps of train_step_indexed (12 examples, batches of 4) -> losses per step and tower, final parameters per replica, the random states."""
    from joint_cnn_mrf_amd.dist import Towers
    from joint_cnn_mrf_amd.main import TowerTrainer
    towers = Towers(p, gpus)
    tt = TowerTrainer(towers, p, augment_rng=np.random.RandomState(31) if augment else None, optimizer='adam', lr=0.001, lmbd=0.001, use_sm=True)
    rng = np.random.RandomState(13)
    ds = DeviceDataset.for_towers(towers, x, y, chunk_rows=5, image_dtype=image_dtype)
    d0 = ds[towers.engines[0].device]
    assert len(ds) == 1 and d0.x.dtype == (torch.uint8 if image_dtype == 'uint8' else torch.float32)
    losses = []
    for batch_idx in d0.epoch_indices(rng, 4, shuffle=True):
        tt.train_step_indexed(ds, batch_idx)
        losses.append(torch.stack([tr.losses for tr in tt.trainers]).cpu().numpy())
        assert all(tr.last_batch[0].dtype == torch.float32 for tr in tt.trainers)
    flat = [np.concatenate([v.reshape(-1) for _k, v in sorted(tr.get_params(p).items())]) for tr in tt.trainers]
    towers.close()
    return np.stack(losses), np.stack(flat), (rng.random_sample(), tt.augment_rng.random_sample() if augment else None)


@pytest.mark.parametrize('augment', [False, True], ids=['plain', 'augmented'])
@pytest.mark.parametrize('gpus', [[0], [0, 0]], ids=['one_tower', 'two_towers'])
def test_training_on_a_byte_dataset_equals_training_on_the_float_one(train_case, gpus, augment):
    p, k, y = train_case
    lf, pf, rf = run_training(p, as_float(k), y, gpus, augment, 'float32')
    lb, pb, rb = run_training(p, k, y, gpus, augment, 'uint8')
    assert lf.shape == (3, len(gpus), 4) and np.isfinite(lf).all() and np.isfinite(pf).all()
    assert rf == rb
    assert np.array_equal(lb, lf), 'losses differ by %g' % float(np.abs(lb - lf).max())
    assert np.array_equal(pb, pf), 'parameters differ by %g' % float(np.abs(pb - pf).max())


# ------------------------------------------------------------------ the streamed feed
@pytest.mark.parametrize('kind', ['uint8', 'float32'])
@pytest.mark.parametrize('use_sm', [True, False])
def test_forward_stream_equals_forward_per_batch_in_order(kind, use_sm):
    from joint_cnn_mrf_amd.stream import ForwardStream, forward_stream
    k = byte_images(14, 480, 720, seed=9)
    x = k if kind == 'uint8' else as_float(k)
    torso = synth.make_torso(14, seed=10)
    bounds = [(0, 3), (3, 6), (6, 9), (9, 12), (12, 14)]              # five batches, the last one short
    eng = engine().load_params(params(True))
    want = []
    for lo, hi in bounds:
        r = eng.forward(dev(x[lo:hi]), dev(torso[lo:hi]) if use_sm else None, use_sm=use_sm, want_prob=False)
        want.append({key: v.cpu().numpy() for key, v in r.items()})
    assert any(not np.array_equal(want[0]['pd_coords'], w['pd_coords'][:3]) for w in want[1:4])      # the batches are told apart
    fed = []

    def batches():
        for lo, hi in bounds:
            fed.append(lo)
            yield x[lo:hi], (torso[lo:hi] if use_sm else None)
    fs = ForwardStream(eng, use_sm=use_sm, depth=2)
    got, fed_at_yield = [], []
    for r in fs.run(batches()):
        got.append(r)
        fed_at_yield.append(len(fed))
    assert len(got) == 5 and fed_at_yield[0] == 3                      # never more than depth = 2 batches in flight: result 0 arrives when batch 2 is asked for
    for w, g in zip(want, got):
        assert sorted(g) == sorted(w)
        for key in w:
            assert isinstance(g[key], np.ndarray) and g[key].dtype == np.int32 and np.array_equal(g[key], w[key]), key
    assert eng._stream.query() and fs.copy_stream.query()              # nothing pending on either stream
    assert fs.bytes_uploaded == x.nbytes + (torso.nbytes if use_sm else 0)
    got2 = list(forward_stream(eng, batches(), use_sm=use_sm, depth=3))
    assert all(np.array_equal(a[key], b[key]) for a, b in zip(got, got2) for key in a)
    with pytest.raises(TypeError):
        list(forward_stream(eng, [(x[:2].astype(np.float64), torso[:2])], use_sm=use_sm))
    eng.close()


# ------------------------------------------------------------------ command line
def _run_ok(args, cwd):
    r = run_cli(args, cwd, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return r.stdout.splitlines()


def test_cli_evaluation_on_bytes_writes_the_predictions_of_a_direct_forward(tmp_path):
    import scipy.io
    from joint_cnn_mrf_amd.dist import Towers
    B, n = 4, 10
    mat = str(tmp_path / 'predictions.mat')
    out = _run_ok(['--synthetic', '--debug', '--use_sm', '--u8_images', '--batch_size', str(B), '--synthetic_size', str(n), '--predictions', mat], str(tmp_path))
    line = json.loads([l for l in out if l.startswith('{')][-1])
    assert line['image_dtype'] == 'uint8' and line['n_images'] == 8
    assert line['bytes_uploaded'] == 8 * (480 * 720 * 3 + 60 * 90 * 4)
    got = scipy.io.loadmat(mat)
    # the same run by hand: the generated test images on the byte grid, one Towers.forward per whole batch
    args = M.build_parser().parse_args(['--synthetic', '--debug', '--use_sm'])
    p = M.initial_params(args, synth.synthetic_priors())
    _, _, x_test, y_test = M._synthetic_dataset(B, n)
    k = M.byte_grid(x_test)
    tw = Towers(p, [0])
    pd, sm = [], []
    for lo in (0, 4):
        r = tw.forward(k[lo:lo + B], np.ascontiguousarray(y_test[lo:lo + B, :, :, 9:]), use_sm=True)
        pd.append(r['pd_coords'])
        sm.append(r['sm_coords'])
    tw.close()
    to_ref = lambda c: torch.cat(c).permute(1, 2, 0).cpu().numpy()
    assert np.array_equal(got['flic_pred_pd'], to_ref(pd)) and np.array_equal(got['flic_pred_sm'], to_ref(sm))


def test_cli_training_on_bytes_prints_finite_epoch_lines_and_saves_a_checkpoint(tmp_path):
    from joint_cnn_mrf_amd import tf_checkpoint
    out = _run_ok(['--train', '--device_data', '--u8_images', '--synthetic', '--debug', '--use_sm', '--synthetic_size', '8', '--batch_size', '4',
                '--n_epochs', '2', '--model_path', str(tmp_path / 'm')], str(tmp_path))
    epochs = [l for l in out if l.startswith('Epoch ')]
    assert [l.split()[1] for l in epochs] == ['0', '1', '2']
    for l in epochs:
        nums = [float(t) for t in l.split()[3:] if t[0].isdigit() or t[0] == '-']
        assert len(nums) == 8 and np.isfinite(nums).all(), l
    held = [l for l in out if l.startswith('device data (') and 'uint8' in l]
    assert len(held) == 2 and str(8 * 480 * 720 * 3 + 8 * 60 * 90 * 10 * 4) in held[1]
    ckpts = sorted(f for f in os.listdir(tmp_path / 'm') if f.endswith('.index'))
    assert len(ckpts) == 1 and ckpts[0].endswith('-2.index')
    state = tf_checkpoint.load_checkpoint(str(tmp_path / 'm' / ckpts[0][:-len('.index')]))
    assert 'conv1_fullres/weights' in state and all(np.isfinite(v).all() for v in state.values())
