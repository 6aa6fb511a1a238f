"""Device-resident training data on the GPU: jcm_gather_batch against torch indexing, the host-side index
checks, jcm_augment_train_indexed against gather + jcm_augment_train, DeviceDataset's chunked upload and its size check, a
training run fed by index against the host-fed run from the same seeds (Trainer / TowerTrainer, one and two towers, without
and with augmentation), and `--device_data` on the command line.  Everything compared here is compared bit for bit, except
where two runs of the HOST-fed loop differ from each other (then twice their largest difference is allowed, and said)."""
import ctypes
import os

import numpy as np
import pytest
import torch

from cli_util import run_cli
import joint_cnn_mrf_amd  # noqa: F401
from joint_cnn_mrf_amd import _lib, evaluation, synth
from joint_cnn_mrf_amd.dataset import DeviceDataset, DeviceDataTooLarge
from test_gpu_augment import edge_params          # the parameter set of the augmentation's own tests

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
SENTINEL = -7.25


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), device='cuda:0')


def engine(**kw):
    from joint_cnn_mrf_amd.engine import Engine
    return Engine(device=0, **kw)


def data(N, H, W, h, w, seed=0):
    rs = np.random.RandomState(seed)
    return dev(rs.random_sample((N, H, W, 3)).astype(f32)), dev(rs.random_sample((N, h, w, 10)).astype(f32))


# ------------------------------------------------------------------ gather
GATHER_CASES = {
    'full_size_b14': (20, 480, 720, 60, 90, [3, 19, 0, 7, 7, 12, 1, 18, 5, 2, 11, 16, 9, 4]),
    'odd_37x53_7x11': (6, 37, 53, 7, 11, [5, 1, 1, 0, 4, 3, 2]),                  # 23 532 and 3 080 bytes per image: 4-byte pieces
    'small_6x10_2x2': (5, 6, 10, 2, 2, [4, 0, 2, 2, 1, 3]),
    'wide_x_narrow_y': (4, 8, 8, 7, 11, [1, 3, 0]),                               # 768 bytes per image, 3 080 per map: one route each
    'narrow_x_wide_y': (4, 37, 53, 2, 2, [2, 2, 3, 0, 1]),
    'one_example': (1, 37, 53, 7, 11, [0]),
    'one_example_repeated': (1, 480, 720, 60, 90, [0, 0, 0]),
    'more_than_the_set': (3, 6, 10, 2, 2, [2, 0, 1, 1, 2, 0, 0, 2]),
    'several_launches': (7, 6, 10, 2, 2, list(np.random.RandomState(1).randint(0, 7, 600))),   # > 256 images: the batch is cut into launches
}


@pytest.mark.parametrize('case', sorted(GATHER_CASES))
def test_gather_equals_torch_indexing(case):
    N, H, W, h, w, idx = GATHER_CASES[case]
    x, y = data(N, H, W, h, w, seed=len(case))
    eng = engine()
    xo, yo = eng.gather_batch(x, y, np.asarray(idx))
    t = torch.as_tensor(np.asarray(idx, np.int64), device='cuda:0')
    assert xo.shape == (len(idx), H, W, 3) and yo.shape == (len(idx), h, w, 10)
    assert torch.equal(xo, x[t]) and torch.equal(yo, y[t])
    # into given buffers, and from a slice of the set whose first image is not the allocation's first
    xb, yb = torch.full_like(xo, SENTINEL), torch.full_like(yo, SENTINEL)
    r = eng.gather_batch(x, y, list(idx), xb, yb)
    assert r[0] is xb and r[1] is yb and torch.equal(xb, x[t]) and torch.equal(yb, y[t])
    if N > 1:
        sub = np.asarray(idx) % (N - 1)
        xs, ys = eng.gather_batch(x[1:], y[1:], sub)
        ts = torch.as_tensor(sub.astype(np.int64), device='cuda:0')
        assert torch.equal(xs, x[1:][ts]) and torch.equal(ys, y[1:][ts])
    eng.close()


def test_bad_indices_are_refused_on_the_host_and_nothing_is_written():
    """The host check only: no launch ever sees an index outside [0, N)."""
    N = 5
    x, y = data(N, 37, 53, 7, 11, seed=3)
    p = dev(edge_params(4))
    eng = engine()
    for bad, pos in (([0, 1, -1, 2], 2), ([0, N, 1, 2], 1), ([1, 2, 3, 2 ** 31 - 1], 3), ([-2 ** 31, 0, 0, 0], 0)):
        for call in (lambda xo, yo: eng.gather_batch(x, y, np.asarray(bad, np.int32), xo, yo),
                     lambda xo, yo: eng.augment_train_indexed(x, y, np.asarray(bad, np.int32), p, xo, yo)):
            xo, yo = torch.full((4, 37, 53, 3), SENTINEL, device='cuda:0'), torch.full((4, 7, 11, 10), SENTINEL, device='cuda:0')
            with pytest.raises(RuntimeError) as ei:
                call(xo, yo)
            assert 'status 1' in str(ei.value) and 'idx[%d]' % pos in str(ei.value), str(ei.value)      # JCM_ERR_ARG, the position named
            torch.cuda.synchronize()
            assert bool((xo == SENTINEL).all()) and bool((yo == SENTINEL).all())
    # the C entry point itself: null pointers, bad sizes, outputs inside the data set
    lib, P = _lib.load(), eng._p
    idx = np.asarray([0, 1], np.int32)
    ip = idx.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
    xo, yo = torch.empty((2, 37, 53, 3), device='cuda:0'), torch.empty((2, 7, 11, 10), device='cuda:0')
    g = lambda xa, ya, n, i, B, xout, yout, H=37: lib.jcm_gather_batch(eng._h, P(xa), P(ya), n, i, B, H, 53, 7, 11, P(xout), P(yout))
    assert g(x, y, N, ip, 2, xo, yo) == 0
    torch.cuda.synchronize()
    assert g(None, y, N, ip, 2, xo, yo) == 1 and g(x, y, N, None, 2, xo, yo) == 1 and g(x, y, N, ip, 2, xo, None) == 1
    assert g(x, y, 0, ip, 2, xo, yo) == 1 and g(x, y, N, ip, 0, xo, yo) == 1 and g(x, y, N, ip, 2, xo, yo, H=0) == 1
    assert g(x, y, N, ip, 2, x[3:], yo) == 1 and g(x, y, N, ip, 2, xo, y[2:]) == 1 and g(x, y, N, ip, 2, xo, xo) == 1
    assert 'overlap' in _lib.last_error()
    a = lambda pp, xout: lib.jcm_augment_train_indexed(eng._h, P(x), P(y), N, ip, P(pp), 2, 37, 53, 7, 11, P(xout), P(yo))
    assert a(p, xo) == 0
    torch.cuda.synchronize()
    assert a(None, xo) == 1 and a(p, x[1:]) == 1
    # the Python layer: idx must be a host array of integers, shapes must agree
    with pytest.raises(ValueError):
        eng.gather_batch(x, y, torch.zeros(2, dtype=torch.int32, device='cuda:0'))
    with pytest.raises(ValueError):
        eng.gather_batch(x, y, np.zeros(2, f32))
    with pytest.raises(ValueError):
        eng.gather_batch(x, y[:4], [0])
    with pytest.raises(ValueError):
        eng.augment_train_indexed(x, y, [0, 1, 2], p)            # four parameter rows, three indices
    eng.close()


# ------------------------------------------------------------------ indexed augmentation
@pytest.mark.parametrize('precision', ['fp32', 'bf16'])
@pytest.mark.parametrize('shape', [(480, 720, 60, 90), (37, 53, 7, 11)])
def test_indexed_augmentation_equals_gather_then_augment(shape, precision):
    H, W, h, w = shape
    N, idx = 9, np.asarray([8, 2, 2, 0, 5, 7, 1], np.int32)
    x, y = data(N, H, W, h, w, seed=H)
    p = dev(edge_params(len(idx), seed=11))
    eng = engine(precision=precision)
    want = eng.augment_train(*eng.gather_batch(x, y, idx), p)
    got = eng.augment_train_indexed(x, y, idx, p)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    assert not torch.equal(got[0], x[torch.as_tensor(idx.astype(np.int64), device='cuda:0')])       # it did augment
    eng.close()


# ------------------------------------------------------------------ DeviceDataset
def test_device_dataset_uploads_a_memory_mapped_pair_in_uneven_chunks(tmp_path):
    rs = np.random.RandomState(5)
    x, y = rs.random_sample((7, 16, 24, 3)).astype(f32), rs.random_sample((7, 2, 3, 10)).astype(f32)
    px, py = str(tmp_path / 'x.npy'), str(tmp_path / 'y.npy')
    np.save(px, x)
    np.save(py, y)
    ds = DeviceDataset(px, py, device=0, chunk_rows=3)                    # chunks of 3, 3, 1 through two staging buffers
    assert len(ds) == 7 and ds.x.is_cuda and ds.x.dtype == torch.float32 and ds.nbytes == x.nbytes + y.nbytes
    assert np.array_equal(ds.x.cpu().numpy(), x) and np.array_equal(ds.y.cpu().numpy(), y)
    mm = DeviceDataset(np.load(px, mmap_mode='r'), np.load(py, mmap_mode='r'), device=0, chunk_rows=2, rows=[6, 0, 3, 3, 5])
    assert len(mm) == 5 and np.array_equal(mm.x.cpu().numpy(), x[[6, 0, 3, 3, 5]]) and np.array_equal(mm.y.cpu().numpy(), y[[6, 0, 3, 3, 5]])
    whole = DeviceDataset(x, y, device=0)                                 # one chunk
    assert torch.equal(whole.x, ds.x) and torch.equal(whole.y, ds.y)
    with pytest.raises(DeviceDataTooLarge) as ei:
        DeviceDataset(px, py, device=0, budget_bytes=x.nbytes + y.nbytes - 1)
    assert str(x.nbytes + y.nbytes) in str(ei.value) and str(x.nbytes + y.nbytes - 1) in str(ei.value)
    with pytest.raises(DeviceDataTooLarge):
        DeviceDataset(px, py, device=0, reserve_bytes=1 << 50)            # nothing is left beside such a reservation
    DeviceDataset(px, py, device=0, budget_bytes=x.nbytes + y.nbytes)     # exactly enough
    # the device tensors go straight into eval_error's batching
    bx, by = next(evaluation.get_next_batch(ds.x[:6], ds.y[:6], 4))
    assert bx.is_cuda and np.array_equal(bx.cpu().numpy(), x[:4]) and np.array_equal(by.cpu().numpy(), y[:4])


# ------------------------------------------------------------------ the same training run
@pytest.fixture(scope='module')
def train_case():
    p = synth.make_pd_params(debug=True, bn='trained')
    p.update(synth.make_sm_params(synth.synthetic_priors(), kind='trained'))
    return p, synth.make_images(8, seed=71), synth.make_targets(8, seed=72)


def run_training(params, x, y, gpus, augment, indexed, batch_size=4, n_epochs=2):
    """The epoch loop of train_main on either route -> per step: the losses of every tower and the batch each tower's step was handed;
    at the end every stored parameter of every replica, flat."""
    from joint_cnn_mrf_amd.dist import Towers
    from joint_cnn_mrf_amd.main import TowerTrainer
    towers = Towers(params, gpus)
    tt = TowerTrainer(towers, params, augment_rng=np.random.RandomState(31) if augment else None, optimizer='adam', lr=0.001, lmbd=0.001, use_sm=True)
    rng = np.random.RandomState(13)
    ds = DeviceDataset.for_towers(towers, x, y, chunk_rows=3) if indexed else None
    if indexed:
        assert len(ds) == 1                                               # `--gpus 0 0` shares one copy
    losses, batches = [], []

    def record():
        losses.append(torch.stack([tr.losses for tr in tt.trainers]).cpu().numpy())
        batches.append([(tr.last_batch[0].cpu().numpy(), tr.last_batch[1].cpu().numpy()) for tr in tt.trainers])
    for _epoch in range(n_epochs):
        if indexed:
            for batch_idx in ds[towers.engines[0].device].epoch_indices(rng, batch_size, shuffle=True):
                tt.train_step_indexed(ds, batch_idx)
                record()
        else:
            for bx, by in evaluation.get_next_batch(x, y, batch_size, shuffle=True, rng=rng):
                tt.train_step(np.ascontiguousarray(bx, f32), np.ascontiguousarray(by, f32))
                record()
    flat = [np.concatenate([v.reshape(-1) for _k, v in sorted(tr.get_params(params).items())]) for tr in tt.trainers]
    towers.close()
    return np.stack(losses), batches, np.stack(flat), (rng.random_sample(), tt.augment_rng.random_sample() if augment else None)


@pytest.mark.parametrize('augment', [False, True], ids=['plain', 'augmented'])
@pytest.mark.parametrize('gpus', [[0], [0, 0]], ids=['one_tower', 'two_towers'])
def test_indexed_training_run_equals_the_host_fed_run(train_case, gpus, augment):
    params, x, y = train_case
    la, ba, pa, ra = run_training(params, x, y, gpus, augment, indexed=False)
    lb, bb, pb, rb = run_training(params, x, y, gpus, augment, indexed=False)
    li, bi, pi, ri = run_training(params, x, y, gpus, augment, indexed=True)
    assert la.shape == (4, len(gpus), 4) and np.isfinite(la).all() and np.isfinite(pa).all()
    assert ra == rb == ri                                                 # both random states were consumed alike
    # the batches handed to the step: bit for bit, on every tower, at every step (the host-fed loop is deterministic here by construction:
    # host slices, and an augmentation whose sums have a fixed order)
    for step, (host, again, idxd) in enumerate(zip(ba, bb, bi)):
        for tower, ((hx, hy), (ax, ay), (ix, iy)) in enumerate(zip(host, again, idxd)):
            assert np.array_equal(hx, ax) and np.array_equal(hy, ay), 'host-fed batches differ between two runs (step %d, tower %d)' % (step, tower)
            assert np.array_equal(hx, ix) and np.array_equal(hy, iy), 'the indexed batch differs from the host-fed one (step %d, tower %d)' % (step, tower)
    # losses and final parameters: equal to the host-fed run to the extent the host-fed run equals itself
    dl, dp = float(np.abs(la - lb).max()), float(np.abs(pa - pb).max())
    print('host-fed run against itself: max |d loss| = %g, max |d param| = %g; indexed against host-fed: %g, %g'
          % (dl, dp, float(np.abs(li - la).max()), float(np.abs(pi - pa).max())))
    if dl == 0.0 and dp == 0.0 and np.array_equal(la, lb) and np.array_equal(pa, pb):
        assert np.array_equal(li, la), 'two host-fed runs agree bit for bit, the indexed run differs in the losses by %g' % float(np.abs(li - la).max())
        assert np.array_equal(pi, pa), 'two host-fed runs agree bit for bit, the indexed run differs in the parameters by %g' % float(np.abs(pi - pa).max())
    else:
        note = 'two host-fed runs differ from each other (losses by %g, parameters by %g): twice that is allowed' % (dl, dp)
        assert float(np.abs(li - la).max()) <= 2 * dl, note
        assert float(np.abs(pi - pa).max()) <= 2 * dp, note


# ------------------------------------------------------------------ command line
def _run_ok(args, cwd):
    r = run_cli(args, cwd, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return [l for l in r.stdout.splitlines() if l.startswith('Epoch ')]


def test_cli_device_data_prints_the_epoch_lines_of_the_host_fed_run(tmp_path):
    common = ['--train', '--debug', '--use_sm', '--synthetic', '--synthetic_size', '8', '--batch_size', '4', '--n_epochs', '2']
    runs = {}
    for name, extra in (('host', []), ('host_again', []), ('device', ['--device_data'])):
        runs[name] = _run_ok(common + extra + ['--model_path', str(tmp_path / name)], str(tmp_path))
        assert [l.split()[1] for l in runs[name]] == ['0', '1', '2'] and 'test_dr' in runs[name][0] and 'train_mse' in runs[name][0]
        ckpts = sorted(f for f in os.listdir(tmp_path / name) if f.endswith('.index'))
        assert len(ckpts) == 1 and ckpts[0].endswith('-2.index')
    print('\n'.join('%-10s %s' % (k, l) for k, v in runs.items() for l in v))
    if runs['host'] == runs['host_again']:
        assert runs['device'] == runs['host']
    else:
        num = lambda lines: np.asarray([[float(t) for t in l.split()[3:] if t[0].isdigit() or t[0] == '-'] for l in lines])
        d = float(np.abs(num(runs['host']) - num(runs['host_again'])).max())
        assert float(np.abs(num(runs['device']) - num(runs['host'])).max()) <= 2 * d, \
            'two host-fed runs print different Epoch lines (largest difference %g): twice that is allowed' % d
