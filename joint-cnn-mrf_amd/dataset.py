"""A data set that lives in device memory.

FLIC in fp32 is 16.5 GB (train) + 4.2 GB (test); an MI355X has 288 GB.  `DeviceDataset` uploads the two arrays once, in chunks
through two pinned staging buffers (one is copied to the device while the other is filled from the file), and a batch is then a
gather by index on the device (`Engine.gather_batch`), or the source of the augmentation directly
(`Engine.augment_train_indexed`).  `epoch_indices` draws the batches exactly as `evaluation.get_next_batch` does, so a run fed
from the device sees the batches of a host-fed run with the same seed.  A set that does not fit raises
`DeviceDataTooLarge`: there is no silent fall-back to the host path and no prefetching for larger sets.
"""
import numpy as np
import torch

DEFAULT_CHUNK_BYTES = 256 << 20      # per staging buffer


class DeviceDataTooLarge(RuntimeError):
    """The data set does not fit into the device memory it may use."""


def plan_chunks(n, chunk_rows):
    """[(lo, hi), ...]: consecutive row ranges of at most chunk_rows rows that cover [0, n) exactly once (the last may be shorter)."""
    n, chunk_rows = int(n), int(chunk_rows)
    if n < 0 or chunk_rows < 1:
        raise ValueError('plan_chunks needs n >= 0 and chunk_rows >= 1; got %d, %d' % (n, chunk_rows))
    return [(lo, min(lo + chunk_rows, n)) for lo in range(0, n, chunk_rows)]


def epoch_indices(n, rng, batch_size, shuffle=True):
    """The [n_batches, batch_size] int32 index table of one epoch over n examples.  Consumes `rng` exactly as
    evaluation.get_next_batch (main.py:184-192) does: one permutation(n) when shuffling, nothing otherwise; whole batches only."""
    n_batches = n // batch_size
    idx = (rng or np.random).permutation(n)[:n_batches * batch_size] if shuffle else np.arange(n)[:n_batches * batch_size]
    return idx.reshape([n_batches, batch_size]).astype(np.int32)


def _open(a):
    return np.load(a, mmap_mode='r') if isinstance(a, (str, bytes)) or hasattr(a, '__fspath__') else a


class DeviceDataset:
    """x [N,H,W,3], y [N,h,w,K+1] as fp32 device tensors `.x`, `.y` on `device`.

    x, y: numpy arrays, np.memmap or paths of .npy files (opened memory-mapped).  rows: optional row subset (the --debug
    selection), taken in the order given.  chunk_rows: rows per staging buffer (default: DEFAULT_CHUNK_BYTES worth of images).
    budget_bytes: the device memory the set may take; default: what torch.cuda.mem_get_info reports free, less reserve_bytes
    (room the engines have not claimed yet: workspace, the filter-spectra cache)."""

    def __init__(self, x, y, device=0, rows=None, chunk_rows=None, budget_bytes=None, reserve_bytes=0):
        x, y = _open(x), _open(y)
        if x.ndim != 4 or y.ndim != 4 or x.shape[3] != 3 or x.shape[0] != y.shape[0]:
            raise ValueError('DeviceDataset expects x [N,H,W,3] and y [N,h,w,K+1] with the same N; got %s, %s' % (x.shape, y.shape))
        if rows is not None:
            rows = np.asarray(rows, np.int64).reshape(-1)
            if rows.size and (rows.min() < 0 or rows.max() >= x.shape[0]):
                raise IndexError('rows outside [0, %d)' % x.shape[0])
        self.n = int(x.shape[0] if rows is None else rows.size)
        if self.n < 1:
            raise ValueError('DeviceDataset needs at least one example')
        self.device = torch.device('cuda', device if isinstance(device, int) else torch.device(device).index or 0)
        shape_x, shape_y = (self.n,) + tuple(x.shape[1:]), (self.n,) + tuple(y.shape[1:])
        self.nbytes = 4 * (int(np.prod(shape_x)) + int(np.prod(shape_y)))
        if budget_bytes is None:
            free, total = torch.cuda.mem_get_info(self.device)
            budget_bytes, where = free - int(reserve_bytes), '%d bytes free of %d on %s, %d of them reserved for the engines' % (free, total, self.device, reserve_bytes)
        else:
            where = 'the budget given'
        if self.nbytes > budget_bytes:
            raise DeviceDataTooLarge('the data set needs %d bytes (%d examples: x %s, y %s, fp32) and may use %d (%s); a set that does not fit '
                                     'is not prefetched from the host: train without device data' % (self.nbytes, self.n, shape_x[1:], shape_y[1:], budget_bytes, where))
        with torch.cuda.device(self.device):
            self.x = torch.empty(shape_x, dtype=torch.float32, device=self.device)
            self.y = torch.empty(shape_y, dtype=torch.float32, device=self.device)
            import time
            t0 = time.perf_counter()
            stream = torch.cuda.Stream(device=self.device)
            for src, dst in ((x, self.x), (y, self.y)):
                self._upload(src, dst, rows, chunk_rows, stream)
            stream.synchronize()         # one-off: afterwards the tensors are safe to read from any stream
            self.upload_seconds = time.perf_counter() - t0

    @staticmethod
    def _upload(src, dst, rows, chunk_rows, stream):
        n = dst.shape[0]
        row_elems = int(np.prod(dst.shape[1:]))
        if chunk_rows is None:
            chunk_rows = max(1, DEFAULT_CHUNK_BYTES // (4 * row_elems))
        chunk_rows = min(int(chunk_rows), n)
        flat = dst.view(n, row_elems)
        stage = [torch.empty((chunk_rows, row_elems), dtype=torch.float32).pin_memory() for _ in range(2)]
        done = [None, None]
        for i, (lo, hi) in enumerate(plan_chunks(n, chunk_rows)):
            k = i % 2
            if done[k] is not None:
                done[k].synchronize()        # the copy that last read this buffer; the other buffer's copy runs meanwhile
            part = src[lo:hi] if rows is None else src[rows[lo:hi]]
            np.copyto(stage[k][:hi - lo].numpy(), np.asarray(part).reshape(hi - lo, row_elems), casting='same_kind')
            with torch.cuda.stream(stream):
                flat[lo:hi].copy_(stage[k][:hi - lo], non_blocking=True)
                done[k] = torch.cuda.Event()
                done[k].record(stream)
        for ev in done:
            if ev is not None:
                ev.synchronize()             # the staging buffers are freed on return

    def __len__(self):
        return self.n

    def epoch_indices(self, rng, batch_size, shuffle=True):
        return epoch_indices(self.n, rng, batch_size, shuffle)

    @classmethod
    def for_towers(cls, towers, x, y, **kw):
        """{device: DeviceDataset}: one copy per distinct device of the towers (`--gpus 0 0` shares one)."""
        x, y = _open(x), _open(y)
        out = {}
        for eng in towers.engines:
            if eng.device not in out:
                out[eng.device] = cls(x, y, device=eng.device, **kw)
        return out
