"""Feeding the tower from host memory: `forward_stream` runs `Engine.forward` over a sequence of host batches with the
upload of batch i+1 overlapping the forward of batch i.

`depth` slots, each a pinned staging set (x, torso), a device set and a pinned result set.  Two streams: the copy stream uploads, the
engine's stream computes and reads the coordinates back.  Two events per slot order them, all recorded and waited for on the device
(the host blocks only where it must touch pinned memory):

  copied[k]    on the copy stream behind the upload of slot k      -> the engine's stream waits for it before the forward;
                                                                       the host waits for it before it refills the staging set
  finished[k]  on the engine's stream behind the forward + read-back -> the copy stream waits for it before it overwrites the device set;
                                                                       the host waits for it before it reads the results (and so before
                                                                       slot k is reused at all: at most `depth` batches are in flight)

Byte images (uint8) are uploaded as bytes and read by the byte-source conv1 kernels: a quarter of the link traffic of float32 images, the
same results bit for bit."""
import numpy as np
import torch


class ForwardStream:
    """The state behind forward_stream: streams, events and buffers, allocated for the first batch's shape and dtype.  `copy_stream` and
    `bytes_uploaded` are there for tools and tests."""

    def __init__(self, engine, use_sm=True, depth=2):
        if int(depth) < 1:
            raise ValueError('depth must be >= 1, got %r' % (depth,))
        self.engine, self.use_sm, self.depth = engine, bool(use_sm), int(depth)
        self.copy_stream = torch.cuda.Stream(device=engine.device)
        self.bytes_uploaded = 0
        self._slots = None

    def _alloc(self, x, torso):
        e, K = self.engine, self.engine.n_joints
        tdt = torch.uint8 if x.dtype == np.uint8 else torch.float32
        self._shape, self._dtype = tuple(x.shape), x.dtype
        self._slots = []
        for _ in range(self.depth):
            s = {'hx': torch.empty(x.shape, dtype=tdt).pin_memory(), 'dx': torch.empty(x.shape, dtype=tdt, device=e.device),
                 'out': {k: torch.empty((x.shape[0], 2, K), dtype=torch.int32).pin_memory() for k in (('pd_coords', 'sm_coords') if self.use_sm else ('pd_coords',))},
                 'copied': torch.cuda.Event(), 'finished': torch.cuda.Event(), 'n': 0}
            if self.use_sm:
                s['ht'] = torch.empty(torso.shape, dtype=torch.float32).pin_memory()
                s['dt'] = torch.empty(torso.shape, dtype=torch.float32, device=e.device)
            self._slots.append(s)

    def _check(self, x, torso):
        if not isinstance(x, np.ndarray) or x.dtype not in (np.uint8, np.float32) or x.ndim != 4 or x.shape[3] != 3 or x.shape[0] < 1:
            raise TypeError('forward_stream: x must be a host uint8 or float32 array [B,H,W,3], got %s' % (getattr(x, 'dtype', type(x)),))
        if self.use_sm:
            if not isinstance(torso, np.ndarray) or torso.dtype != np.float32 or tuple(torso.shape) != (x.shape[0], 60, 90, 1):
                raise ValueError('forward_stream: use_sm needs torso as a host float32 array [%d,60,90,1]' % x.shape[0])
        if self._slots is None:
            self._alloc(x, torso)
        elif x.dtype != self._dtype or x.shape[1:] != self._shape[1:] or x.shape[0] > self._shape[0]:
            raise ValueError('forward_stream: a batch of %s %s after the first of %s %s (later batches share its dtype and image size and are not larger)'
                             % (x.dtype, x.shape, self._dtype, self._shape))

    def _result(self, s):
        s['finished'].synchronize()
        n, s['n'] = s['n'], 0
        return {k: v[:n].numpy().copy() for k, v in s['out'].items()}

    def run(self, batches):
        e = self.engine
        es, cs = e._stream, self.copy_stream
        i = 0
        for x, torso in batches:
            self._check(x, torso)
            s = self._slots[i % self.depth]
            if s['n']:                               # the batch that used this slot `depth` batches ago: its results are due now
                yield self._result(s)                # (waits for finished[k]: the copy and the forward that read this slot are over)
            n = x.shape[0]
            s['copied'].synchronize()                # (implied by finished[k]; never-recorded events return at once)
            np.copyto(s['hx'].numpy()[:n], x, casting='no')
            if self.use_sm:
                np.copyto(s['ht'].numpy()[:n], torso, casting='no')
            with torch.cuda.stream(cs):
                cs.wait_event(s['finished'])         # the forward that last read the device set
                s['dx'][:n].copy_(s['hx'][:n], non_blocking=True)
                if self.use_sm:
                    s['dt'][:n].copy_(s['ht'][:n], non_blocking=True)
                s['copied'].record(cs)
            self.bytes_uploaded += x.nbytes + (torso.nbytes if self.use_sm else 0)
            with torch.cuda.device(e.device), torch.cuda.stream(es):
                es.wait_event(s['copied'])
                r = e.forward(s['dx'][:n], s['dt'][:n] if self.use_sm else None, use_sm=self.use_sm, want_prob=False)
                for k, v in s['out'].items():
                    v[:n].copy_(r[k], non_blocking=True)
                s['finished'].record(es)
            s['n'] = n
            i += 1
        for j in range(i, i + self.depth):           # drain, oldest first
            s = self._slots[j % self.depth] if self._slots else None
            if s is not None and s['n']:
                yield self._result(s)


def forward_stream(engine, batches, use_sm=True, depth=2):
    """Engine.forward over host batches, uploads overlapped with compute.  `batches` yields (x, torso): x uint8 or float32 [B,H,W,3], torso
    float32 [B,60,90,1] or None (use_sm=False); all batches share the first one's dtype and image size, none is larger (the last may be
    shorter).  Yields, in order, {'pd_coords', 'sm_coords'} as host int32 arrays [B,2,K] ('pd_coords' alone without use_sm): each equals
    Engine.forward on that batch bit for bit.  At most `depth` batches are in flight; results come `depth` batches behind the input."""
    yield from ForwardStream(engine, use_sm=use_sm, depth=depth).run(batches)
