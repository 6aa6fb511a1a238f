"""A data set that lives in device memory.

FLIC in fp32 is 16.5 GB (train) + 4.2 GB (test); an MI355X has 288 GB.  `DeviceDataset` uploads the two arrays once, in chunks
through two pinned staging buffers (one is copied to the device while the other is filled from the file), and a batch is then a
gather by index on the device (`Engine.gather_batch`), or the source of the augmentation directly
(`Engine.augment_train_indexed`).  `epoch_indices` draws the batches exactly as `evaluation.get_next_batch` does, so a run fed
from the device sees the batches of a host-fed run with the same seed.  A set that does not fit raises
`DeviceDataTooLarge`: there is no silent fall-back to the host path and no prefetching for larger sets.

`image_dtype='uint8'` holds the images as the bytes they were made from: data.load_image computes every value as
float32(k) / float32(255), so the byte image is the float image at a quarter of the memory (FLIC: 4.1 + 1.05 GB), of the upload and of the
gather's reads.  Float input is converted by `to_u8_exact`, which proves the round trip and refuses data that is not on that grid.
"""
import numpy as np
import torch

DEFAULT_CHUNK_BYTES = 256 << 20      # per staging buffer


class DeviceDataTooLarge(RuntimeError):
    """The data set does not fit into the device memory it may use."""


class NotByteExact(ValueError):
    """An image value is not float32(k) / float32(255) for a byte k: storing it as a byte would change it."""

    def __init__(self, index, value):
        self.index, self.value = tuple(int(i) for i in index), value
        super().__init__('image value %r at index %s is not float32(k) / float32(255) for any byte k: it cannot be stored as uint8 without '
                         'rounding (image_dtype=\'uint8\' holds byte images only)' % (value, self.index))


_F255 = np.float32(255)


CONVERT_ROWS_BYTES = 32 << 20      # to_u8_exact works on slices of this many source bytes: its temporaries stay a few times that, whatever the array


def to_u8_exact(a):
    """The byte image of a float image made as float32(k) / float32(255) (data.load_image): rint(a * 255) as uint8, VERIFIED -- the bytes
    widened by that same division must give back `a` bit for bit, otherwise NotByteExact names the first offending index and value (NaN,
    values outside [0, 1] and values off the grid all fail it).  A uint8 array is returned unchanged."""
    a = np.asarray(a)
    if a.dtype == np.uint8:
        return a
    if a.dtype != np.float32:
        raise TypeError('to_u8_exact takes float32 or uint8 images, got %s' % a.dtype)
    out = np.empty(a.shape, np.uint8)
    if a.ndim == 0 or a.size == 0:
        flat_a, flat_o, step = a.reshape(1, -1), out.reshape(1, -1), 1
    else:                                  # slices along the first axis (views: a non-contiguous input is not copied as a whole)
        flat_a, flat_o = a, out
        step = max(1, CONVERT_ROWS_BYTES // max(1, 4 * (a.size // a.shape[0])))
    for lo in range(0, flat_a.shape[0], step):
        part = np.ascontiguousarray(flat_a[lo:lo + step])
        with np.errstate(invalid='ignore'):
            k = np.rint(part * _F255)
            k = np.where((k >= 0) & (k <= 255), k, 0).astype(np.uint8)      # (NaN and out-of-range values: any byte, they fail the check below)
        bad = (k.astype(np.float32) / _F255).view(np.uint32) != part.view(np.uint32)
        if bad.any():
            i = np.unravel_index(int(np.argmax(bad)), part.shape)
            i = (i[0] + lo,) + tuple(i[1:]) if a.ndim else ()
            raise NotByteExact(i, a[i].item())
        flat_o[lo:lo + step] = k
    return out


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
    """x [N,H,W,3], y [N,h,w,K+1] as fp32 device tensors `.x`, `.y` on `device`; with image_dtype='uint8' `.x` is a uint8 tensor (x given as
    uint8 is uploaded as is, x given as float32 goes through to_u8_exact chunk by chunk: NotByteExact if it is not a byte image).

    x, y: numpy arrays, np.memmap or paths of .npy files (opened memory-mapped).  rows: optional row subset (the --debug
    selection), taken in the order given.  chunk_rows: rows per staging buffer (default: DEFAULT_CHUNK_BYTES worth of images).
    budget_bytes: the device memory the set may take; default: what torch.cuda.mem_get_info reports free, less reserve_bytes
    (room the engines have not claimed yet: workspace, the filter-spectra cache).
    cells: optional integers [N,K+1,2], the (row, col) heat-map cell of every channel's joint (data.joint_cells), indexed like x and y (`rows` selects from
    them too) -> `.cells`, int32 on the device, read by the affine augmentation (Engine.augment_affine_indexed).  Without it `.cells` is derived once at
    upload as the arg-max cell of each map (the first maximum): exact for a whole blob, but a blob cut by the border -- a joint clamped to row h or
    column w -- has lost its true centre, and only passing `cells` keeps it."""

    def __init__(self, x, y, device=0, rows=None, chunk_rows=None, budget_bytes=None, reserve_bytes=0, image_dtype='float32', cells=None):
        if image_dtype not in ('float32', 'uint8'):
            raise ValueError("image_dtype must be 'float32' or 'uint8', got %r" % (image_dtype,))
        self.image_dtype = image_dtype
        x, y = _open(x), _open(y)
        if x.ndim != 4 or y.ndim != 4 or x.shape[3] != 3 or x.shape[0] != y.shape[0]:
            raise ValueError('DeviceDataset expects x [N,H,W,3] and y [N,h,w,K+1] with the same N; got %s, %s' % (x.shape, y.shape))
        if rows is not None:
            rows = np.asarray(rows, np.int64).reshape(-1)
            if rows.size and (rows.min() < 0 or rows.max() >= x.shape[0]):
                raise IndexError('rows outside [0, %d)' % x.shape[0])
        if cells is not None:
            cells = np.asarray(cells)
            if cells.shape != (x.shape[0], y.shape[3], 2) or cells.dtype.kind not in 'iu':
                raise ValueError('cells must be integers [N,%d,2] = (row, col) per example of x and channel of y; got %s %s' % (y.shape[3], cells.shape, cells.dtype))
            if cells.size and (cells.min() < 0 or cells[..., 0].max() > y.shape[1] or cells[..., 1].max() > y.shape[2]):
                raise ValueError('cells outside [0, %d] x [0, %d] (data.joint_cells clamps to the image, so row h / column w are the last)' % (y.shape[1], y.shape[2]))
            cells = np.ascontiguousarray(cells if rows is None else cells[rows], np.int32)
        self.n = int(x.shape[0] if rows is None else rows.size)
        if self.n < 1:
            raise ValueError('DeviceDataset needs at least one example')
        self.device = torch.device('cuda', device if isinstance(device, int) else torch.device(device).index or 0)
        shape_x, shape_y = (self.n,) + tuple(x.shape[1:]), (self.n,) + tuple(y.shape[1:])
        xes = 1 if image_dtype == 'uint8' else 4                    # bytes per image value
        self.nbytes = xes * int(np.prod(shape_x)) + 4 * int(np.prod(shape_y))
        if budget_bytes is None:
            free, total = torch.cuda.mem_get_info(self.device)
            budget_bytes, where = free - int(reserve_bytes), '%d bytes free of %d on %s, %d of them reserved for the engines' % (free, total, self.device, reserve_bytes)
        else:
            where = 'the budget given'
        if self.nbytes > budget_bytes:
            raise DeviceDataTooLarge('the data set needs %d bytes (%d examples: x %s, y %s, %s) and may use %d (%s); a set that does not fit '
                                     'is not prefetched from the host: train without device data'
                                     % (self.nbytes, self.n, shape_x[1:], shape_y[1:], 'fp32' if xes == 4 else 'x uint8, y fp32', budget_bytes, where))
        with torch.cuda.device(self.device):
            self.x = torch.empty(shape_x, dtype=torch.uint8 if xes == 1 else torch.float32, device=self.device)
            self.y = torch.empty(shape_y, dtype=torch.float32, device=self.device)
            import time
            t0 = time.perf_counter()
            stream = torch.cuda.Stream(device=self.device)
            for src, dst in ((x, self.x), (y, self.y)):
                self._upload(src, dst, rows, chunk_rows, stream)
            stream.synchronize()         # one-off: afterwards the tensors are safe to read from any stream
            self.upload_seconds = time.perf_counter() - t0
            # .cells int32 [N,K+1,2]: the (row, col) heat-map cell of every channel's joint, which the affine augmentation transforms (8 bytes
            # per map, not counted in nbytes).  Given as `cells` (data.joint_cells) they are exact.  Derived, they are the arg-max cell of each map, the first
            # maximum as in jcm_argmax_coords -- which for a blob cut by the border (a centre on row h or column w) is a neighbour of the true centre.
            self.cells = torch.as_tensor(cells, device=self.device) if cells is not None else self._argmax_cells(self.y)

    @staticmethod
    def _argmax_cells(y, chunk_bytes=64 << 20):
        """int32 [N,C,2] = (row, col) of the first maximum of every map of y [N,h,w,C], in slices of chunk_bytes of y."""
        n, h, w, ch = y.shape
        out = torch.empty((n, ch, 2), dtype=torch.int32, device=y.device)
        pos = torch.arange(h * w, dtype=torch.int32, device=y.device).view(1, h * w, 1)
        step = max(1, chunk_bytes // (4 * h * w * ch))
        for lo in range(0, n, step):
            part = y[lo:lo + step].reshape(-1, h * w, ch)
            first = torch.where(part == part.amax(dim=1, keepdim=True), pos, h * w).amin(dim=1)      # [n', C]: the lowest index that holds the maximum
            out[lo:lo + step, :, 0] = torch.div(first, w, rounding_mode='floor')
            out[lo:lo + step, :, 1] = first % w
        return out

    @staticmethod
    def _upload(src, dst, rows, chunk_rows, stream):
        n = dst.shape[0]
        row_elems = int(np.prod(dst.shape[1:]))
        if chunk_rows is None:      # sized by the SOURCE: a float chunk that is converted to bytes is as large on the host as one that is uploaded as floats
            chunk_rows = max(1, DEFAULT_CHUNK_BYTES // (max(dst.element_size(), np.dtype(src.dtype).itemsize) * row_elems))
        chunk_rows = min(int(chunk_rows), n)
        flat = dst.view(n, row_elems)
        stage = [torch.empty((chunk_rows, row_elems), dtype=dst.dtype).pin_memory() for _ in range(2)]
        done = [None, None]
        for i, (lo, hi) in enumerate(plan_chunks(n, chunk_rows)):
            k = i % 2
            if done[k] is not None:
                done[k].synchronize()        # the copy that last read this buffer; the other buffer's copy runs meanwhile
            part = src[lo:hi] if rows is None else src[rows[lo:hi]]
            part = np.asarray(part).reshape(hi - lo, row_elems)
            if dst.dtype == torch.uint8:                   # a byte data set: bytes pass, floats are converted and the round trip checked
                try:
                    part = to_u8_exact(part)       # uint8 passes, float32 is converted with proof, anything else (float64, ...) is a TypeError
                except NotByteExact as e:                  # the index in the caller's array: row of the upload order, then the position in the image
                    r, c = e.index
                    raise NotByteExact((lo + r,) + tuple(int(v) for v in np.unravel_index(c, dst.shape[1:])), e.value) from None
            np.copyto(stage[k][:hi - lo].numpy(), part, casting='same_kind')
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

    def rerender_people(self, engine, poses, indices, seed, batch=64, **ranges):
        """A byte set of rendered people (render_people) drawn again in place: example i becomes a new scene of the pose
        poses[indices[i]] -- new draws from RandomState(seed), the same poses -- written by Engine.synth_people straight into `.x`; `.y` and `.cells`
        are replaced with the new scenes' targets and cells.  Everything -- the launches and the copies into `.y` and `.cells` -- is enqueued batch by batch
        on the ENGINE's stream, behind whatever that stream still reads of the set (a gather in flight); the host does not wait.  Work on another
        stream that reads the set has to wait for the engine's stream, as for every call of the engine."""
        indices = np.asarray(indices).reshape(-1)
        if self.image_dtype != 'uint8':
            raise ValueError('rerender_people draws bytes: the set must be held with image_dtype=\'uint8\'')
        if indices.shape[0] != self.n:
            raise ValueError('rerender_people: %d indices for a set of %d examples' % (indices.shape[0], self.n))
        if engine.device != self.device:
            raise ValueError('the data set is on %s, the engine on %s' % (self.device, engine.device))
        engine._on_stream(self.x, self.y, self.cells)      # (the engine's stream waits for the current one, as in every call of the engine)
        for lo, _x, y, cells in _people_batches(engine, poses, indices, seed, batch, ranges, into=self.x):
            with torch.cuda.stream(engine._stream):
                self.y[lo:lo + y.shape[0]].copy_(torch.as_tensor(y))
                self.cells[lo:lo + y.shape[0]].copy_(torch.as_tensor(np.ascontiguousarray(cells, np.int32)))
        return self


def _people_batches(engine, poses, indices, seed, batch, ranges, into=None, dtype=torch.uint8):
    """The scenes of poses[indices] from RandomState(seed), `batch` at a time in index order: yields (lo, x device [n,H,W,3], y host, cells host).
    into: a device tensor [N,H,W,3] whose rows [lo, lo + n) receive the images (its height and width are the scenes'); otherwise 480x720."""
    from . import synth
    indices = np.asarray(indices).reshape(-1)
    rng = np.random.RandomState(seed)
    H, W = (int(into.shape[1]), int(into.shape[2])) if into is not None else (480, 720)
    for lo in range(0, indices.shape[0], int(batch)):
        recs, prims, _xy, cells, y = synth.people_batch(rng, poses, indices[lo:lo + int(batch)], H, W, **ranges)
        x = engine.synth_people(recs, prims, H, W, out=None if into is None else into[lo:lo + recs.shape[0]], dtype=dtype)
        yield lo, x, y, cells


def render_people(engine, poses, indices, seed, image_dtype='uint8', batch=64, **ranges):
    """A data set of rendered people: one scene per entry of `indices` into poses [N,2,9] (data.py's xy), drawn from
    RandomState(seed) by synth.people_batch, rendered `batch` at a time on the engine's device and downloaded -> (x [n,480,720,3] uint8, or float32
    = byte / 255 with image_dtype='float32'; y float32 [n,60,90,10]; cells int64 [n,10,2]): host arrays of the shapes and dtypes get_dataset returns,
    and the cells DeviceDataset(cells=...) and the affine augmentation take."""
    if image_dtype not in ('float32', 'uint8'):
        raise ValueError("image_dtype must be 'float32' or 'uint8', got %r" % (image_dtype,))
    indices = np.asarray(indices).reshape(-1)
    n = indices.shape[0]
    if n < 1:
        raise ValueError('render_people needs at least one index')
    x = np.empty((n, 480, 720, 3), np.uint8 if image_dtype == 'uint8' else np.float32)
    ys, cs = [], []
    for lo, xb, y, cells in _people_batches(engine, poses, indices, seed, batch, ranges, dtype=torch.uint8 if image_dtype == 'uint8' else torch.float32):
        x[lo:lo + y.shape[0]] = xb.cpu().numpy()
        ys.append(y)
        cs.append(cells)
    return x, np.concatenate(ys), np.concatenate(cs)


def render_clip(engine, rng, pose_a, pose_b, T, other_xy=None, H=480, W=720, cuts=(), image_dtype='uint8', **ranges):
    """A clip of rendered people: the T frames synth.people_clip(rng, pose_a, pose_b, T, other_xy, H, W, cuts, **ranges) lists,
    drawn by ONE Engine.synth_people call -> (x device [T,H,W,3], uint8 or float32 = byte / 255; records int32 [T,20]; prims int32 [NP,16]; xy
    float64 [T,2,9], the annotated person's joints (x, y) of every frame).  No kernel of its own: a clip is a batch whose scenes share everything
    but one person's joints -- the sensor noise too, whose seed is the record's."""
    from . import synth
    if image_dtype not in ('float32', 'uint8'):
        raise ValueError("image_dtype must be 'float32' or 'uint8', got %r" % (image_dtype,))
    records, prims, xy = synth.people_clip(rng, pose_a, pose_b, T, other_xy, H, W, cuts, **ranges)
    x = engine.synth_people(records, prims, H, W, dtype=torch.uint8 if image_dtype == 'uint8' else torch.float32)
    return x, records, prims, xy


def pan_origins(pan, margin, T, H=480, W=720):
    """Where the crops of a panned clip lie on its canvas of (H + 2 my) x (W + 2 mx), margin = (my, mx): pan int [T,2] = (dy, dx) per frame ->
    int64 [T,2], (oy_t, ox_t) = (my, mx) + pan_0 + .. + pan_t.  A crop that would leave the canvas raises ValueError.  Host integers only."""
    pan = np.asarray(pan)
    my, mx = int(margin[0]), int(margin[1])
    if pan.dtype.kind not in 'iu' or pan.shape != (int(T), 2) or my < 0 or mx < 0:
        raise ValueError('pan must be an integer array [T,2] = (%d, 2) and margin two non-negative ints, got %s %s and %r' % (int(T), pan.dtype, pan.shape, margin))
    o = np.array([my, mx], np.int64)[None, :] + np.cumsum(pan.astype(np.int64), axis=0)
    bad = (o < 0).any(axis=1) | (o[:, 0] > 2 * my) | (o[:, 1] > 2 * mx)
    if bad.any():
        t = int(np.argmax(bad))
        raise ValueError('crop %d at (%d, %d) leaves the canvas: origins lie in [0, %d] x [0, %d]' % (t, o[t, 0], o[t, 1], 2 * my, 2 * mx))
    return o


def crop_pan(canvas, xy, origins, H=480, W=720):
    """canvas [T,Hc,Wc,3] (a tensor or an array), xy float [T,2,9] = (x, y) on the canvas, origins int [T,2] -> (the crops canvas_t[oy_t : oy_t + H,
    ox_t : ox_t + W] stacked as [T,H,W,3], xy moved into each crop, inside bool [T,9]: is the joint within the crop?).  Plain slicing."""
    o = np.asarray(origins, np.int64)
    crops = [canvas[t, int(o[t, 0]):int(o[t, 0]) + H, int(o[t, 1]):int(o[t, 1]) + W] for t in range(o.shape[0])]
    x = torch.stack(crops).contiguous() if isinstance(canvas, torch.Tensor) else np.ascontiguousarray(np.stack(crops))
    moved = np.asarray(xy, np.float64) - o[:, ::-1, None].astype(np.float64)
    inside = (moved[:, 0] >= 0) & (moved[:, 0] <= W - 1) & (moved[:, 1] >= 0) & (moved[:, 1] <= H - 1)
    return x, moved, inside


def render_clip_pan(engine, rng, pose_a, pose_b, T, pan, margin, other_xy=None, cuts=(), image_dtype='uint8', **ranges):
    """A clip of rendered people seen by a camera that pans: synth.people_clip draws the T frames of one scene on a canvas of
    (480 + 2 my) x (720 + 2 mx), margin = (my, mx), in ONE Engine.synth_people call, and frame t is the crop canvas_t[oy_t : oy_t + 480, ox_t :
    ox_t + 720] with (oy_t, ox_t) = (my, mx) + pan_0 + .. + pan_t, pan int [T,2] (pan_origins; a crop that would leave the canvas raises
    ValueError).  Returns (x device [T,480,720,3]; xy float64 [T,2,9], the annotated person's joints (x, y) in every crop; inside bool [T,9], is
    the joint within its crop; disp int64 [T,2], the true displacement of frame t against frame t-1 with the sign of Engine.frame_shift -- the
    content at (y, x) of frame t is at (y, x) + disp_t of frame t-1 --, which is pan_t, and (0, 0) for frame 0, which has no frame before it).
    Cropping is tensor slicing: the renderer and its records are unchanged.  A property of these clips: the sensor noise belongs to the canvas
    (its seed is the record's and its pattern is a function of the canvas pixel), so it pans with the crop like the scene does -- a real
    sensor's noise stays with the sensor.  The estimate therefore sees frames that match exactly at the true displacement."""
    from . import synth
    if image_dtype not in ('float32', 'uint8'):
        raise ValueError("image_dtype must be 'float32' or 'uint8', got %r" % (image_dtype,))
    origins = pan_origins(pan, margin, T)
    Hc, Wc = 480 + 2 * int(margin[0]), 720 + 2 * int(margin[1])
    records, prims, xy = synth.people_clip(rng, pose_a, pose_b, T, other_xy, Hc, Wc, cuts, **ranges)
    canvas = engine.synth_people(records, prims, Hc, Wc, dtype=torch.uint8 if image_dtype == 'uint8' else torch.float32)
    with torch.cuda.stream(engine._stream):
        x, moved, inside = crop_pan(canvas, xy, origins)
    disp = np.asarray(pan, np.int64).copy()
    disp[0] = 0
    return x, moved, inside, disp
