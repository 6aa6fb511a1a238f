"""Mirror of the reference's evaluation.py -- the detection-rate metric of MODEC (evaluation.py:4-37) -- and of the
batch loop that calls it, eval_error (main.py:275-283).

The arg-max over the heat maps is libjcm's kernel (first occurrence); the remaining arithmetic of det_rate is a
handful of [B,2,K] operations done with torch on the device.

DetCurve / eval_curves are the detection-rate CURVES the reference's report shows (one per joint, radii 1..20 % of the torso length): the
same metric for every joint and every radius, counted by one kernel launch per batch (Engine.det_curve)."""
import numpy as np
import torch


def det_rate_from_coords(pred, true, normalized_radius=10, joints='all'):
    """evaluation.py:26-37 on arg-max coordinates [B,2,K] (row, col)."""
    lhip_idx, rsho_idx = 0, 7                                        # evaluation.py:26
    pred, true = pred.to(torch.float32), true.to(torch.float32)
    torso = torch.linalg.norm(true[:, :, lhip_idx] - true[:, :, rsho_idx], dim=1, keepdim=True)     # [B,1]
    nd = torch.linalg.norm(pred - true, dim=1) * 100 / torso                                        # [B,K]
    if joints != 'all':
        nd = nd[:, list(joints)]
    return 100 * (nd <= normalized_radius).to(torch.float32).mean()


def det_rate(heat_map_pred, heat_map_target, normalized_radius=10, joints='all', engine=None):
    """evaluation.py:4-37.  heat_map_* [n_images, height, width, n_joints] torch CUDA fp32.
    Percentage of (image, joint) pairs whose predicted arg-max lies within `normalized_radius` % of the
    torso length (distance between channels 0 and 7 of the target, evaluation.py:26,29) of the target's."""
    if engine is None:
        from . import main as M
        engine = M.engine()
    pred = engine.argmax_coords(heat_map_pred)                       # [B,2,K]
    true = engine.argmax_coords(heat_map_target.contiguous())
    return float(det_rate_from_coords(pred, true, normalized_radius, joints))


def peaks_to_pixels(peaks, stride=8):
    """The dict of Engine.hm_peaks (device tensors or host arrays: 'cells' [N,K,P,2], 'offsets' [N,K,P,2], 'scores' [N,K,P]; 'offsets' may be
    absent) -> host fp32 [N,K,P,3] = ((row + d_row) * stride, (col + d_col) * stride, score): image pixels by the reference's `coords * 8`
    (test.py), refined by the sub-cell offsets.  Filler slots (cells -1) give (-1, -1, 0)."""
    host = lambda a: a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    cells = host(peaks['cells'])
    scores = host(peaks['scores']).astype(np.float32)
    offsets = host(peaks['offsets']).astype(np.float32) if peaks.get('offsets') is not None else np.zeros(cells.shape, np.float32)
    if cells.ndim != 4 or cells.shape[3] != 2 or offsets.shape != cells.shape or scores.shape != cells.shape[:3]:
        raise ValueError('peaks_to_pixels expects cells / offsets [N,K,P,2] and scores [N,K,P]; got %s, %s, %s' % (cells.shape, offsets.shape, scores.shape))
    out = np.empty(cells.shape[:3] + (3,), np.float32)
    out[..., :2] = (cells.astype(np.float32) + offsets) * np.float32(stride)
    out[..., 2] = scores
    filler = cells[..., 0] < 0
    out[filler] = np.array([-1, -1, 0], np.float32)
    return out


def pose_to_pixels(pose, peaks, stride=8):
    """The dict of Engine.pose_decode ('index' [N,K], 'coords' [N,2,K], 'score' [N]) and the dict of Engine.hm_peaks it chose from ('offsets'
    [N,K,P,2]; may be absent), device tensors or host arrays -> host fp32 [N,K,3] = ((row + d_row) * stride, (col + d_col) * stride, score):
    the chosen cell in image pixels as peaks_to_pixels gives it, refined by the chosen peak's sub-cell offset, and the score of the pose.
    An image without a pose (index -1) gives (-1, -1, -inf)."""
    host = lambda a: a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    index, coords, score = host(pose['index']), host(pose['coords']), host(pose['score']).astype(np.float32)
    if index.ndim != 2 or coords.shape != (index.shape[0], 2, index.shape[1]) or score.shape != index.shape[:1]:
        raise ValueError('pose_to_pixels expects index [N,K], coords [N,2,K] and score [N]; got %s, %s, %s' % (index.shape, coords.shape, score.shape))
    pick = np.maximum(index, 0).astype(np.int64)
    if peaks.get('offsets') is not None:
        offsets = np.take_along_axis(host(peaks['offsets']).astype(np.float32), pick[:, :, None, None], axis=2)[:, :, 0, :]      # [N,K,2]
    else:
        offsets = np.zeros(index.shape + (2,), np.float32)
    out = np.empty(index.shape + (3,), np.float32)
    out[..., :2] = (coords.transpose(0, 2, 1).astype(np.float32) + offsets) * np.float32(stride)
    out[..., 2] = score[:, None]
    out[index < 0] = np.array([-1, -1, -np.inf], np.float32)
    return out


def fit_to_source(points, geom):
    """Points of the fitted frame back into their source images.  points: host array [N,...,2+] = (row, col, ...) in pixels of
    the frame Engine.fit_images made, as peaks_to_pixels / pose_to_pixels and `coords * 8` give them; geom: the [N,6] (or [N,4] + sizes) int
    array fit_images returned, (y0, x0, ch, cw, h, w) per image.  Returns (the same array as float64 with
        row_s = (row - y0 + 0.5) * h / ch - 0.5,   col_s = (col - x0 + 0.5) * w / cw - 0.5
    -- the inverse of the fit's pixel-centre mapping; trailing entries (scores) pass through, filler rows (row, col < 0) stay as they are -- and
    `inside`, bool [N,...]: whether the fitted point lay in the content rectangle [y0, y0 + ch) x [x0, x0 + cw); filler rows are outside)."""
    pts = np.array(points, dtype=np.float64)
    geom = np.asarray(geom)
    if pts.ndim < 2 or pts.shape[-1] < 2 or geom.ndim != 2 or geom.shape != (pts.shape[0], 6):
        raise ValueError('fit_to_source expects points [N,...,2+] and geom [N,6]; got %s, %s' % (pts.shape, geom.shape))
    g = geom.astype(np.float64).reshape((geom.shape[0],) + (1,) * (pts.ndim - 2) + (6,))
    row, col = pts[..., 0], pts[..., 1]
    filler = (row < 0) & (col < 0)
    inside = ~filler & (row >= g[..., 0]) & (row < g[..., 0] + g[..., 2]) & (col >= g[..., 1]) & (col < g[..., 1] + g[..., 3])
    out = pts.copy()
    out[..., 0] = np.where(filler, row, (row - g[..., 0] + 0.5) * g[..., 4] / g[..., 2] - 0.5)
    out[..., 1] = np.where(filler, col, (col - g[..., 1] + 0.5) * g[..., 5] / g[..., 3] - 0.5)
    return out, inside


def fit_geometry(h, w, OH, OW):
    """(y0, x0, ch, cw): the content rectangle of an h x w source in an OH x OW frame, the integer arithmetic include/jcm.h states for
    jcm_fit_images (and, on a window's size, jcm_fit_windows)."""
    h, w, OH, OW = int(h), int(w), int(OH), int(OW)
    if OH * w <= OW * h:
        ch, cw = OH, max(1, (2 * w * OH + h) // (2 * h))
    else:
        cw, ch = OW, max(1, (2 * h * OW + w) // (2 * w))
    return (OH - ch) // 2, (OW - cw) // 2, ch, cw


def window_to_source(points, geom, windows, sizes):
    """Points of fitted windows back into the images the windows were cut from.  points [N,...,2+] and geom [N,6] as for
    fit_to_source, geom being what Engine.fit_windows returned -- (y0, x0, ch, cw, wh, ww), the WINDOW's size --; windows: the int [N,5] =
    (image index, wy0, wx0, wh, ww) that call was given; sizes: int [n_images,2] = (h, w) of the images the windows index.  Returns
    fit_to_source(points, geom) with (wy0, wx0) added to the row and column entries, and `inside`: fit_to_source's (the fitted point lay in the
    content rectangle) and the mapped point lies in [-0.5, h - 0.5) x [-0.5, w - 0.5) of its image -- not in the part of the window that the
    image does not cover.  Filler rows pass through as in fit_to_source."""
    windows, sizes = np.asarray(windows), np.asarray(sizes)
    if windows.ndim != 2 or windows.shape[1] != 5 or sizes.ndim != 2 or sizes.shape[1] != 2:
        raise ValueError('window_to_source expects windows [N,5] and sizes [n_images,2]; got %s, %s' % (windows.shape, sizes.shape))
    out, inside = fit_to_source(points, geom)
    if windows.shape[0] != out.shape[0] or windows[:, 0].min() < 0 or windows[:, 0].max() >= sizes.shape[0]:
        raise ValueError('window_to_source: %d windows naming images %d..%d for %d points and %d sizes' %
                         (windows.shape[0], windows[:, 0].min(), windows[:, 0].max(), out.shape[0], sizes.shape[0]))
    lead = (windows.shape[0],) + (1,) * (out.ndim - 2)
    hw = sizes[windows[:, 0]].astype(np.float64)
    pts = np.asarray(points, dtype=np.float64)
    filler = (pts[..., 0] < 0) & (pts[..., 1] < 0)      # fit_to_source left these rows as they were
    row = out[..., 0] + windows[:, 1].astype(np.float64).reshape(lead)
    col = out[..., 1] + windows[:, 2].astype(np.float64).reshape(lead)
    inside = inside & (row >= -0.5) & (row < hw[:, 0].reshape(lead) - 0.5) & (col >= -0.5) & (col < hw[:, 1].reshape(lead) - 0.5)
    out[..., 0] = np.where(filler, out[..., 0], row)
    out[..., 1] = np.where(filler, out[..., 1], col)
    return out, inside


def get_next_batch(X, Y, batch_size, shuffle=False, rng=None):
    """main.py:184-192: whole batches only -- the remainder len(X) % batch_size is dropped; `shuffle` draws a permutation."""
    import numpy as np
    n_batches = len(X) // batch_size
    idx = (rng or np.random).permutation(len(X))[:n_batches * batch_size] if shuffle else np.arange(len(X))[:n_batches * batch_size]
    for batch_idx in idx.reshape([n_batches, batch_size]):
        yield X[batch_idx], Y[batch_idx]


class DetCurve:
    """Accumulator of detection-rate curves: counts[k, r] = number of images seen whose joint k lies within radii[r] % of the torso length
    of its target (evaluation.py:26-36, the comparison before the mean).  update() adds a batch on the device without synchronising;
    counts() / rates() read the [K,R] table back.  `engine` may be None for an accumulator that only merges or reports counts."""

    def __init__(self, engine, radii=range(1, 21), n_joints=None):
        self.engine = engine
        self.radii = np.asarray(list(radii), dtype=np.float32)
        if n_joints is None and engine is None:
            raise ValueError('DetCurve without an engine needs n_joints')
        self.n_joints = int(engine.n_joints if n_joints is None else n_joints)
        self.n_images = 0
        self._hits = None                                                 # device int32 [K,R], made by the first update
        self._extra = np.zeros((self.n_joints, len(self.radii)), np.int64)   # counts merged in from other accumulators

    def update(self, pred_coords, y):
        """pred_coords int32 [B,2,K] on the engine's device, y [B,H,W,C >= K] the targets of the same images."""
        if pred_coords.shape[2] != self.n_joints:
            raise ValueError('pred_coords has %d joints, this curve %d' % (pred_coords.shape[2], self.n_joints))
        self._hits = self.engine.det_curve(pred_coords, y, self.radii, hits=self._hits)['hits']
        self.n_images += int(pred_coords.shape[0])
        return self

    def counts(self):
        own = self._hits.cpu().numpy().astype(np.int64) if self._hits is not None else 0
        return self._extra + own

    def rates(self):
        """Detection rates in percent [K,R]."""
        if self.n_images == 0:
            raise ValueError('DetCurve has seen no image')
        return 100.0 * self.counts() / self.n_images

    def merge(self, other):
        """Add another accumulator's counts (a tower on another device, another shard of the set)."""
        if self.n_joints != other.n_joints or not np.array_equal(self.radii, other.radii):
            raise ValueError('merge needs the same joints and radii')
        self._extra = self._extra + other.counts()
        self.n_images += other.n_images
        return self

    def rate(self, joint, radius):
        r = np.flatnonzero(self.radii == np.float32(radius))
        if r.size == 0:
            raise KeyError('radius %r is not one of %s' % (radius, self.radii.tolist()))
        return float(self.rates()[joint, r[0]])

    def as_dict(self, joint_names):
        names = [str(n) for n in list(joint_names)[:self.n_joints]]
        if len(names) != self.n_joints:
            raise ValueError('%d joint names for %d joints' % (len(names), self.n_joints))
        rates = self.rates()
        d = {'radii': [float(r) for r in self.radii], 'n_images': int(self.n_images)}
        for k, n in enumerate(names):
            d[n] = [float(v) for v in rates[k]]
        return d


def _to_device_batch(bx, by, engine):
    bx = torch.as_tensor(bx)
    # byte images (a uint8 DeviceDataset, --u8_images) go to the byte entry as they are; everything else is widened to fp32
    x = bx.to(device=engine.device, dtype=torch.uint8 if bx.dtype == torch.uint8 else torch.float32).contiguous()
    y = torch.as_tensor(by, dtype=torch.float32, device=engine.device).contiguous()
    return x, y


def eval_curves(X, Y, engine, batch_size, use_sm=True, radii=range(1, 21), flip_test=False):
    """Detection-rate curves of a whole set: every image goes through engine.forward once (the last batch may be partial -- unlike
    eval_error, nothing is dropped) and its coordinates into two accumulators.  X [N,480,720,3] float or uint8, Y [N,60,90,K+1], numpy or
    torch, host or device.  Returns (DetCurve of the part detector, DetCurve of the spatial model); without use_sm the second counts the part
    detector's coordinates too (main.py:535).  flip_test=True: the coordinates of the mirrored test-time evaluation (Engine.forward(flip_test=True))
    are judged, against the same targets."""
    K = engine.n_joints
    pd, sm = DetCurve(engine, radii), DetCurve(engine, radii)
    for lo in range(0, len(X), batch_size):
        x, y = _to_device_batch(X[lo:lo + batch_size], Y[lo:lo + batch_size], engine)
        r = engine.forward(x, y[..., K:].contiguous() if use_sm else None, use_sm=use_sm, want_prob=False, flip_test=flip_test)
        pd.update(r['pd_coords'], y)
        sm.update(r['sm_coords'] if use_sm else r['pd_coords'], y)
    return pd, sm


def eval_curves_affine(X, cells, engine, batch_size, scales, angle=0.0, pad=0.0, use_sm=True, radii=range(1, 21), antialias=True):
    """Detection-rate curves of a set shown to the tower at other scales: for every scale, every batch (the last may be partial) is
    drawn through ONE fixed geometry -- augmentation.fixed_affine(scale, angle) about the centre, `pad` outside, the antialiased sample unless
    antialias=False -- by Engine.augment_affine, which also redraws the targets at the moved cells; the transformed batch goes through
    engine.forward with the redrawn tenth channel as the torso, and the coordinates are judged against the redrawn targets.
    X [N,H,W,3] float or uint8 (bytes are widened to the floats they stand for), cells [N,10,2] int (data.joint_cells, Engine.joint_cells(Y)); numpy or
    torch, host or device.  An image any of whose ten points leaves the frame under the forward map (augmentation.affine_joints_inside, decided on the
    host in float64) has a clamped target and is left out of that scale's counts: DetCurve.n_images of a scale is the number counted.
    Returns {scale: (DetCurve of the part detector, DetCurve of the spatial model)}; without use_sm the second counts the part detector's coordinates."""
    from .augmentation import affine_joints_inside, fixed_affine
    K = engine.n_joints
    host_cells = cells.cpu().numpy() if isinstance(cells, torch.Tensor) else np.asarray(cells)
    out = {}
    for scale in scales:
        pd, sm = DetCurve(engine, radii), DetCurve(engine, radii)
        for lo in range(0, len(X), batch_size):
            bx = torch.as_tensor(X[lo:lo + batch_size]).to(engine.device)
            x = (bx.to(torch.float32) / 255.0 if bx.dtype == torch.uint8 else bx.to(torch.float32)).contiguous()      # float32(k) / float32(255)
            c = torch.as_tensor(host_cells[lo:lo + batch_size].astype(np.int32), device=engine.device).contiguous()
            n, H, W, _ = x.shape
            draw = fixed_affine(n, H, W, scale, angle=angle, pad=pad, antialias=antialias)
            xa, ya = engine.augment_affine(x, c, draw.colour, draw.geom, draw.pad, width=draw.width)
            keep = affine_joints_inside(host_cells[lo:lo + batch_size], draw.geom, H, W)
            r = engine.forward(xa, ya[..., K:].contiguous() if use_sm else None, use_sm=use_sm, want_prob=False)
            if not keep.any():
                continue
            rows = torch.as_tensor(np.flatnonzero(keep), device=engine.device)
            with torch.cuda.stream(engine._stream):      # the coordinates and the targets were written on the engine's stream
                yk = ya.index_select(0, rows).contiguous()
                pk = r['pd_coords'].index_select(0, rows).contiguous()
                sk = r['sm_coords'].index_select(0, rows).contiguous() if use_sm else pk
            pd.update(pk, yk)
            sm.update(sk, yk)
        out[scale] = (pd, sm)
    return out


def eval_error(X_np, Y_np, engine, batch_size, use_sm=True, joints=(2,), det_radius=10, curves=None):
    """main.py:275-283: run a data set through the tower in inference mode batch by batch and return the means over
    batches of (loss_pd, loss_sm, det_rate_pd, det_rate_sm).  X_np [N,480,720,3] (float, or uint8 byte images), Y_np [N,60,90,10] (numpy or torch,
    host or device); the remainder N % batch_size is dropped as in the reference (get_next_batch).  Everything stays on
    the device until the four means are read back.  curves: an optional pair of DetCurve (part detector, spatial model) that is fed the
    coordinates of every batch on the way; the four numbers do not depend on it."""
    n_batches = len(X_np) // batch_size
    if n_batches == 0:
        raise ValueError('eval_error needs at least one whole batch (%d examples, batch size %d)' % (len(X_np), batch_size))
    K = engine.n_joints
    acc = torch.zeros(4, dtype=torch.float64, device=engine.device)
    for bx, by in get_next_batch(X_np, Y_np, batch_size):
        x, y = _to_device_batch(bx, by, engine)
        r = engine.eval_forward(x, y, use_sm=use_sm, want_prob=False)
        true = engine.argmax_coords(y[..., :K].contiguous())
        dr_pd = det_rate_from_coords(r['pd_coords'], true, det_radius, 'all' if joints == 'all' else list(joints))
        dr_sm = det_rate_from_coords(r['sm_coords'], true, det_radius, 'all' if joints == 'all' else list(joints)) if use_sm else dr_pd
        acc += torch.stack([r['losses'][0].double(), r['losses'][1].double(), dr_pd.double(), dr_sm.double()])
        if curves is not None:
            curves[0].update(r['pd_coords'], y)
            curves[1].update(r['sm_coords'] if use_sm else r['pd_coords'], y)
    return tuple(float(v) for v in (acc / n_batches).cpu())


def argmax_agreement(ref_prob, ref_coords, got_prob, got_coords, margin_mult=6.0, topk=32):
    """How far the arg-max coordinates of one arithmetic (`got_*`, e.g. a bf16 engine) are from another's (`ref_*`, the fp32 engine),
    evaluation.py:15-24 / main.py:389-397 being what the reference does with the heat maps.  prob [B,H,W,K] (softmax outputs), coords int32
    [B,2,K].  Returns, over all B*K joints and over the "safe" ones -- joints whose reference top-2 log-probability margin exceeds
    `margin_mult` x the measured rms log-probability error of `got` (taken on the reference's `topk` largest pixels per map, where
    the arg-max is decided) -- the exact-agreement rate, the rate within one heat-map cell (Chebyshev) and the mean Euclidean cell distance."""
    B, H, W, K = ref_prob.shape
    lr = torch.log(ref_prob.reshape(B, H * W, K).clamp_min(1e-37))
    lg = torch.log(got_prob.reshape(B, H * W, K).clamp_min(1e-37))
    top, idx = lr.topk(topk, dim=1)                                   # [B,topk,K]
    err = torch.gather(lg, 1, idx) - top
    rms = float(torch.sqrt((err.double() ** 2).mean()))
    margin = top[:, 0, :] - top[:, 1, :]                              # [B,K]
    safe = margin > margin_mult * rms
    d = (ref_coords.to(torch.int64) - got_coords.to(torch.int64))
    cheb = d.abs().amax(dim=1)                                        # [B,K]
    eucl = torch.sqrt((d.double() ** 2).sum(dim=1))

    def rates(mask):
        n = int(mask.sum())
        if n == 0:
            return {'n_joints': 0, 'exact': None, 'within1': None, 'mean_dist': None}
        return {'n_joints': n, 'exact': float((cheb[mask] == 0).double().mean()), 'within1': float((cheb[mask] <= 1).double().mean()),
                'mean_dist': float(eucl[mask].mean())}
    out = rates(torch.ones_like(safe))
    out.update({'rms_logprob_err': rms, 'max_logprob_err': float(err.abs().max()), 'margin_mult': margin_mult,
                'median_margin': float(margin.median()), 'safe': rates(safe)})
    return out
