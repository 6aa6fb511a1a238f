"""Frame sequences: predict_sequence takes the frames of a clip, all of one size, and adds to every frame's result a 'track': one
position per joint that is consistent over the clip, from Engine.seq_filter (causal) or Engine.seq_viterbi (the most probable track) on the
stacked heat maps.  SequenceTracker is the online form of the filter.  SEQ_SIGMA and SEQ_RHO (motion.py) are not fitted to anything; what tracking
buys has been measured on rendered clips only, not on real video.

Clips with several people: predict_sequence_people pulls up to four consistent torso tracks out of the frames' torso maps
(Engine.seq_tracks: successive passes of the temporal model, each with the earlier tracks' neighbourhoods excluded), runs the spatial model
once per (frame, track) with the blob at the track's cell and tracks every person's joints; PeopleTracker is its online form.  SEQ_EXCLUDE and
SEQ_TORSO_SIGMA are untuned placeholders too.

Smoothed marginals and the fit: predict_sequence(mode='marginal') takes every frame's position from the smoothed posterior
P(x_t | all frames) of Engine.seq_smooth, with its confidence; motion.seq_fit re-estimates sigma (per joint) and rho on a clip's own maps by EM,
without annotations, and predict_sequence(fit_iters=) runs any mode with the fitted values.

Zoomed clips: predict_sequence_zoom runs the zoom pass on every frame of a clip in windows that follow the person and share
one cell lattice (zoom_window_track), so that two frames' maps differ by a whole number of cells, and tracks the joints through them with
Engine.seq_filter / seq_viterbi(shift=), the scans with a per-frame shift of the belief plane.

The fixed-lag smoother: predict_sequence(mode='lag', lag=L) takes every frame's position from P(x_t | frames 0 .. t+L) of
Engine.seq_smooth_lag, and LagTracker is its online form: a frame's dict becomes final L frames after it was pushed.

Camera pans: predict_sequence(camera=True) and SequenceTracker(camera=True) estimate the camera's translation between consecutive
fitted frames on the device (Engine.frame_shift), turn it into whole-cell lattice shifts (motion.camera_shifts) and run the filter or Viterbi with
shift=, so that the motion kernel is centred on where the camera's motion takes a joint, not on where it was.

Local motion: predict_sequence(flow=N) estimates one displacement per heat-map cell between every frame and the N frames before
and after it (Engine.frame_flow), warps those frames' maps onto the frame and pools them with its own (Engine.hm_flow_pool); the chosen mode then
runs on the pooled maps, which are maps like any other.

Flow-centred scans: predict_sequence(flow_centre=True) and SequenceTracker(flow_centre=True) match every frame against the one before
it (Engine.frame_flow, the causal slot), round the displacement of every cell to whole cells (motion.flow_cell_shifts) and run the filter or Viterbi
with centre=, so that the motion kernel of a cell is centred on where that cell's own content was, not on the cell itself.

Clip pose decoding: predict_sequence(mode='viterbi', pose=P) also decodes ONE skeleton per frame over the whole clip -- the P^9 poses
of every frame's pose_decode, linked in time by the motion model between the candidates (motion.seq_pose_tau, Engine.seq_pose_viterbi) -- as
'track_pose'; there is no online form."""
import numpy as np
import torch

from ..evaluation import fit_to_source, window_to_source
from ..motion import (SEQ_CAMERA_SEARCH, SEQ_EXCLUDE, SEQ_FLOW_MAX, SEQ_FLOW_SEARCH, SEQ_KEYS, SEQ_MODES, SEQ_RHO, SEQ_SIGMA, SEQ_TORSO_SIGMA, camera_shifts,
                      flow_cell_shifts, flow_refs, flow_weights, seq_fit, seq_pose_tau)
from .images import FIT_SIDE_MAX, FRAME, STRIDE, ZOOM_TORSO_JOINTS, ZOOM_TORSO_PIXELS, DeviceTimer, _coords_to_points, _upload, predict_images, second_pass, zoom_entry


def torso_length(points):
    """images.torso_length as the package's surface has it bound when the call is made: what replaces predict.torso_length replaces it for the clips too."""
    from .. import predict
    return predict.torso_length(points)


def _first_pass(engine, frames, clip=None, **kw):
    """Pass 1 of a clip: the frames, of one size -- that of the earlier pushes of `clip`, a tracker --, through predict_images(keep_maps=True, **kw)."""
    if not isinstance(frames, (list, tuple)) or len(frames) == 0:
        raise ValueError('frames must be a non-empty list of uint8 [h,w,3] images of one size')
    shapes = {tuple(f.shape) for f in frames}
    if len(shapes) != 1:
        raise ValueError('the frames of a clip have one size (one letterbox geometry); got %s' % sorted(shapes))
    if clip is not None:
        clip.same_size(shapes.pop())
    return predict_images(engine, frames, keep_maps=True, **kw)


def _track_entries(seq, mode, to_source, extra=None):
    """The dict of one scan (Engine.seq_filter / seq_viterbi / seq_smooth) over T frames -> one 'track' dict per frame, by the mode's keys in SEQ_KEYS.
    to_source: cells as points [T,K,2] of the maps' frame -> (points, inside) in the frames' own pixels; extra: per frame, fields that follow 'inside'."""
    cells, *keys = SEQ_KEYS[mode]
    pts, inside = to_source(_coords_to_points(seq[cells]))
    host = {k: seq[k].cpu().numpy() for k in keys}
    return [dict({'mode': mode, 'points': pts[t], 'inside': inside[t]}, **(extra[t] if extra else {}), **{k: host[k][t] for k in keys}) for t in range(pts.shape[0])]


def _geom(results):
    return np.array([r['geom'] for r in results], np.int64)


def _stacked(results, key):
    return torch.stack([r['maps'][key] for r in results]).contiguous()


def _finish(results, keep_maps):
    for r in ([] if keep_maps else results):
        del r['maps']
    return results


def _seq_call(engine, mode, hm, sigma, rho, radius, lag=None, **kw):
    if mode == 'lag':      # one flushed call over the clip: no state comes back
        seq = engine.seq_smooth_lag(hm, sigma, rho, lag, radius=radius, flush=True)
        return {k: seq[k] for k in SEQ_KEYS[mode]}
    if mode == 'marginal':
        return engine.seq_smooth(hm, sigma, rho, radius=radius, want_smoothed=False)
    return (engine.seq_filter if mode == 'filter' else engine.seq_viterbi)(hm, sigma, rho, radius=radius, **kw)


SEQ_CAMERA_MODES = ('filter', 'viterbi')      # the scans that have a moving form


def _camera(engine, results, search, prev=None, carry=(0, 0), x=None):
    """The camera's motion over the frames of `results` (dicts of pass 1 with the fitted frames kept): one Engine.frame_shift call on the stacked
    frames (x, when the caller has stacked them already) with the clip's content rectangle, prev the last fitted frame of the push before (None at
    a clip's start), then motion.camera_shifts from `carry`.  Every dict gains 'camera'.  Returns (shift int32 [T,2], the last fitted frame, the
    new carry)."""
    x = _stacked(results, 'frame') if x is None else x
    cam = engine.frame_shift(x, _geom(results)[0, :4], search=search, prev=prev)
    disp, sad = cam['disp'].cpu().numpy(), cam['sad'].cpu().numpy()
    shift, carry = camera_shifts(disp, carry, STRIDE)
    for t, r in enumerate(results):
        r['camera'] = {'disp': (int(disp[t, 0]), int(disp[t, 1])), 'shift': (int(shift[t, 0]), int(shift[t, 1])), 'sad': (int(sad[t, 0]), int(sad[t, 1]))}
    return shift, x[-1].clone(), carry


def _check_camera_search(camera, camera_search):
    if not 1 <= int(camera_search) <= 16:
        raise ValueError('camera_search must be in 1..16, got %r' % (camera_search,))
    return bool(camera)


SEQ_FLOW_MODES = ('filter', 'viterbi', 'marginal')      # every offline mode: the pooling reads the frames after a frame as well as those before


def _check_flow(flow, flow_search, flow_weights_):
    """flow = 0 (off) or the neighbours on either side, 1..4 -> (N, D, the N + 1 pooling weights or None)."""
    if isinstance(flow, bool) or not isinstance(flow, (int, np.integer)) or not 0 <= int(flow) <= SEQ_FLOW_MAX:
        raise ValueError('flow must be 0 (off) or the neighbouring frames on either side, 1..4, got %r' % (flow,))
    N = int(flow)
    if not N:      # off: flow_search is the radius of flow = N >= 1 and is not looked at; weights given for no pooling are a mistake
        if flow_weights_ is not None:
            raise ValueError('flow_weights belongs to flow = N >= 1 (flow is %r)' % (flow,))
        return 0, None, None
    if not 1 <= int(flow_search) <= 16:
        raise ValueError('flow_search must be in 1..16, got %r' % (flow_search,))
    w = flow_weights(N) if flow_weights_ is None else np.asarray(flow_weights_, np.float64).reshape(-1)
    if w.size != N + 1 or not np.isfinite(w).all() or not w[0] > 0 or (w < 0).any():
        raise ValueError('flow_weights must be %d finite values, the first > 0 and the others >= 0 (flow=%d), got %r' % (N + 1, N, flow_weights_))
    return N, int(flow_search), w


def _flow_pool(engine, results, hm, x, N, search, weights, keep=None):
    """The maps of a clip pooled along its local motion: one Engine.frame_flow call on the stacked fitted frames x with
    motion.flow_refs and the clip's content rectangle, one Engine.hm_flow_pool on the stacked maps hm.  Every dict gains 'flow' -- the per-frame
    arg-max of the pooled maps through fit_to_source -- and its 'maps' 'pooled'.  Returns the pooled maps; keep, a list, receives the flow
    [T,2N,HH,WW,2] for a caller who has a second use for it."""
    T = hm.shape[0]
    flow = engine.frame_flow(x, _geom(results)[0, :4], flow_refs(T, N), search=search)['flow']
    if keep is not None:
        keep.append(flow)
    pooled = engine.hm_flow_pool(hm, flow, weights)
    pts, inside = fit_to_source(_coords_to_points(engine.argmax_coords(pooled)), _geom(results))
    for t, r in enumerate(results):
        r['flow'] = {'n': N, 'search': search, 'points': pts[t], 'inside': inside[t]}
        r['maps']['pooled'] = pooled[t]
    return pooled


SEQ_FLOW_CENTRE_MODES = ('filter', 'viterbi')      # the scans that have a centred form


def _check_flow_centre(flow_centre, flow_search, mode=None, camera=False, fit_iters=0):
    """flow_centre and what it cannot go with -> bool; flow_search is looked at only when it is on (flow = N checks its own use of it)."""
    if not flow_centre:
        return False
    if not 1 <= int(flow_search) <= 16:
        raise ValueError('flow_search must be in 1..16, got %r' % (flow_search,))
    if mode is not None and mode not in SEQ_FLOW_CENTRE_MODES:
        raise ValueError("flow_centre=True: mode must be 'filter' or 'viterbi', got %r (the smoother has no centred form)" % (mode,))
    if camera:
        raise ValueError('flow_centre=True cannot be combined with camera=True: the flow of a cell already contains the pan')
    if int(fit_iters) != 0:
        raise ValueError('flow_centre=True has no fit: fit_iters=%r needs the smoother, which has no centred form' % (fit_iters,))
    return True


def _flow_centre(engine, results, search, x=None, prev=None, flow=None):
    """The centre table of the frames of `results` (dicts of pass 1 with the fitted frames kept): every frame matched against the one
    before it -- slot `flow` [T,HH,WW,2] of a frame_flow call the caller has made already, or ONE Engine.frame_flow call here on the stacked frames x
    with a one-slot ref table and the clip's content rectangle; prev [H,W,3], the last fitted frame of the push before, is stacked in front and its
    row dropped again --, then motion.flow_cell_shifts.  Every dict gains 'flow_centre'.  Returns (centre int32 [T,HH,WW,2], the stacked frames or
    None when none were needed); row 0 is zero without prev."""
    if flow is None:
        x = _stacked(results, 'frame') if x is None else x
        lead = 0 if prev is None else 1
        if lead:
            x = torch.cat([prev.unsqueeze(0), x])
        n = int(x.shape[0])
        ref = np.arange(-1, n - 1, dtype=np.int32).reshape(n, 1)      # frame t against t-1; the first has none
        flow = engine.frame_flow(x, _geom(results)[0, :4], ref, search=search)['flow'][lead:, 0]
    centre = flow_cell_shifts(flow).contiguous()
    moved = (centre != 0).any(dim=3).sum(dim=(1, 2)).cpu().numpy()
    for t, r in enumerate(results):
        r['flow_centre'] = {'search': int(search), 'moved': int(moved[t])}
    return centre, x


def predict_sequence(engine, frames, mode='filter', sigma=SEQ_SIGMA, rho=SEQ_RHO, radius=None, use_sm=True, batch_size=16, people=1, zoom=False,
                     keep_maps=False, fit_iters=0, lag=None, camera=False, camera_search=SEQ_CAMERA_SEARCH, flow=0, flow_search=SEQ_FLOW_SEARCH,
                     flow_weights=None, flow_centre=False, pose=0, pose_weight=1.0, **kw):
    """The frames of ONE clip, in order: a list of uint8 [h,w,3] images of one size (any other size raises ValueError: a clip has one letterbox
    geometry).  predict_images(frames, keep_maps=True, **kw) runs over them; the 'sm' maps ('pd' without use_sm) are stacked on the device as
    [T,60,90,K] and go through ONE call of Engine.seq_filter (mode 'filter', causal), Engine.seq_viterbi (mode 'viterbi', the most probable
    track), Engine.seq_smooth (mode 'marginal', the arg-max of every frame's smoothed posterior P(x_t | all frames)) or
    Engine.seq_smooth_lag (mode 'lag' with lag = L >= 1, the marginal given frames 0 .. t+L only: what LagTracker reports online);
    evaluation.fit_to_source maps the cells back.  Returns predict_images' dicts, every key with the value it has there, plus
      'track': {'mode', 'points' float64 [K,2] (row, col) in the frame's own pixels, 'inside' bool [K], 'norm' or 'maxes' float64 [K], 'reset' or
                'breaks' int [K]}  (the library's Z / M and its flags, include/jcm.h); mode 'marginal': 'conf' float32 [K] (the posterior at the
                point), 'norm', 'reset' and 'cut' int [K]; mode 'lag': those and 'lag', the lag the frame got (below L at the clip's end).
    lag is required with mode 'lag' and refused with any other.
    fit_iters = ITERS > 0 first re-estimates sigma (per joint) and rho on the clip's own maps (seq_fit below, starting from sigma and rho) and runs
    the mode with the fitted values; frame 0's dict then carries 'seq_fit', seq_fit's return value for the clip.
    camera=True (modes 'filter' and 'viterbi' only -- 'marginal', 'lag' and fit_iters raise ValueError, the smoother has no moving
    form): the fitted frames are kept and stacked, ONE Engine.frame_shift call with the clip's content rectangle and search radius camera_search
    (1..16) estimates the camera's translation per frame, motion.camera_shifts turns it into whole-cell shifts and the scan runs with shift=.
    Every frame's dict gains 'camera': {'disp': (dy, dx) in fitted-frame pixels, 'shift': (sy, sx) in cells, 'sad': (best, zero), the sums of
    absolute luma differences at disp and at no displacement -- there is no cut detection, a caller judges by the two}.  Global translation
    only; camera_search = 8 is an untuned placeholder like sigma and rho.
    flow = N in 1..4 (modes 'filter', 'viterbi' and 'marginal', with fit_iters and with camera=True too -- the two are independent,
    and the frames are stacked once for both; mode 'lag' raises ValueError: two-sided pooling reads frames the lag has not yet seen): the fitted
    frames are kept and stacked, ONE Engine.frame_flow call with motion.flow_refs(T, N), the clip's content rectangle and search radius flow_search
    (1..16 pixels) gives one displacement per heat-map cell against the N frames before and after every frame, ONE Engine.hm_flow_pool warps those
    frames' maps onto the frame and pools them with its own under flow_weights (N + 1 values, default motion.flow_weights(N): uniform), and the
    fit and the mode run on the pooled maps.  Every frame's dict gains 'flow': {'n', 'search', 'points' float64 [K,2], 'inside' bool [K]: the
    frame's own arg-max of the pooled maps}, and 'maps' gains 'pooled'.  Block matching on luma, whole pixels, no occlusion reasoning, no gating
    of a neighbour by its match; flow_search = 8 and the uniform weights are untuned placeholders.  flow = 0 changes nothing.
    flow_centre=True (modes 'filter' and 'viterbi' only -- 'marginal', 'lag' and fit_iters raise ValueError, the smoother has no centred
    form; camera=True raises ValueError too, the flow of a cell already contains the pan): the fitted frames are kept and stacked, ONE
    Engine.frame_flow call matches every frame against the one before it with search radius flow_search, motion.flow_cell_shifts rounds every
    cell's displacement to whole cells and the scan runs with centre=: a cell's motion kernel is centred on where the cell's own content was.
    With flow = N as well there is no second matching call -- slot 0 of the pooling's own call IS the frame before -- and the scan runs with
    centre= on the pooled maps.  Every frame's dict gains 'flow_centre': {'search', 'moved': the cells of the frame with a non-zero shift}.
    Whole cells of a whole-pixel flow, no gating of a cell by its match; what it buys in detection rate has not been measured.  flow_centre=False
    changes nothing.
    pose = P in 1..4 (mode 'viterbi' with use_sm only; camera, flow, flow_centre, fit_iters and any other P raise ValueError): pass 1
    runs with peaks=P, decode=True and keeps its candidates on the device; ONE Engine.pose_decode(want_tables=True) call covers the clip, then
    motion.seq_pose_tau(cells, count, sigma, rho, radius, pose_weight) on the host and ONE Engine.seq_pose_viterbi call: the exact MAP over the
    sequence of poses, where 'track' follows every joint on its own.  'track' is what it is without pose; every frame's dict gains the keys of
    peaks=P, decode=True and 'track_pose': {'peaks': P, 'index' int [K] (the candidate per joint, -1 without a pose), 'points' float64 [K,2] and
    'inside' bool [K] (the candidate's cell with its sub-cell offset, through fit_to_source), 'score' (E_t of the pose), 'maxes', 'breaks' (the
    library's m_t and flag), 'changed': the joints whose candidate is not the one of the frame's own decode}.  pose_weight = 1.0 mixes two
    log-scores of different origin -- the spatial model's energy and the motion kernel -- and is an untuned placeholder; with 0 the clip decode is
    every frame's own.  What this buys in detection rate has not been measured.  pose = 0 changes nothing.
    'maps' is kept only with keep_maps.  sigma (a scalar or K values, heat-map cells per frame), rho and radius are those of Engine.seq_filter;
    the defaults SEQ_SIGMA and SEQ_RHO are untuned placeholders, and what the track buys with trained weights has not been measured.
    One person, one pass: people != 1 and zoom=True raise ValueError -- associating people across frames, and windows that move from frame to
    frame, are out of scope."""
    if mode not in SEQ_MODES:
        raise ValueError("mode must be 'filter', 'viterbi', 'marginal' or 'lag', got %r" % (mode,))
    if (mode == 'lag') != (lag is not None):
        raise ValueError("lag=%r: mode 'lag' needs lag = L >= 1, and lag belongs to mode 'lag' alone (mode is %r)" % (lag, mode))
    if lag is not None and int(lag) < 1:
        raise ValueError('lag must be >= 1, got %r (lag 0 is the causal filter: mode=\'filter\')' % (lag,))
    if not 0 <= int(fit_iters) <= 100:
        raise ValueError('fit_iters must be 0 (off) or the EM iterations 1..100, got %r' % (fit_iters,))
    if people != 1:
        raise ValueError('predict_sequence tracks one person: people=%r would need an association of people across frames, which is out of scope' % (people,))
    if zoom:
        raise ValueError('predict_sequence has no zoom pass: its windows would move from frame to frame, which is out of scope')
    if _check_camera_search(camera, camera_search):
        if mode not in SEQ_CAMERA_MODES:
            raise ValueError("camera=True: mode must be 'filter' or 'viterbi', got %r (the smoother has no moving form)" % (mode,))
        if int(fit_iters) != 0:
            raise ValueError('camera=True has no fit: fit_iters=%r needs the smoother, which has no moving form' % (fit_iters,))
        kw = dict(kw, keep_frames=True)
    centred = _check_flow_centre(flow_centre, flow_search, mode, camera, fit_iters)
    centre_search = int(flow_search) if centred else None
    n_flow, flow_search, flow_w = _check_flow(flow, flow_search, flow_weights)
    if n_flow:
        if mode not in SEQ_FLOW_MODES:
            raise ValueError("flow=%d: mode must be 'filter', 'viterbi' or 'marginal', got %r (two-sided pooling reads frames the lag has not yet seen)" % (n_flow, mode))
    if n_flow or centred:
        kw = dict(kw, keep_frames=True)
    n_pose = _check_pose(pose, pose_weight, mode, use_sm, camera, n_flow, centred, fit_iters)
    if n_pose:
        kw = dict(kw, peaks=n_pose, decode=True, keep_peaks=True)
    results = _first_pass(engine, frames, use_sm=use_sm, batch_size=batch_size, **kw)
    with torch.cuda.stream(engine._stream):
        hm = _stacked(results, 'sm' if use_sm else 'pd')
        x = _stacked(results, 'frame') if camera or n_flow or centred else None      # stacked once for all
        flows = []
        if n_flow:
            hm = _flow_pool(engine, results, hm, x, n_flow, flow_search, flow_w, keep=flows if centred else None)
        fit = seq_fit(engine, hm, sigma, rho, iters=int(fit_iters)) if int(fit_iters) else None
        if fit is not None:
            sigma, rho = fit['sigma'], fit['rho']
        moving = {'shift': _camera(engine, results, int(camera_search), x=x)[0]} if camera else {}
        if centred:      # with flow = N slot 0 of the pooling's call is the frame before: no second matching call
            moving = {'centre': _flow_centre(engine, results, centre_search, x=x, flow=flows[0][:, 0] if flows else None)[0]}
        seq = _seq_call(engine, mode, hm, sigma, rho, radius, lag=lag, **moving)
        geom = _geom(results)
        for r, track in zip(results, _track_entries(seq, mode, lambda pts: fit_to_source(pts, geom))):
            r['track'] = track
        if fit is not None:
            results[0]['seq_fit'] = fit
        if n_pose:
            _pose_track(engine, results, n_pose, sigma, rho, radius, float(pose_weight))
    return _finish(results, keep_maps)


def _check_pose(pose, pose_weight, mode, use_sm, camera, n_flow, centred, fit_iters):
    """pose = 0 (off) or the candidates per joint of the clip decode, 1..4, and what it cannot go with -> P."""
    if isinstance(pose, bool) or not isinstance(pose, (int, np.integer)) or not 0 <= int(pose) <= 4:
        raise ValueError('pose must be 0 (off) or the candidates per joint, 1..4, got %r' % (pose,))
    if not int(pose):
        return 0
    if not np.isfinite(float(pose_weight)) or float(pose_weight) < 0:
        raise ValueError('pose_weight must be finite and >= 0, got %r' % (pose_weight,))
    if mode != 'viterbi' or not use_sm:
        raise ValueError("pose=%d: the clip decode goes with mode='viterbi' and use_sm=True (mode is %r, use_sm %r)" % (pose, mode, bool(use_sm)))
    if camera or n_flow or centred or int(fit_iters):
        raise ValueError('pose=%d cannot be combined with camera, flow, flow_centre or fit_iters: the transition between candidates is the plain motion '
                         'kernel with the given sigma and rho' % (pose,))
    return int(pose)


def _pose_track(engine, results, P, sigma, rho, radius, weight):
    """The clip decode over the frames of `results` (dicts of pass 1 with keep_peaks): ONE Engine.pose_decode(want_tables=True) on the stacked
    part-detector maps and torso maps, motion.seq_pose_tau on the host, ONE Engine.seq_pose_viterbi.  Every dict gains 'track_pose'."""
    maps = [r['maps'] for r in results]
    hm10 = torch.cat([torch.stack([m['pd'] for m in maps]), torch.stack([m['torso'] for m in maps])], dim=3).contiguous()
    peaks = {f: torch.stack([m['pd_peaks'][f] for m in maps]).contiguous() for f in ('cells', 'count')}
    dec = engine.pose_decode(hm10, peaks, want_tables=True)
    cells, count = peaks['cells'].cpu().numpy(), peaks['count'].cpu().numpy()
    tau = seq_pose_tau(cells, count, sigma, rho, radius=radius, weight=weight, hw=hm10.shape[1] * hm10.shape[2])
    seq = {k: v.cpu().numpy() for k, v in engine.seq_pose_viterbi(dec['V'], dec['M'], peaks['count'], peaks['cells'], tau).items()}
    own = torch.stack([m['pose_index'] for m in maps]).cpu().numpy()
    index = seq['index']
    # the chosen candidates in fitted-frame pixels as pose_to_pixels gives them: cell plus sub-cell offset; pass 1 kept the offsets in 'pd_peaks'
    pk = np.stack([np.asarray(r['pd_peaks'], np.float64) for r in results])      # [T,K,P,3], already in source pixels
    pin = np.stack([np.asarray(r['pd_peaks_inside']) for r in results])
    pick = np.maximum(index, 0).astype(np.int64)[:, :, None]
    pts = np.take_along_axis(pk[..., :2], pick[..., None], axis=2)[:, :, 0, :]
    inside = np.take_along_axis(pin, pick, axis=2)[:, :, 0]
    none = index < 0
    pts[none] = -1.0
    inside = inside & ~none
    for t, r in enumerate(results):
        r['track_pose'] = {'peaks': P, 'index': index[t], 'points': pts[t], 'inside': inside[t], 'score': float(seq['frame_score'][t]),
                           'maxes': float(seq['maxes'][t]), 'breaks': int(seq['breaks'][t]), 'changed': int((index[t] != own[t]).sum())}
        for key in ('torso', 'pd_peaks', 'pose_index'):
            del r['maps'][key]


# ------------------------------------------------------------------ zoomed clips
ZOOM_MAP = (FRAME[0] // STRIDE, FRAME[1] // STRIDE)      # 60 x 90 cells: a window of 60 p x 90 p source pixels puts p x p of them into every cell
SEQ_ZOOM_MODES = ('filter', 'viterbi')


def zoom_window_track(points, inside, torso, geom, frame=FRAME):
    """Where the second pass of a CLIP looks; host arithmetic only, float64 and integers.  One row per frame: points float
    [T,K,2] and inside bool [T,K], the tracked pass-1 joints in the frame's pixels ('track' of predict_sequence); torso float [T,2], the torso
    track in the frame's pixels; geom int [6] or [T,6], the clip's one pass-1 fit (y0, x0, ch, cw, h, w).  All windows of the clip share ONE
    lattice of pitch p source pixels per heat-map cell, so that two windows differ by a whole number of cells:
      valid frame: the four torso joints are inside and torso_length >= 2 * STRIDE * h / ch (the skip rules of zoom_windows);
      tmed = the median of torso_length over the valid frames;  p = max(1, floor(tmed * STRIDE / ZOOM_TORSO_PIXELS + 0.5));
      wh = 60 p, ww = 90 p for every frame: exactly 3:2, so fit_geometry gives the whole 480 x 720 frame and a cell is exactly p x p pixels;
      wy0 = p * floor((cy - 30 p) / p + 0.5), wx0 = p * floor((cx - 45 p) / p + 0.5) with (cy, cx) the frame's torso point, clamped to the
        nearest multiple of p at which the window still holds a pixel of the frame: -59 p <= wy0 <= p * ((h - 1) // p), -89 p <= wx0 <=
        p * ((w - 1) // p) (Engine.fit_windows refuses a window that shares nothing with the image);
      shift[t] = ((wy0[t] - wy0[t-1]) / p, (wx0[t] - wx0[t-1]) / p), exact integers, shift[0] = (0, 0): cell (y, x) of frame t's maps is cell
        (y + sy, x + sx) of frame t-1's -- the convention of jcm_seq_filter_moving / jcm_seq_viterbi_moving;
      cells = the torso point taken forward through the window, floor((c - w0 + 0.5) / p - 0.5) // STRIDE clamped to the map, as zoom_windows
        computes it: where the torso blob of the second pass goes.
    Returns (windows int64 [T,5] = (frame, wy0, wx0, wh, ww), cells int32 [T,2], shift int32 [T,2], p, valid bool [T]).  Every frame gets a
    window, a valid one or not: the track needs the maps of all of them.  With no valid frame the clip is not zoomed: p = 0 and windows,
    cells and shift are zero.  90 p > FIT_SIDE_MAX raises ValueError.
    One pitch per clip is a stated limit: a person who walks towards the camera changes scale, and the clip's median decides the pitch."""
    pts, inside, torso = np.asarray(points, np.float64), np.asarray(inside, bool), np.asarray(torso, np.float64)
    T = pts.shape[0]
    geom = np.asarray(geom, np.int64)
    if geom.ndim == 1:
        geom = np.broadcast_to(geom, (T, 6)) if geom.shape == (6,) else geom
    if pts.ndim != 3 or T < 1 or pts.shape[2] != 2 or pts.shape[1] < 8 or inside.shape != pts.shape[:2] or torso.shape != (T, 2) or geom.shape != (T, 6):
        raise ValueError('zoom_window_track expects points [T,K >= 8,2], inside [T,K], torso [T,2] and geom [6] or [T,6]; got %s, %s, %s, %s' %
                         (pts.shape, inside.shape, torso.shape, geom.shape))
    if (geom != geom[0]).any():
        raise ValueError('zoom_window_track: the frames of a clip have one fit; got several')
    OH, OW = int(frame[0]), int(frame[1])
    MH, MW = OH // STRIDE, OW // STRIDE
    ch, h, w = int(geom[0, 2]), int(geom[0, 4]), int(geom[0, 5])
    t = torso_length(pts)
    torso_joints = [j for pair in ZOOM_TORSO_JOINTS for j in pair]
    valid = inside[:, torso_joints].all(axis=1) & ~(t < 2.0 * STRIDE * h / ch)
    windows = np.zeros((T, 5), np.int64)
    windows[:, 0] = np.arange(T)
    if not valid.any():
        return windows, np.zeros((T, 2), np.int32), np.zeros((T, 2), np.int32), 0, valid
    p = max(1, int(np.floor(np.median(t[valid]) * STRIDE / ZOOM_TORSO_PIXELS + 0.5)))
    wh, ww = MH * p, MW * p
    if ww > FIT_SIDE_MAX or wh > FIT_SIDE_MAX:
        raise ValueError('zoom_window_track: a torso of %.1f pixels gives windows of %d x %d pixels; the sides a fit takes end at %d' %
                         (float(np.median(t[valid])), wh, ww, FIT_SIDE_MAX))
    origin, cells = np.empty((T, 2), np.int64), np.empty((T, 2), np.int32)
    for axis, (half, cells_n, size, content) in enumerate(((MH // 2, MH, h, OH), (MW // 2, MW, w, OW))):
        o = p * np.floor((torso[:, axis] - half * p) / p + 0.5).astype(np.int64)
        o = np.clip(o, -(cells_n - 1) * p, p * ((size - 1) // p))
        origin[:, axis] = o
        at = np.floor((torso[:, axis] - o + 0.5) * content / (cells_n * p) - 0.5).astype(np.int64) // STRIDE      # the fit's content origin is 0
        cells[:, axis] = np.clip(at, 0, cells_n - 1)
    windows[:, 1:3] = origin
    windows[:, 3], windows[:, 4] = wh, ww
    shift = np.zeros((T, 2), np.int64)
    shift[1:] = (origin[1:] - origin[:-1]) // p
    return windows, cells, shift.astype(np.int32), p, valid


def predict_sequence_zoom(engine, frames, mode='viterbi', sigma=SEQ_SIGMA, torso_sigma=SEQ_TORSO_SIGMA, rho=SEQ_RHO, radius=None, batch_size=16, people=1,
                          keep_maps=False, fit_iters=0, pad=0, timing=None, camera=False, flow=0, flow_centre=False, **kw):
    """The frames of ONE clip with one person in it, tracked a second time at the scale the tower was trained on; frames as
    for predict_sequence.
      1. predict_sequence(frames, mode, ..., torso_prob=True): the first pass and its 'track'; the torso track comes from the frames'
         torso_prob maps with Engine.seq_tracks(people=1), as predict_sequence_people obtains its tracks;
      2. zoom_window_track: one window per frame around the torso track, all on one lattice of pitch p, and the whole-cell shift of every
         frame's lattice against the one before;
      3. Engine.fit_windows of every frame, a forward with the blob at the window's torso cell and want_prob=True, batch_size at a time; the
         'sm' maps stacked as [T,60,90,K]; Engine.seq_filter or Engine.seq_viterbi with shift=; evaluation.window_to_source maps every frame's
         cells back through that frame's window.
    Returns predict_sequence's dicts, every key with its value, plus
      'zoom': one entry as predict_images(zoom=True) writes it, the per-frame arg-max of the second pass; 'window' is the frame's window here;
      'track_zoom': {'mode', 'points' float64 [K,2] (row, col) in the frame's own pixels, 'inside' bool [K], 'window' (y0, x0, h, w), 'shift'
                     (sy, sx), 'pitch', and 'norm' / 'reset' or 'maxes' / 'breaks' [K] as in 'track'}.
    A clip with no valid frame (zoom_window_track) is not zoomed: every frame's 'zoom' entry has zoomed False and the pass-1 values, and there
    is no 'track_zoom'.  timing also receives 'zoom_fit_ms', 'zoom_forward_ms' and 'seq_zoom_pitch'.
    The modes are 'filter' and 'viterbi': mode='marginal' and fit_iters raise ValueError (jcm_seq_smooth has no moving form), people != 1 too.
    One pitch per clip is a stated limit; torso_sigma, sigma and rho are untuned placeholders, and what this buys with trained weights has not
    been measured.  camera=True raises ValueError: the windows already move with the person, and a camera estimate under them is out of scope;
    flow != 0 raises ValueError too: the windows move the lattice from frame to frame, and flow under moving windows is out of scope;
    flow_centre=True likewise (there is no centred form with a frame shift on top)."""
    if flow_centre:
        raise ValueError('predict_sequence_zoom has no flow-centred scan: its windows move the lattice from frame to frame (flow_centre=True belongs to predict_sequence)')
    if camera:
        raise ValueError('predict_sequence_zoom has no camera estimate: its windows follow the person already (camera=True belongs to predict_sequence)')
    if flow:
        raise ValueError('predict_sequence_zoom has no flow pooling: its windows move the lattice from frame to frame (flow=%r belongs to predict_sequence)' % (flow,))
    if mode not in SEQ_ZOOM_MODES:
        raise ValueError("mode must be 'filter' or 'viterbi', got %r (the smoother has no moving form: mode 'marginal' is not offered with zoomed clips)" % (mode,))
    if int(fit_iters) != 0:
        raise ValueError('predict_sequence_zoom has no fit: fit_iters=%r needs the smoother, which has no moving form' % (fit_iters,))
    if people != 1:
        raise ValueError('predict_sequence_zoom tracks one person: people=%r is out of scope' % (people,))
    B = int(batch_size)
    results = predict_sequence(engine, frames, mode=mode, sigma=sigma, rho=rho, radius=radius, use_sm=True, batch_size=B, keep_maps=True, torso_prob=True,
                               pad=pad, timing=timing, **kw)
    T, zoom_ms = len(results), [0.0, 0.0]
    with torch.cuda.stream(engine._stream):
        torso = engine.seq_tracks(_stacked(results, 'torso_prob'), 1, torso_sigma, rho, mode=mode)
        tc = torso[SEQ_KEYS[mode][0]].cpu().numpy().reshape(T, 2).astype(np.float64)
        geom1 = _geom(results)
        torso_px, _ = fit_to_source(tc * STRIDE, geom1)
        points, inside = np.stack([r['track']['points'] for r in results]), np.stack([r['track']['inside'] for r in results])
        wins, cells, shift, pitch, valid = zoom_window_track(points, inside, torso_px, geom1)
        lengths = torso_length(points)
        second, parts = None, []
        if pitch:
            for lo in range(0, T, B):
                local = wins[lo:lo + B].copy()
                local[:, 0] -= lo
                parts.append(second_pass(engine, [_upload(im, engine.device) for im in frames[lo:lo + B]], local, cells[lo:lo + B], B, pad, True, zoom_ms))
            second = {key: tuple(np.concatenate([p[0][key][i] for p in parts]) for i in range(2)) for key in ('pd', 'sm')}
            geom2, hm = np.concatenate([p[1] for p in parts]), torch.cat([p[2] for p in parts]).contiguous()
            seq = _seq_call(engine, mode, hm, sigma, rho, radius, shift=shift)
            sizes = np.array([r['size'] for r in results], np.int64)
            extra = [{'window': tuple(int(v) for v in wins[t, 1:]), 'shift': (int(shift[t, 0]), int(shift[t, 1])), 'pitch': int(pitch)} for t in range(T)]
            for r, track, maps in zip(results, _track_entries(seq, mode, lambda pts: window_to_source(pts, geom2, wins, sizes), extra), hm):
                r['track_zoom'] = track
                r['maps']['sm_zoom'] = maps
        for t, r in enumerate(results):
            r['zoom'] = [zoom_entry(wins[t], lengths[t], r, second, t)]
    if timing is not None:
        timing.update(zoom_fit_ms=zoom_ms[0], zoom_forward_ms=zoom_ms[1], seq_zoom_pitch=int(pitch))
    return _finish(results, keep_maps)


class _Clip:
    """What the online trackers share: the size of the clip's frames, fixed by the first push, and push().  A tracker has its state, None at a clip's
    start, and _track(results), which adds what it tracks to the dicts of pass 1 and moves the state on."""

    def reset(self):
        self.state, self.shape = None, None

    def same_size(self, shape):
        if self.shape is not None and shape != self.shape:
            raise ValueError('the frames of a clip have one size: this clip began with %s, got %s' % (self.shape, shape))
        self.shape = shape

    def push(self, frames, keep_maps=False):
        results = _first_pass(self.engine, frames, clip=self, **self.pass1)
        self._track(results)
        return _finish(results, keep_maps)


class SequenceTracker(_Clip):
    """The online form of predict_sequence(mode='filter'): push(frames) takes the next frames of the clip, a few or one at a time, and returns
    their dicts with 'track'; the filter's float64 belief is carried from call to call, so any split of a clip gives the values of one
    predict_sequence over all of it.  Every push must bring frames of the first push's size.  reset() starts a new clip.
    camera=True is the online form of predict_sequence(mode='filter', camera=True): the last fitted frame and the carry of
    motion.camera_shifts travel from push to push beside the belief (the shift of a push's first frame applies to the transition from the carried
    belief), so any split gives the values of the one call; reset() clears both.
    flow_centre=True is the online form of predict_sequence(mode='filter', flow_centre=True), the first online use of local motion:
    the last fitted frame travels from push to push; a push stacks it in front of its own frames, matches every frame against its predecessor
    (one Engine.frame_flow call with a one-slot ref table, search radius flow_search) and drops the carried frame's row again -- the first row of
    a clip's first push has no predecessor and is zero --, so any split gives the bits of the one call; reset() forgets the frame.  Not with
    camera=True (ValueError)."""

    def __init__(self, engine, sigma=SEQ_SIGMA, rho=SEQ_RHO, radius=None, use_sm=True, batch_size=16, camera=False, camera_search=SEQ_CAMERA_SEARCH,
                 flow_centre=False, flow_search=SEQ_FLOW_SEARCH, **kw):
        self.engine, self.sigma, self.rho, self.radius, self.use_sm = engine, sigma, rho, radius, use_sm
        self.camera, self.camera_search = _check_camera_search(camera, camera_search), int(camera_search)
        self.flow_centre, self.flow_search = _check_flow_centre(flow_centre, flow_search, camera=self.camera), int(flow_search)
        self.pass1 = dict(kw, use_sm=use_sm, batch_size=batch_size, **({'keep_frames': True} if self.camera or self.flow_centre else {}))
        self.reset()

    def reset(self):
        super().reset()
        self.last_frame, self.carry = None, (0, 0)

    def _track(self, results):
        with torch.cuda.stream(self.engine._stream):
            moving = {}
            if self.camera:
                moving['shift'], self.last_frame, self.carry = _camera(self.engine, results, self.camera_search, self.last_frame, self.carry)
            if self.flow_centre:
                moving['centre'], x = _flow_centre(self.engine, results, self.flow_search, prev=self.last_frame)
                self.last_frame = x[-1].clone()
            seq = self.engine.seq_filter(_stacked(results, 'sm' if self.use_sm else 'pd'), self.sigma, self.rho, radius=self.radius, state=self.state, **moving)
            self.state = seq['state']
            geom = _geom(results)
            for r, track in zip(results, _track_entries(seq, 'filter', lambda pts: fit_to_source(pts, geom))):
                r['track'] = track


class LagTracker(_Clip):
    """The online form of predict_sequence(mode='lag', lag=L): push(frames) takes the next frames of the clip, runs pass 1 on
    them and returns the dicts that became FINAL with this push -- those of the frames now `lag` frames old, possibly an empty list --, each
    with a 'track' of mode 'lag'; flush() returns the rest, with the future they have, and starts a new clip.  The pending frames' maps, float64
    beliefs, norm and reset live in the state of Engine.seq_smooth_lag, so a held-back dict carries no 'maps'.  Any split of a clip into pushes
    gives the values of one predict_sequence over all of it.  Every push must bring frames of the first push's size.  reset() drops the
    pending frames and starts a new clip."""

    def __init__(self, engine, lag, sigma=SEQ_SIGMA, rho=SEQ_RHO, radius=None, use_sm=True, batch_size=16, **kw):
        if int(lag) < 1:
            raise ValueError('lag must be >= 1, got %r (lag 0 is the causal filter: SequenceTracker)' % (lag,))
        self.engine, self.lag, self.sigma, self.rho, self.radius, self.use_sm = engine, int(lag), sigma, rho, radius, use_sm
        self.pass1 = dict(kw, use_sm=use_sm, batch_size=batch_size)
        self.reset()

    def reset(self):
        super().reset()
        self.pending = []

    def _emit(self, hm, flush):
        """The new frames' maps (None: none) through the engine -> the pending dicts that became final, with their 'track'."""
        with torch.cuda.stream(self.engine._stream):
            if hm is None:
                hm = self.state['hm'][0, :0]      # no new frame: [0,HH,WW,K]
            seq = self.engine.seq_smooth_lag(hm, self.sigma, self.rho, self.lag, radius=self.radius, state=self.state, flush=flush)
            self.state = seq['state']
            E = int(seq['lag'].shape[0])
            done, self.pending = self.pending[:E], self.pending[E:]
            if E:
                geom = _geom(done)
                for r, track in zip(done, _track_entries(seq, 'lag', lambda pts: fit_to_source(pts, geom))):
                    r['track'] = track
        return done

    def push(self, frames):
        results = _first_pass(self.engine, frames, clip=self, **self.pass1)
        with torch.cuda.stream(self.engine._stream):
            hm = _stacked(results, 'sm' if self.use_sm else 'pd')
        self.pending += _finish(results, False)      # the state holds the maps it needs
        return self._emit(hm, False)

    def flush(self):
        done = self._emit(None, True) if self.pending else []
        self.reset()
        return done


# ------------------------------------------------------------------ clips with several people
def _people_joint_maps(engine, pd, cells, batch_size):
    """pd [T,60,90,9], the frames' part-detector probabilities, and cells int32 [M,T,2], every track's torso cell -> [M,T,60,90,9]: per (frame,
    track) the spatial model on [pd of the frame, the torso blob at the track's cell], as probabilities; batch_size frames at a time."""
    M, T = cells.shape[:2]
    out = []
    for lo in range(0, T, batch_size):
        hi = min(T, lo + batch_size)
        at = cells[:, lo:hi].permute(1, 0, 2).reshape(-1, 2).contiguous()                      # (frame, track) order
        blob = engine.torso_infer(None, cells=at)['torso']
        hm10 = torch.cat([pd[lo:hi].repeat_interleave(M, dim=0), blob], dim=3)
        prob, _ = engine.softmax_argmax(engine.spatial_model(hm10), want_prob=True)
        out.append(prob.view(hi - lo, M, *prob.shape[1:]))
    return torch.cat(out).permute(1, 0, 2, 3, 4).contiguous()




def _people_pass(engine, results, people, mode, sigma, torso_sigma, rho, radius, exclude, people_threshold, batch_size, states, timing):
    """Steps 2 to 5 of predict_sequence_people on the dicts of pass 1, which gain 'tracks' and 'track'; states: the filter's (torso, joints).  Returns the new states."""
    M, (cells_key, value, flag) = int(people), SEQ_KEYS[mode]
    with torch.cuda.stream(engine._stream):
        timer = DeviceTimer(engine)
        torso = engine.seq_tracks(_stacked(results, 'torso_prob'), M, torso_sigma, rho, exclude=exclude, mode=mode, state=states[0])
        timer.mark()
        hm = _people_joint_maps(engine, _stacked(results, 'pd'), torso[cells_key], int(batch_size))
        timer.mark()
        seq = _seq_call(engine, mode, hm, sigma, rho, radius, **({'state': states[1]} if mode == 'filter' else {}))
        geom = _geom(results)
        tc, tv, tf = (torso[k].cpu().numpy() for k in (cells_key, 'value', flag))                 # [M,T,2], [M,T], [M,T]
        tpts, _ = fit_to_source(np.where(tc < 0, -1.0, tc.astype(np.float64) * STRIDE).transpose(1, 0, 2), geom)      # [T,M,2]
        present = (tv > people_threshold) & (tf != 2)
        count = int(present.any(axis=1).sum())      # the tracks present in at least one frame of the call
        person = [_track_entries({k: seq[k][m] for k in SEQ_KEYS[mode]}, mode, lambda pts: fit_to_source(pts, geom)) for m in range(M)]
        for t, r in enumerate(results):
            r['tracks'] = dict({'mode': mode, 'count': count, 'torso': tpts[t], 'torso_value': tv[:, t], 'present': present[:, t]},
                               **{k: np.stack([p[t][k] for p in person]) for k in ('points', 'inside', value, flag)})
            r['track'] = person[0][t]
        if timing is not None:
            timer.add(timing, 'seq_torso_ms', 'seq_people_sm_ms')
    return torso.get('state'), seq.get('state')


def _check_people(people, zoom):
    if not isinstance(people, int) or not 1 <= people <= 4:
        raise ValueError('people must be an integer in 1..4, got %r' % (people,))
    if zoom:
        raise ValueError('predict_sequence_people has no zoom pass: a zoom pass per track is out of scope')


def predict_sequence_people(engine, frames, people, mode='viterbi', sigma=SEQ_SIGMA, torso_sigma=SEQ_TORSO_SIGMA, rho=SEQ_RHO, exclude=SEQ_EXCLUDE,
                            people_threshold=0.0, radius=None, batch_size=16, keep_maps=False, zoom=False, timing=None, camera=False, flow=0, flow_centre=False, **kw):
    """The frames of ONE clip with up to people = M (1..4) persons in it; frames as for predict_sequence.  On the device:
      1. predict_images(frames, use_sm=True, people=1, keep_maps=True, torso_prob=True, **kw): per frame the part-detector maps and the torso map
         spatial_softmax(E);
      2. Engine.seq_tracks on the stacked torso maps [T,60,90]: M torso tracks -- track 0 the most probable torso track (mode 'viterbi') or the
         causal filter's (mode 'filter'), track n the same through what is left once the cells within `exclude` of the tracks before it are
         taken out of every frame; identity is stable by construction, tracks are reported in pass order and never re-sorted;
      3. per (frame, track) the spatial model on [the frame's pd maps, the blob at the track's cell], batch_size frames at a time;
      4. the existing Engine.seq_filter / seq_viterbi on the [M,T,60,90,K] maps, the persons as its sequences;
      5. evaluation.fit_to_source.
    Returns predict_images' dicts, every key with its value, plus
      'tracks': {'mode', 'count' (the tracks present in at least one frame of the call), 'torso' float64 [M,2] (row, col) in the frame's pixels,
                 'torso_value' float32 [M] (the torso map at the track's cell, 0 where an earlier track excludes it), 'present' bool [M]
                 (torso_value > people_threshold and the torso pass did not meet an all-zero map there, flag 2), 'points' float64 [M,K,2],
                 'inside' bool [M,K], 'maxes' / 'breaks' or 'norm' / 'reset' [M,K]}
      'track': track 0 in the layout of predict_sequence, so that what reads 'track' works unchanged.
    timing also receives 'seq_torso_ms' and 'seq_people_sm_ms', the device times of steps 2 and 3.  'maps' is kept only with keep_maps.
    exclude (SEQ_EXCLUDE = 4 cells), torso_sigma (SEQ_TORSO_SIGMA = 1.5), sigma, rho and people_threshold are untuned placeholders -- no
    consecutive-frame data and no trained weights are at hand -- and what this buys with trained weights has not been measured.  zoom=True
    and camera=True raise ValueError (the torso passes have no moving form), flow != 0 too (pooling per track is out of scope), and
    flow_centre=True (the torso passes have no centred form)."""
    if flow_centre:
        raise ValueError('predict_sequence_people has no flow-centred scan: the torso passes have no centred form (flow_centre=True belongs to predict_sequence)')
    if camera:
        raise ValueError('predict_sequence_people has no camera estimate: the torso passes have no moving form (camera=True belongs to predict_sequence)')
    if flow:
        raise ValueError('predict_sequence_people has no flow pooling: every track has maps of its own (flow=%r belongs to predict_sequence)' % (flow,))
    if mode not in ('filter', 'viterbi'):
        raise ValueError("mode must be 'filter' or 'viterbi', got %r (the torso tracks have the filter and Viterbi only)" % (mode,))
    _check_people(people, zoom)
    results = _first_pass(engine, frames, use_sm=True, people=1, batch_size=batch_size, torso_prob=True, timing=timing, **kw)
    _people_pass(engine, results, people, mode, sigma, torso_sigma, rho, radius, exclude, people_threshold, batch_size, (None, None), timing)
    return _finish(results, keep_maps)


class PeopleTracker(_Clip):
    """The online form of predict_sequence_people(mode='filter'): push(frames) takes the next frames of the clip and returns their dicts with
    'tracks' and 'track'; the float64 beliefs of the torso passes and of the persons' joints are both carried from call to call, so any split of
    a clip gives the values of one predict_sequence_people over all of it -- except 'count', which counts over the frames of its own push.
    Every push must bring frames of the first push's size.  reset() starts a new clip."""

    def __init__(self, engine, people, sigma=SEQ_SIGMA, torso_sigma=SEQ_TORSO_SIGMA, rho=SEQ_RHO, exclude=SEQ_EXCLUDE, people_threshold=0.0, radius=None,
                 batch_size=16, **kw):
        _check_people(people, False)
        self.engine, self.people, self.pass1 = engine, people, dict(kw, use_sm=True, people=1, batch_size=batch_size, torso_prob=True)
        self.args = (sigma, torso_sigma, rho, radius, exclude, people_threshold, batch_size)
        self.reset()

    def _track(self, results):
        self.state = _people_pass(self.engine, results, self.people, 'filter', *self.args, self.state or (None, None), None)
