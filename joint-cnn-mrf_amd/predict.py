"""From images of any size to joints in each image's own pixels: Engine.fit_images letterboxes a ragged batch of byte images
into the 480x720 frame the tower was built for, Engine.forward runs on the bytes -- with use_sm the torso map is inferred (torso='infer',
DESIGN.md 4.15): a photo has no annotation -- and evaluation.fit_to_source maps every coordinate back through the fit.

Black bars and a changed scale are inputs the network was not trained on; how well a FLIC-trained model does on letterboxed photos has not been
measured.  Multi-scale and mirrored evaluation are not offered here: the inferred torso is not defined under them (multiscale.py).

The zoom pass (predict_images(zoom=True)) answers the changed scale: a window around every person the first pass found, sized
so that the person's torso gets the length FLIC torsos have in a 480-row frame, is fitted by Engine.fit_windows and run through the tower
again, with the torso blob at the window's centre; evaluation.window_to_source maps the joints back.  What this buys with FLIC-trained weights
has not been measured either.

Pictures: skeleton_primitives turns results into capsules, render_images draws them -- and, with keep_maps, the heat maps
under them -- onto the images at their own size through Engine.render_poses.

Frame sequences: predict_sequence takes the frames of a clip, all of one size, and adds to every frame's result a 'track': one
position per joint that is consistent over the clip, from Engine.seq_filter (causal) or Engine.seq_viterbi (the most probable track) on the
stacked heat maps.  SequenceTracker is the online form of the filter.  SEQ_SIGMA and SEQ_RHO are not fitted to anything; what tracking buys has
been measured on rendered clips only, not on real video.

Clips with several people: predict_sequence_people pulls up to four consistent torso tracks out of the frames' torso maps
(Engine.seq_tracks: successive passes of the temporal model, each with the earlier tracks' neighbourhoods excluded), runs the spatial model
once per (frame, track) with the blob at the track's cell and tracks every person's joints; PeopleTracker is its online form.  SEQ_EXCLUDE and
SEQ_TORSO_SIGMA are untuned placeholders too.

Smoothed marginals and the fit: predict_sequence(mode='marginal') takes every frame's position from the smoothed posterior
P(x_t | all frames) of Engine.seq_smooth, with its confidence; seq_fit re-estimates sigma (per joint) and rho on a clip's own maps by EM, without
annotations, and predict_sequence(fit_iters=) runs any mode with the fitted values.

Zoomed clips: predict_sequence_zoom runs the zoom pass on every frame of a clip in windows that follow the person and share
one cell lattice (zoom_window_track), so that two frames' maps differ by a whole number of cells, and tracks the joints through them with
Engine.seq_filter / seq_viterbi(shift=), the scans with a per-frame shift of the belief plane."""
import os

import numpy as np
import torch

from .engine import SEQ_EXCLUDE      # the exclusion half-width of Engine.seq_tracks, cells: an untuned placeholder
from .evaluation import fit_geometry, fit_to_source, peaks_to_pixels, pose_to_pixels, window_to_source

JOINT_NAMES = ('lsho', 'lelb', 'lwri', 'rsho', 'relb', 'rwri', 'lhip', 'rhip', 'nose')      # main.py:18, without the torso channel
STRIDE = 8                      # heat-map cell -> pixel of the fitted frame (the reference's `coords * 8`, test.py)
FRAME = (480, 720)
# The median over the FLIC training annotations (tests/golden/flic_train_xy.npy, 3987 people) of the distance, in pixels of their 480 x 720
# frames, from the midpoint of the shoulders to the midpoint of the hips.  A statistic of the data the network is trained on, not a tuned
# value: a zoom window is sized so that the person's torso has this length in the frame the tower reads.  tests/test_fit_windows_cpu.py
# recomputes it.
ZOOM_TORSO_PIXELS = 130.63038126031898
ZOOM_TORSO_JOINTS = ((0, 3), (6, 7))      # (lsho, rsho), (lhip, rhip)
FIT_SIDE_MAX = 16384                      # include/jcm.h: the sides of what jcm_fit_images / jcm_fit_windows fit
# The motion model of the sequence stages: the standard deviation of a joint's motion per frame in heat-map cells, and the mass of the uniform
# "anywhere" term.  Untuned placeholders: no consecutive-frame data is at hand to derive them from.
SEQ_SIGMA = 1.5
SEQ_RHO = 0.05
SEQ_TORSO_SIGMA = 1.5                     # a torso's motion per frame in cells (predict_sequence_people): an untuned placeholder
SEQ_RADIUS_MAX = 16                       # include/jcm.h: R of jcm_seq_filter / jcm_seq_viterbi
SEQ_SIGMA_MAX = 64.0                      # what seq_fit clamps a joint's sigma to when its moment reaches that of flat taps (at R = 16 such taps are flat within 3 %)
SEQ_MODES = ('filter', 'viterbi', 'marginal')
IMAGE_EXTENSIONS = ('.npy', '.png', '.jpg', '.jpeg', '.bmp', '.gif', '.tif', '.tiff', '.webp', '.ppm')


def _coords_to_points(coords):
    """int32 [B,2,K] (row, col) cells, device -> host float64 [B,K,2] pixels of the fitted frame; -1 (an empty slot) stays -1."""
    c = coords.cpu().numpy().transpose(0, 2, 1).astype(np.float64)
    return np.where(c < 0, -1.0, c * STRIDE)


def predict_images(engine, images, use_sm=True, peaks=0, decode=False, people=1, batch_size=16, pad=0, timing=None, zoom=False, keep_maps=False,
                   torso_prob=False):
    """images: a list of uint8 [h,w,3] arrays or tensors of mixed sizes (what Engine.fit_images takes).  They are fitted and run through
    engine.forward(x_u8, torso='infer' if use_sm else None, use_sm=use_sm, peaks=peaks, decode=decode, people=people) batch_size at a time.
    Returns one dict per image, everything in the image's own pixels (row, col), host numpy:
      'size' (h, w); 'joint_names'; 'geom' (y0, x0, ch, cw, h, w), the fit;
      'pd' float64 [K,2] and 'pd_inside' bool [K] (did the arg-max lie in the content rectangle, not in a bar?);
      with use_sm: 'sm', 'sm_inside', and 'torso_cell' (row, col) of the inferred torso in heat-map cells of the fitted frame;
      with peaks = P: 'pd_peaks' (and 'sm_peaks') float64 [K,P,3] = (row, col, score), filler slots (-1, -1, 0), and '*_peaks_inside' [K,P];
      with decode: 'pose' float64 [K,3] = (row, col, pose score) and 'pose_inside' [K] (people > 1: the pose of slot 0, the arg-max torso);
      with people = M > 1: 'people' = {'count', 'torso_cell' [M,2], 'torso_score' [M], 'sm' [M,K,2], 'sm_inside' [M,K]}, slots from count on -1.
      with zoom (needs use_sm; every key above keeps its value): 'zoom', a list with one entry per person -- one when people == 1, the slots
        below count otherwise -- from the second pass (zoom_windows, Engine.fit_windows, forward with the torso blob at the window's centre,
        evaluation.window_to_source): {'zoomed' bool, 'window' (y0, x0, h, w) in the image's pixels, 'torso_len' (the person's pass-1
        shoulder-to-hip distance in the image's pixels), 'pd', 'pd_inside', 'sm', 'sm_inside'}; a person zoom_windows skips has zoomed False
        and the pass-1 values.
      with keep_maps (every key above keeps its value): 'maps' = {'pd': device float32 [60,90,K]} and with use_sm also 'sm' (people > 1: slot 0),
        views of the first pass's probability maps of the image's batch -- what render_images(heat=...) tints with.
      with torso_prob (needs keep_maps and use_sm; every key above keeps its value): 'maps' also holds 'torso_prob', device float32 [60,90] =
        spatial_softmax of the torso energy E -- the map predict_sequence_people tracks torsos through.
    timing: a dict that receives 'fit_ms' and 'forward_ms', device-event times summed over the batches (the upload of host images is part of
    neither), and with zoom 'zoom_fit_ms' and 'zoom_forward_ms', those of the second pass."""
    if not isinstance(images, (list, tuple)) or len(images) == 0:
        raise ValueError('images must be a non-empty list of uint8 [h,w,3] images')
    if zoom and not use_sm:
        raise ValueError('zoom=True needs use_sm=True: the windows are placed at the inferred torso and sized by the spatial model\'s shoulders and hips')
    if int(batch_size) < 1:
        raise ValueError('batch_size must be >= 1, got %r' % (batch_size,))
    if torso_prob and not (keep_maps and use_sm):
        raise ValueError('torso_prob=True needs keep_maps=True and use_sm=True: the map is kept in \'maps\' and comes from the inferred torso')
    names = list(JOINT_NAMES[:engine.n_joints])
    out = []
    fit_ms = fwd_ms = 0.0
    zoom_ms = [0.0, 0.0]
    with torch.cuda.stream(engine._stream):
        for lo in range(0, len(images), int(batch_size)):
            # host images go up first, so that the fit's time is the fit's; anything that is no byte image is left for fit_images to refuse
            batch = [_upload(im, engine.device) for im in images[lo:lo + int(batch_size)]]
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
            ev[0].record(engine._stream)
            x, geom = engine.fit_images(batch, out_hw=FRAME, pad=pad)
            ev[1].record(engine._stream)
            r = engine.forward(x, 'infer' if use_sm else None, use_sm=use_sm, want_prob=bool(keep_maps), peaks=peaks, decode=decode, people=people,
                               **({'want_torso_prob': True} if torso_prob else {}))
            ev[2].record(engine._stream)
            ev[2].synchronize()
            fit_ms += ev[0].elapsed_time(ev[1])
            fwd_ms += ev[1].elapsed_time(ev[2])
            res = _to_source(r, geom, names, use_sm, peaks, decode, people)
            if keep_maps:
                for b, e in enumerate(res):
                    e['maps'] = {key: r[key + '_prob'][b] for key in (('pd', 'sm') if use_sm else ('pd',))}
                    if torso_prob:
                        e['maps']['torso_prob'] = r['torso_prob'][b]
            if zoom:
                _zoom_pass(engine, batch, res, people, int(batch_size), pad, zoom_ms)
            out.extend(res)
    if timing is not None:
        timing.update(fit_ms=fit_ms, forward_ms=fwd_ms)
        if zoom:
            timing.update(zoom_fit_ms=zoom_ms[0], zoom_forward_ms=zoom_ms[1])
    return out


def torso_length(sm):
    """sm [...,K,2] joints (row, col) -> [...]: the distance from the midpoint of the shoulders to the midpoint of the hips."""
    sm = np.asarray(sm, np.float64)
    (a, b), (c, d) = ZOOM_TORSO_JOINTS
    return np.sqrt((((sm[..., a, :] + sm[..., b, :]) / 2 - (sm[..., c, :] + sm[..., d, :]) / 2) ** 2).sum(-1))


def zoom_windows(sm, sm_inside, torso_cell, geom, image=None, frame=FRAME):
    """Where the second pass looks; host arithmetic only.  One row per person of the first pass: sm float [P,K,2] and
    sm_inside bool [P,K], the person's spatial-model joints in the pixels of their image as predict_images returns them; torso_cell int
    [P,2], the person's torso cell in the fitted frame; geom int [P,6], the first pass's fit of the person's image (y0, x0, ch, cw, h, w);
    image int [P], the index the windows name (default 0..P-1).  Returns (windows int64 [P,5] = (image, wy0, wx0, wh, ww), cells int32 [P,2],
    skipped bool [P]):
      t = torso_length(sm), in the image's pixels;  wh = max(1, floor(t * frame rows / ZOOM_TORSO_PIXELS + 0.5)),  ww = (3 * wh + 1) // 2:
        the window that puts a torso of FLIC's median length into the frame;
      (cy, cx) = the torso cell in the image's pixels (cell * STRIDE through evaluation.fit_to_source);
      wy0 = floor(cy + 0.5) - wh // 2,  wx0 = floor(cx + 0.5) - ww // 2;
      cells = the centre taken forward through the window's fit, (c - w0 + 0.5) * content / size - 0.5 + content origin, floored, // STRIDE,
        clamped to the map: where the torso blob of the second pass goes.
    skipped: one of the four torso joints is not inside; t < 2 * STRIDE * h / ch, two cells of the first pass in the image's pixels, below
    which t is quantisation; wh or ww above 16384; or the window shares no pixel with the image (a torso cell far out in a bar), which
    Engine.fit_windows would refuse.  A skipped person is not zoomed; their window and cell are still reported."""
    sm, sm_inside = np.asarray(sm, np.float64), np.asarray(sm_inside, bool)
    cell, geom = np.asarray(torso_cell, np.int64), np.asarray(geom, np.int64)
    P = sm.shape[0]
    if sm.ndim != 3 or sm.shape[2] != 2 or sm.shape[1] < 8 or sm_inside.shape != sm.shape[:2] or cell.shape != (P, 2) or geom.shape != (P, 6):
        raise ValueError('zoom_windows expects sm [P,K >= 8,2], sm_inside [P,K], torso_cell [P,2] and geom [P,6]; got %s, %s, %s, %s' %
                         (sm.shape, sm_inside.shape, cell.shape, geom.shape))
    image = np.arange(P, dtype=np.int64) if image is None else np.asarray(image, np.int64).reshape(P)
    OH, OW = int(frame[0]), int(frame[1])
    t = torso_length(sm)
    wh = np.maximum(1, np.floor(t * OH / ZOOM_TORSO_PIXELS + 0.5)).astype(np.int64)
    ww = (3 * wh + 1) // 2
    centre, _ = fit_to_source((cell * STRIDE).astype(np.float64), geom)
    wy0 = np.floor(centre[:, 0] + 0.5).astype(np.int64) - wh // 2
    wx0 = np.floor(centre[:, 1] + 0.5).astype(np.int64) - ww // 2
    cells = np.empty((P, 2), np.int32)
    for i in range(P):
        y0, x0, ch, cw = fit_geometry(wh[i], ww[i], OH, OW)
        row = (centre[i, 0] - wy0[i] + 0.5) * ch / wh[i] - 0.5 + y0
        col = (centre[i, 1] - wx0[i] + 0.5) * cw / ww[i] - 0.5 + x0
        cells[i] = (min(max(int(np.floor(row)) // STRIDE, 0), OH // STRIDE - 1), min(max(int(np.floor(col)) // STRIDE, 0), OW // STRIDE - 1))
    torso_joints = [j for pair in ZOOM_TORSO_JOINTS for j in pair]
    h, w, ch = geom[:, 4], geom[:, 5], geom[:, 2]
    skipped = ~sm_inside[:, torso_joints].all(axis=1)
    skipped |= t < 2.0 * STRIDE * h / ch
    skipped |= (wh > FIT_SIDE_MAX) | (ww > FIT_SIDE_MAX)
    skipped |= (wy0 >= h) | (wy0 + wh <= 0) | (wx0 >= w) | (wx0 + ww <= 0)
    return np.stack([image, wy0, wx0, wh, ww], axis=1), cells, skipped


def _zoom_pass(engine, batch, res, people, batch_size, pad, zoom_ms):
    """The second pass over one batch: res, the batch's dicts from _to_source, each gain 'zoom'."""
    who = []      # (image of the batch, sm, sm_inside, torso cell) per person
    for b, r in enumerate(res):
        if people == 1:
            who.append((b, r['sm'], r['sm_inside'], r['torso_cell']))
        else:
            p = r['people']
            who.extend((b, p['sm'][m], p['sm_inside'][m], p['torso_cell'][m]) for m in range(p['count']))
    for r in res:
        r['zoom'] = []
    if not who:
        return
    image = np.array([p[0] for p in who], np.int64)
    sm, sm_inside = np.stack([p[1] for p in who]), np.stack([p[2] for p in who])
    geom1 = np.array([res[b]['geom'] for b in image], np.int64)
    wins, cells, skipped = zoom_windows(sm, sm_inside, np.array([p[3] for p in who], np.int64), geom1, image=image)
    t = torso_length(sm)
    keep = np.flatnonzero(~skipped)
    second = {}
    if len(keep):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        ev[0].record(engine._stream)
        x2, geom2 = engine.fit_windows(batch, wins[keep], out_hw=FRAME, pad=pad)
        cells_dev = torch.from_numpy(np.ascontiguousarray(cells[keep])).to(engine.device)
        ev[1].record(engine._stream)
        coords = {'pd': [], 'sm': []}
        for lo in range(0, len(keep), batch_size):
            torso = engine.torso_infer(None, cells=cells_dev[lo:lo + batch_size].contiguous())['torso']
            r2 = engine.forward(x2[lo:lo + batch_size], torso=torso, use_sm=True, want_prob=False)
            for key in coords:
                coords[key].append(r2[key + '_coords'])
        ev[2].record(engine._stream)
        ev[2].synchronize()
        zoom_ms[0] += ev[0].elapsed_time(ev[1])
        zoom_ms[1] += ev[1].elapsed_time(ev[2])
        sizes = np.array([r['size'] for r in res], np.int64)
        for key in coords:
            second[key] = window_to_source(_coords_to_points(torch.cat(coords[key])), geom2, wins[keep], sizes)
    at = {int(i): n for n, i in enumerate(keep)}
    for i, (b, sm_i, inside_i, _) in enumerate(who):
        e = {'zoomed': i in at, 'window': tuple(int(v) for v in wins[i, 1:]), 'torso_len': float(t[i])}
        if i in at:
            for key in ('pd', 'sm'):
                e[key], e[key + '_inside'] = second[key][0][at[i]], second[key][1][at[i]]
        else:
            e.update(pd=res[b]['pd'], pd_inside=res[b]['pd_inside'], sm=sm_i, sm_inside=inside_i)
        res[b]['zoom'].append(e)


def _upload(im, device):
    if isinstance(im, np.ndarray) and im.dtype == np.uint8:
        return torch.from_numpy(np.ascontiguousarray(im)).to(device)
    if isinstance(im, torch.Tensor) and im.dtype == torch.uint8 and im.device.type == 'cpu':
        return im.to(device)
    return im


def _to_source(r, geom, names, use_sm, peaks, decode, people):
    """The dict of one forward on fitted images -> the per-image dicts of predict_images."""
    B = geom.shape[0]
    res = [{'size': (int(g[4]), int(g[5])), 'joint_names': names, 'geom': tuple(int(v) for v in g)} for g in geom]
    for key in (('pd', 'sm') if use_sm else ('pd',)):
        pts, inside = fit_to_source(_coords_to_points(r[key + '_coords']), geom)
        for b in range(B):
            res[b][key], res[b][key + '_inside'] = pts[b], inside[b]
        if peaks:
            pk, pin = fit_to_source(peaks_to_pixels(r[key + '_peaks'], STRIDE), geom)
            for b in range(B):
                res[b][key + '_peaks'], res[b][key + '_peaks_inside'] = pk[b], pin[b]
    if use_sm:
        cells = r['torso_cell'].cpu().numpy()
        for b in range(B):
            res[b]['torso_cell'] = (int(cells[b, 0]), int(cells[b, 1]))
    if decode:
        pose = r['pose'] if people == 1 else {f: v[:, 0].contiguous() for f, v in r['pose'].items()}
        ps, pin = fit_to_source(pose_to_pixels(pose, r['pd_peaks'], STRIDE), geom)
        for b in range(B):
            res[b]['pose'], res[b]['pose_inside'] = ps[b], pin[b]
    if people > 1:
        p = r['people']
        M, K = p['sm_coords'].shape[1], p['sm_coords'].shape[3]
        pts = _coords_to_points(p['sm_coords'].reshape(B * M, 2, K)).reshape(B, M, K, 2)
        pts, inside = fit_to_source(pts, geom)
        count, cells, score = p['count'].cpu().numpy(), p['torso_cell'].cpu().numpy(), p['torso_score'].cpu().numpy()
        for b in range(B):
            res[b]['people'] = {'count': int(count[b]), 'torso_cell': cells[b], 'torso_score': score[b], 'sm': pts[b], 'sm_inside': inside[b]}
    return res


# ------------------------------------------------------------------ frame sequences
def _seq_sigma(sigma, K=None):
    sg = np.asarray(sigma, np.float64).reshape(-1)
    if sg.size == 0 or not np.all(np.isfinite(sg)) or np.any(sg <= 0):
        raise ValueError('sigma must be positive and finite, got %r' % (sigma,))
    if K is not None:
        if sg.size not in (1, K):
            raise ValueError('sigma must be a scalar or %d values (one per joint), got %d' % (K, sg.size))
        sg = np.broadcast_to(sg, (K,))
    return sg


def seq_radius(sigma):
    """The default tap radius of the sequence stages: min(16, ceil(3 * max sigma))."""
    return int(min(SEQ_RADIUS_MAX, np.ceil(3.0 * _seq_sigma(sigma).max())))


def seq_taps(sigma, radius, K):
    """The 1-D taps of the motion kernel jcm_seq_filter / jcm_seq_viterbi take: float64 [K, 2 * radius + 1], row k = exp(-d^2 / (2 sigma_k^2)) for
    d = -radius .. radius, divided by its sum.  sigma: a scalar or K values, in heat-map cells per frame.  The one builder: Engine.seq_* and the
    restatement of the tests share it."""
    R = int(radius)
    if R < 0:
        raise ValueError('radius must be >= 0, got %r' % (radius,))
    sg = _seq_sigma(sigma, int(K))
    d = np.arange(-R, R + 1, dtype=np.float64)
    w = np.exp(-(d[None, :] * d[None, :]) / (2.0 * sg[:, None] * sg[:, None]))
    return np.ascontiguousarray(w / w.sum(axis=1, keepdims=True))


def _one_size(frames):
    if not isinstance(frames, (list, tuple)) or len(frames) == 0:
        raise ValueError('frames must be a non-empty list of uint8 [h,w,3] images of one size')
    shapes = {tuple(f.shape) for f in frames}
    if len(shapes) != 1:
        raise ValueError('the frames of a clip have one size (one letterbox geometry); got %s' % sorted(shapes))


def _track_entries(seq, geom, mode):
    """The dict of Engine.seq_filter / seq_viterbi / seq_smooth on [T,HH,WW,K] maps and the frames' fit -> one 'track' dict per frame."""
    cells = seq['path' if mode == 'viterbi' else 'coords']
    pts, inside = fit_to_source(_coords_to_points(cells), geom)
    keys = {'filter': ('norm', 'reset'), 'viterbi': ('maxes', 'breaks'), 'marginal': ('conf', 'norm', 'reset', 'cut')}[mode]
    host = {k: seq[k].cpu().numpy() for k in keys}
    return [dict({'mode': mode, 'points': pts[t], 'inside': inside[t]}, **{k: host[k][t] for k in keys}) for t in range(pts.shape[0])]


def _seq_call(engine, mode, hm, sigma, rho, radius):
    if mode == 'marginal':
        return engine.seq_smooth(hm, sigma, rho, radius=radius, want_smoothed=False)
    return (engine.seq_filter if mode == 'filter' else engine.seq_viterbi)(hm, sigma, rho, radius=radius)


def _seq_maps(results, use_sm):
    return torch.stack([r['maps']['sm' if use_sm else 'pd'] for r in results]).contiguous()


def predict_sequence(engine, frames, mode='filter', sigma=SEQ_SIGMA, rho=SEQ_RHO, radius=None, use_sm=True, batch_size=16, people=1, zoom=False,
                     keep_maps=False, fit_iters=0, **kw):
    """The frames of ONE clip, in order: a list of uint8 [h,w,3] images of one size (any other size raises ValueError: a clip has one letterbox
    geometry).  predict_images(frames, keep_maps=True, **kw) runs over them; the 'sm' maps ('pd' without use_sm) are stacked on the device as
    [T,60,90,K] and go through ONE call of Engine.seq_filter (mode 'filter', causal), Engine.seq_viterbi (mode 'viterbi', the most probable
    track) or Engine.seq_smooth (mode 'marginal', the arg-max of every frame's smoothed posterior P(x_t | all frames));
    evaluation.fit_to_source maps the cells back.  Returns predict_images' dicts, every key with the value it has there, plus
      'track': {'mode', 'points' float64 [K,2] (row, col) in the frame's own pixels, 'inside' bool [K], 'norm' or 'maxes' float64 [K], 'reset' or
                'breaks' int [K]}  (the library's Z / M and its flags, include/jcm.h); mode 'marginal': 'conf' float32 [K] (the posterior at the
                point), 'norm', 'reset' and 'cut' int [K].
    fit_iters = ITERS > 0 first re-estimates sigma (per joint) and rho on the clip's own maps (seq_fit below, starting from sigma and rho) and runs
    the mode with the fitted values; frame 0's dict then carries 'seq_fit', seq_fit's return value for the clip.
    'maps' is kept only with keep_maps.  sigma (a scalar or K values, heat-map cells per frame), rho and radius are those of Engine.seq_filter;
    the defaults SEQ_SIGMA and SEQ_RHO are untuned placeholders, and what the track buys with trained weights has not been measured.
    One person, one pass: people != 1 and zoom=True raise ValueError -- associating people across frames, and windows that move from frame to
    frame, are out of scope."""
    if mode not in SEQ_MODES:
        raise ValueError("mode must be 'filter', 'viterbi' or 'marginal', got %r" % (mode,))
    if not 0 <= int(fit_iters) <= 100:
        raise ValueError('fit_iters must be 0 (off) or the EM iterations 1..100, got %r' % (fit_iters,))
    if people != 1:
        raise ValueError('predict_sequence tracks one person: people=%r would need an association of people across frames, which is out of scope' % (people,))
    if zoom:
        raise ValueError('predict_sequence has no zoom pass: its windows would move from frame to frame, which is out of scope')
    _one_size(frames)
    results = predict_images(engine, frames, use_sm=use_sm, batch_size=batch_size, keep_maps=True, **kw)
    with torch.cuda.stream(engine._stream):
        hm = _seq_maps(results, use_sm)
        fit = seq_fit(engine, hm, sigma, rho, iters=int(fit_iters)) if int(fit_iters) else None
        if fit is not None:
            sigma, rho = fit['sigma'], fit['rho']
        seq = _seq_call(engine, mode, hm, sigma, rho, radius)
        geom = np.array([r['geom'] for r in results], np.int64)
        for r, track in zip(results, _track_entries(seq, geom, mode)):
            r['track'] = track
            if not keep_maps:
                del r['maps']
        if fit is not None:
            results[0]['seq_fit'] = fit
    return results


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
                          keep_maps=False, fit_iters=0, pad=0, timing=None, **kw):
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
    been measured."""
    if mode not in SEQ_ZOOM_MODES:
        raise ValueError("mode must be 'filter' or 'viterbi', got %r (the smoother has no moving form: mode 'marginal' is not offered with zoomed clips)" % (mode,))
    if int(fit_iters) != 0:
        raise ValueError('predict_sequence_zoom has no fit: fit_iters=%r needs the smoother, which has no moving form' % (fit_iters,))
    if people != 1:
        raise ValueError('predict_sequence_zoom tracks one person: people=%r is out of scope' % (people,))
    B = int(batch_size)
    results = predict_sequence(engine, frames, mode=mode, sigma=sigma, rho=rho, radius=radius, use_sm=True, batch_size=B, keep_maps=True, torso_prob=True,
                               pad=pad, timing=timing, **kw)
    T = len(results)
    zoom_ms = [0.0, 0.0]
    with torch.cuda.stream(engine._stream):
        torso_maps = torch.stack([r['maps']['torso_prob'] for r in results]).contiguous()
        torso = engine.seq_tracks(torso_maps, 1, torso_sigma, rho, mode=mode)
        tc = torso['coords' if mode == 'filter' else 'path'].cpu().numpy().reshape(T, 2).astype(np.float64)
        geom1 = np.array([r['geom'] for r in results], np.int64)
        torso_px, _ = fit_to_source(tc * STRIDE, geom1)
        points, inside = np.stack([r['track']['points'] for r in results]), np.stack([r['track']['inside'] for r in results])
        wins, cells, shift, pitch, valid = zoom_window_track(points, inside, torso_px, geom1)
        lengths = torso_length(points)
        if pitch:
            maps, coords = [], {'pd': [], 'sm': []}
            geom2 = np.empty((T, 6), np.int64)
            for lo in range(0, T, B):
                hi = min(T, lo + B)
                batch = [_upload(im, engine.device) for im in frames[lo:hi]]
                local = wins[lo:hi].copy()
                local[:, 0] -= lo
                ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
                ev[0].record(engine._stream)
                x2, g2 = engine.fit_windows(batch, local, out_hw=FRAME, pad=pad)
                ev[1].record(engine._stream)
                blob = engine.torso_infer(None, cells=torch.from_numpy(np.ascontiguousarray(cells[lo:hi])).to(engine.device))['torso']
                r2 = engine.forward(x2, torso=blob, use_sm=True, want_prob=True)
                ev[2].record(engine._stream)
                ev[2].synchronize()
                zoom_ms[0] += ev[0].elapsed_time(ev[1])
                zoom_ms[1] += ev[1].elapsed_time(ev[2])
                geom2[lo:hi] = g2
                maps.append(r2['sm_prob'])
                for key in coords:
                    coords[key].append(r2[key + '_coords'])
            hm = torch.cat(maps).contiguous()
            seq = (engine.seq_filter if mode == 'filter' else engine.seq_viterbi)(hm, sigma, rho, radius=radius, shift=shift)
            sizes = np.array([r['size'] for r in results], np.int64)
            second = {key: window_to_source(_coords_to_points(torch.cat(coords[key])), geom2, wins, sizes) for key in coords}
            tpts, tin = window_to_source(_coords_to_points(seq['path' if mode == 'viterbi' else 'coords']), geom2, wins, sizes)
            keys = ('norm', 'reset') if mode == 'filter' else ('maxes', 'breaks')
            host = {k: seq[k].cpu().numpy() for k in keys}
        for t, r in enumerate(results):
            e = {'zoomed': bool(pitch), 'window': tuple(int(v) for v in wins[t, 1:]), 'torso_len': float(lengths[t])}
            if pitch:
                for key in ('pd', 'sm'):
                    e[key], e[key + '_inside'] = second[key][0][t], second[key][1][t]
                r['track_zoom'] = dict({'mode': mode, 'points': tpts[t], 'inside': tin[t], 'window': e['window'], 'shift': (int(shift[t, 0]), int(shift[t, 1])),
                                        'pitch': int(pitch)}, **{k: host[k][t] for k in keys})
                if keep_maps:
                    r['maps']['sm_zoom'] = hm[t]
            else:
                e.update(pd=r['pd'], pd_inside=r['pd_inside'], sm=r['sm'], sm_inside=r['sm_inside'])
            r['zoom'] = [e]
            if not keep_maps:
                del r['maps']
    if timing is not None:
        timing.update(zoom_fit_ms=zoom_ms[0], zoom_forward_ms=zoom_ms[1], seq_zoom_pitch=int(pitch))
    return results


def seq_moment(sigma, radius):
    """sum over d of d^2 w_sigma[d] of the truncated taps seq_taps builds: the 1-D second moment of the motion kernel, float64.  Monotone in sigma,
    from 0 towards the flat taps' R (R + 1) / 3."""
    R = int(radius)
    d = np.arange(-R, R + 1, dtype=np.float64)
    return float(np.sum(d * d * seq_taps(sigma, R, 1)[0]))


def seq_sigma_of_moment(target, radius, sigma_max=SEQ_SIGMA_MAX):
    """The M-step of one joint: the sigma whose truncated taps have seq_moment == target, by bisection in float64 -> (sigma, clamped).  A target at or
    above the flat taps' R (R + 1) / 3 (no sigma reaches it), or one only a sigma above sigma_max reaches, gives (sigma_max, True); a target so small
    that no representable taps have it gives the lower end of the bracket, 2^-6 cells."""
    R = int(radius)
    target = float(target)
    if R < 1:
        raise ValueError('a motion kernel of radius 0 has no sigma to fit')
    if not target < R * (R + 1) / 3.0 or seq_moment(sigma_max, R) <= target:
        return float(sigma_max), True
    lo, hi = 2.0 ** -6, float(sigma_max)
    if seq_moment(lo, R) >= target:
        return lo, False
    for _ in range(200):      # moment(lo) < target <= moment(hi) throughout
        mid = 0.5 * (lo + hi)
        if mid <= lo or mid >= hi:
            break
        if seq_moment(mid, R) < target:
            lo = mid
        else:
            hi = mid
    return (lo if abs(seq_moment(lo, R) - target) <= abs(seq_moment(hi, R) - target) else hi), False


def seq_m_step(trans_sum, sigma, rho, radius, fit_rho=True, sigma_max=SEQ_SIGMA_MAX):
    """trans_sum float64 [K,3] = (moved, jumped, squared displacement) summed over sequences and frames; sigma [K], rho: the current values ->
    (sigma' [K], rho', clamped bool [K]).  rho' = sum jumped / (sum moved + sum jumped) over all joints (rho when that is 0 / 0, or with
    fit_rho=False); sigma_k' solves seq_moment(sigma_k') = squared_k / (2 moved_k) -- the displacement has two axes with the same taps -- and a
    joint with moved_k == 0 keeps its sigma."""
    tr = np.asarray(trans_sum, np.float64)
    sigma = np.array(sigma, np.float64)
    move, jump, sq = tr[:, 0], tr[:, 1], tr[:, 2]
    total = move.sum() + jump.sum()
    new_rho = float(jump.sum() / total) if fit_rho and total > 0 else float(rho)
    new_sigma, clamped = sigma.copy(), np.zeros(sigma.shape, bool)
    for k in range(sigma.size):
        if move[k] > 0:
            new_sigma[k], clamped[k] = seq_sigma_of_moment(sq[k] / (2.0 * move[k]), radius, sigma_max)
    return new_sigma, min(max(new_rho, 0.0), 1.0), clamped


def seq_fit(engine, hm, sigma=SEQ_SIGMA, rho=SEQ_RHO, iters=10, radius=16, fit_rho=True):
    """Fit the motion model to a clip without annotations (Baum-Welch).  hm [T,HH,WW,K] or [S,T,HH,WW,K] device maps as for
    Engine.seq_smooth; sigma (a scalar or K values) and rho are the start.  Each of the `iters` iterations is one Engine.seq_smooth at the current
    values (E-step), whose 'trans' is read back and summed over s and t on the host in float64 (np.sum over the two axes), and seq_m_step
    (M-step).  Returns {'sigma' float64 [K], 'rho' float, 'loglik' float64 [iters + 1] -- the sum over sequences, frames and joints of log norm
    (frames with norm 0, reset 2, left out) at the values BEFORE each iteration and, last, at the returned ones (one more seq_smooth) --,
    'history' [(sigma [K], rho)] * (iters + 1), the values the entries of loglik belong to, 'clamped' bool [K]: the joints whose sigma the last
    M-step held at SEQ_SIGMA_MAX}.
    What is approximate: the motion kernel is not renormalised at the map's border (cells outside contribute nothing), so the transition rows of
    cells within `radius` of the border sum to less than 1 and the M-step -- exact EM for mass away from the border -- slightly overstates rho and
    understates sigma for tracks along it; and the taps are truncated at `radius`, so no sigma explains a mean squared step of R (R + 1) / 3 per
    axis or more: such a joint is clamped and reported.  radius is fixed over the iterations (16, the largest, by default) so that a growing sigma
    is not cut off by the radius its start implied."""
    iters = int(iters)
    if iters < 1:
        raise ValueError('iters must be >= 1, got %r' % (iters,))
    K = int(hm.shape[-1])
    sg = np.array(_seq_sigma(sigma, K), np.float64)
    rho = float(rho)
    R = int(radius)
    loglik, history = [], []
    clamped = np.zeros(K, bool)

    def e_step():
        r = engine.seq_smooth(hm, sg, rho, radius=R, want_smoothed=False)
        norm = r['norm'].cpu().numpy().reshape(-1)
        loglik.append(float(np.sum(np.log(norm[norm > 0]))))
        history.append((sg.copy(), rho))
        return r['trans'].cpu().numpy().reshape(-1, K, 3).sum(axis=0)

    for _ in range(iters):
        sg, rho, clamped = seq_m_step(e_step(), sg, rho, R, fit_rho=fit_rho)
    e_step()
    return {'sigma': sg, 'rho': rho, 'loglik': np.array(loglik, np.float64), 'history': history, 'clamped': clamped}


class SequenceTracker:
    """The online form of predict_sequence(mode='filter'): push(frames) takes the next frames of the clip, a few or one at a time, and returns
    their dicts with 'track'; the filter's float64 belief is carried from call to call, so any split of a clip gives the values of one
    predict_sequence over all of it.  Every push must bring frames of the first push's size.  reset() starts a new clip."""

    def __init__(self, engine, sigma=SEQ_SIGMA, rho=SEQ_RHO, radius=None, use_sm=True, batch_size=16, **kw):
        self.engine, self.sigma, self.rho, self.radius, self.use_sm, self.batch_size, self.kw = engine, sigma, rho, radius, use_sm, batch_size, kw
        self.reset()

    def reset(self):
        self.state, self.shape = None, None

    def push(self, frames, keep_maps=False):
        _one_size(frames)
        shape = tuple(frames[0].shape)
        if self.shape is not None and shape != self.shape:
            raise ValueError('the frames of a clip have one size: this clip began with %s, got %s' % (self.shape, shape))
        self.shape = shape
        results = predict_images(self.engine, frames, use_sm=self.use_sm, batch_size=self.batch_size, keep_maps=True, **self.kw)
        with torch.cuda.stream(self.engine._stream):
            seq = self.engine.seq_filter(_seq_maps(results, self.use_sm), self.sigma, self.rho, radius=self.radius, state=self.state)
            self.state = seq['state']
            geom = np.array([r['geom'] for r in results], np.int64)
            for r, track in zip(results, _track_entries(seq, geom, 'filter')):
                r['track'] = track
                if not keep_maps:
                    del r['maps']
        return results


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


def _people_entries(torso, seq, geom, mode, people_threshold):
    """The dicts of Engine.seq_tracks on [T,60,90] and of Engine.seq_filter / seq_viterbi on [M,T,60,90,K], and the frames' fit -> per frame
    ('tracks', 'track'); `count` is filled in by the caller."""
    cells_key, value, flag = ('coords', 'norm', 'reset') if mode == 'filter' else ('path', 'maxes', 'breaks')
    tc = torso[cells_key].cpu().numpy()                                                       # [M,T,2]
    tv, tf = torso['value'].cpu().numpy(), torso[flag].cpu().numpy()                          # [M,T]
    M, T = tv.shape
    tpts, _ = fit_to_source(np.where(tc < 0, -1.0, tc.astype(np.float64) * STRIDE).transpose(1, 0, 2), geom)      # [T,M,2]
    jc = seq[cells_key]                                                                       # [M,T,2,K]
    K = jc.shape[3]
    pts, inside = fit_to_source(_coords_to_points(jc.permute(1, 0, 2, 3).reshape(T * M, 2, K)).reshape(T, M, K, 2), geom)
    v, f = seq[value].cpu().numpy(), seq[flag].cpu().numpy()                                  # [M,T,K]
    present = (tv > people_threshold) & (tf != 2)
    out = []
    for t in range(T):
        tracks = {'mode': mode, 'count': 0, 'torso': tpts[t], 'torso_value': tv[:, t], 'present': present[:, t], 'points': pts[t], 'inside': inside[t],
                  value: v[:, t], flag: f[:, t]}
        track = {'mode': mode, 'points': pts[t, 0], 'inside': inside[t, 0], value: v[0, t], flag: f[0, t]}
        out.append((tracks, track))
    return out, present


def _people_pass(engine, results, people, mode, sigma, torso_sigma, rho, radius, exclude, people_threshold, batch_size, states, timing):
    """Steps 2 to 5 of predict_sequence_people on the dicts of predict_images(keep_maps=True, torso_prob=True); states: (torso state, joint
    state) of the filter or (None, None).  Returns the new states and the [M,T] presence."""
    M = int(people)
    with torch.cuda.stream(engine._stream):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        ev[0].record(engine._stream)
        torso_maps = torch.stack([r['maps']['torso_prob'] for r in results]).contiguous()
        torso = engine.seq_tracks(torso_maps, M, torso_sigma, rho, exclude=exclude, mode=mode, state=states[0])
        ev[1].record(engine._stream)
        pd = torch.stack([r['maps']['pd'] for r in results]).contiguous()
        hm = _people_joint_maps(engine, pd, torso['coords' if mode == 'filter' else 'path'], int(batch_size))
        ev[2].record(engine._stream)
        seq = engine.seq_filter(hm, sigma, rho, radius=radius, state=states[1]) if mode == 'filter' else engine.seq_viterbi(hm, sigma, rho, radius=radius)
        geom = np.array([r['geom'] for r in results], np.int64)
        entries, present = _people_entries(torso, seq, geom, mode, people_threshold)
        for r, (tracks, track) in zip(results, entries):
            r['tracks'], r['track'] = tracks, track
        if timing is not None:
            ev[2].synchronize()
            timing['seq_torso_ms'] = timing.get('seq_torso_ms', 0.0) + ev[0].elapsed_time(ev[1])
            timing['seq_people_sm_ms'] = timing.get('seq_people_sm_ms', 0.0) + ev[1].elapsed_time(ev[2])
    return (torso.get('state'), seq.get('state')), present


def _check_people(people, zoom):
    if not isinstance(people, int) or not 1 <= people <= 4:
        raise ValueError('people must be an integer in 1..4, got %r' % (people,))
    if zoom:
        raise ValueError('predict_sequence_people has no zoom pass: a zoom pass per track is out of scope')


def predict_sequence_people(engine, frames, people, mode='viterbi', sigma=SEQ_SIGMA, torso_sigma=SEQ_TORSO_SIGMA, rho=SEQ_RHO, exclude=SEQ_EXCLUDE,
                            people_threshold=0.0, radius=None, batch_size=16, keep_maps=False, zoom=False, timing=None, **kw):
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
    raises ValueError."""
    if mode not in ('filter', 'viterbi'):
        raise ValueError("mode must be 'filter' or 'viterbi', got %r (the torso tracks have the filter and Viterbi only)" % (mode,))
    _check_people(people, zoom)
    _one_size(frames)
    results = predict_images(engine, frames, use_sm=True, people=1, batch_size=batch_size, keep_maps=True, torso_prob=True, timing=timing, **kw)
    _, present = _people_pass(engine, results, people, mode, sigma, torso_sigma, rho, radius, exclude, people_threshold, batch_size, (None, None), timing)
    for r in results:
        r['tracks']['count'] = int(present.any(axis=1).sum())
        if not keep_maps:
            del r['maps']
    return results


class PeopleTracker:
    """The online form of predict_sequence_people(mode='filter'): push(frames) takes the next frames of the clip and returns their dicts with
    'tracks' and 'track'; the float64 beliefs of the torso passes and of the persons' joints are both carried from call to call, so any split of
    a clip gives the values of one predict_sequence_people over all of it -- except 'count', which counts over the frames of its own push.
    Every push must bring frames of the first push's size.  reset() starts a new clip."""

    def __init__(self, engine, people, sigma=SEQ_SIGMA, torso_sigma=SEQ_TORSO_SIGMA, rho=SEQ_RHO, exclude=SEQ_EXCLUDE, people_threshold=0.0, radius=None,
                 batch_size=16, **kw):
        _check_people(people, False)
        self.engine, self.people, self.kw = engine, people, kw
        self.args = (sigma, torso_sigma, rho, radius, exclude, people_threshold, batch_size)
        self.reset()

    def reset(self):
        self.states, self.shape = (None, None), None

    def push(self, frames, keep_maps=False):
        _one_size(frames)
        shape = tuple(frames[0].shape)
        if self.shape is not None and shape != self.shape:
            raise ValueError('the frames of a clip have one size: this clip began with %s, got %s' % (self.shape, shape))
        self.shape = shape
        results = predict_images(self.engine, frames, use_sm=True, people=1, batch_size=self.args[-1], keep_maps=True, torso_prob=True, **self.kw)
        self.states, present = _people_pass(self.engine, results, self.people, 'filter', *self.args, self.states, None)
        for r in results:
            r['tracks']['count'] = int(present.any(axis=1).sum())
            if not keep_maps:
                del r['maps']
        return results


# ------------------------------------------------------------------ pictures of the result
NECK = -1      # no joint of the network: the midpoint of the shoulders, the floor-halved sum of their fixed-point coordinates
# limbs as (first joint, second joint); a limb takes the colour of its second joint
SKELETON = ((0, 1), (1, 2), (3, 4), (4, 5), (0, 3), (0, 6), (3, 7), (6, 7), (NECK, 8))
# colorize's table (tensorboard.py:6-18), 0xRRGGBB per joint of JOINT_NAMES: shoulders green, elbows blue, wrists yellow, hips magenta, nose red
JOINT_RGB = (0x00FF00, 0x0000FF, 0xFFFF00, 0x00FF00, 0x0000FF, 0xFFFF00, 0xFF00FF, 0xFF00FF, 0xFF0000)
# bits 0, 1, 2: the joint's map tints R, G, B (jcm_render_poses)
HEAT_MASK = tuple((1 if c >> 16 & 255 else 0) | (2 if c >> 8 & 255 else 0) | (4 if c & 255 else 0) for c in JOINT_RGB)
LIMB_ALPHA, JOINT_ALPHA = 192, 255


def _fixed(v):
    """Pixels (integer coordinates are pixel centres) -> sixteenths of a pixel."""
    return int(np.floor(16.0 * float(v) + 0.5))


def _skeletons(r, which, zoom):
    """The (joints [K,2], inside [K]) pairs one image's result draws: the tracked joints for 'track' (with 'tracks' in the result one per track present in the frame); else one per entry of 'zoom' (a person the second pass skipped carries the
    first pass's values), else one per counted slot of 'people' (spatial model only), else the image's one set of joints."""
    if which == 'track' and 'tracks' in r:
        p = r['tracks']
        return [(p['points'][m], p['inside'][m]) for m in range(len(p['present'])) if p['present'][m]]
    if which in ('track', 'track_zoom'):
        return [(r[which]['points'], r[which]['inside'])]
    if zoom and 'zoom' in r:
        return [(e[which], e[which + '_inside']) for e in r['zoom']]
    if which == 'sm' and 'people' in r:
        p = r['people']
        return [(p['sm'][m], p['sm_inside'][m]) for m in range(int(p['count']))]
    return [(r[which], r[which + '_inside'])]


def skeleton_primitives(results, which='sm', zoom=True):
    """The capsules Engine.render_poses draws for `results` (dicts of predict_images; image i of the list is image i of the primitives) ->
    int32 [NP,8] = (image, ay, ax, by, bx, r, rgb, alpha), coordinates and radii in sixteenths of a pixel (floor(16 v + 0.5)).  Per image
    rl = max(16, 2 * (h + w) // 75), 2 px at 480 x 720.  Per skeleton, first the limbs of SKELETON whose two ends are inside (radius rl, the
    colour of the second joint, alpha 192; the neck exists when both shoulders do), then a disc per inside joint (radius 2 rl, alpha 255).
    which: 'sm' or 'pd', whose joints are drawn, 'track_zoom', the joints predict_sequence_zoom tracked through the windows, or 'track', the tracked joints of predict_sequence (one skeleton per present track of predict_sequence_people); with 'people' in a result one skeleton per counted slot ('sm' only); with zoom=True and 'zoom'
    in a result, one skeleton per entry of it, a zoomed person's from the second pass."""
    if which not in ('sm', 'pd', 'track', 'track_zoom'):
        raise ValueError("which must be 'sm', 'pd', 'track' or 'track_zoom', got %r" % (which,))
    rows = []
    for i, r in enumerate(results):
        if which not in r:
            raise ValueError("results[%d] has no %r joints (%s makes them)" % (i, which, {'track': 'predict_sequence', 'track_zoom': 'predict_sequence_zoom'}.get(which, 'predict_images(use_sm=%s)' % (which == 'sm'))))
        rl = max(16, 2 * (int(r['size'][0]) + int(r['size'][1])) // 75)
        for joints, inside in _skeletons(r, which, zoom):
            K = len(inside)
            pts = [(_fixed(joints[j][0]), _fixed(joints[j][1])) if inside[j] else None for j in range(K)]
            neck = None
            if K > 3 and pts[0] is not None and pts[3] is not None:
                neck = ((pts[0][0] + pts[3][0]) // 2, (pts[0][1] + pts[3][1]) // 2)
            for ja, jb in SKELETON:
                if jb >= K or ja >= K:
                    continue
                a, b = neck if ja == NECK else pts[ja], pts[jb]
                if a is not None and b is not None:
                    rows.append((i, a[0], a[1], b[0], b[1], rl, JOINT_RGB[jb], LIMB_ALPHA))
            for j in range(min(K, len(JOINT_RGB))):
                if pts[j] is not None:
                    rows.append((i, pts[j][0], pts[j][1], pts[j][0], pts[j][1], 2 * rl, JOINT_RGB[j], JOINT_ALPHA))
    return np.array(rows, np.int32).reshape(-1, 8)


def render_images(engine, images, results, heat=None, which=None, zoom=True, heat_gain=255, batch_size=16, timing=None):
    """`images` (what predict_images took) with `results` (what it returned) drawn on them by Engine.render_poses, batch_size at a time -> a list
    of host uint8 [h,w,3] arrays.  which: 'sm', 'pd', 'track' or 'track_zoom' (default: 'track_zoom' where the results have it, else 'sm' where they have it); zoom as for
    skeleton_primitives.  heat:
    None, or 'pd' / 'sm': the maps of that stage tinted under the skeleton (JOINT_RGB's colours; needs predict_images(keep_maps=True)).
    timing: a dict that receives 'render_ms', the device-event time of the render calls summed over the batches (uploads and the read-back
    are not part of it)."""
    if not isinstance(images, (list, tuple)) or len(images) != len(results) or len(images) == 0:
        raise ValueError('images and results must be non-empty lists of the same length')
    if heat not in (None, 'pd', 'sm'):
        raise ValueError("heat must be None, 'pd' or 'sm', got %r" % (heat,))
    if which is None:
        which = 'track_zoom' if 'track_zoom' in results[0] else 'sm' if 'sm' in results[0] else 'pd'
    out, ms = [], 0.0
    with torch.cuda.stream(engine._stream):
        for lo in range(0, len(images), int(batch_size)):
            batch = [_upload(im, engine.device) for im in images[lo:lo + int(batch_size)]]
            res = results[lo:lo + int(batch_size)]
            kw = {}
            if heat is not None:
                if any('maps' not in r or heat not in r['maps'] for r in res):
                    raise ValueError('heat=%r needs the maps of that stage: run predict_images(keep_maps=True%s)' % (heat, ', use_sm=True' if heat == 'sm' else ''))
                maps = [r['maps'][heat] for r in res]
                kw = dict(hm=maps, geom=np.array([r['geom'][:4] for r in res], np.int32), heat_mask=HEAT_MASK[:maps[0].shape[-1]],
                          heat_gain=heat_gain, stride=STRIDE)
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            ev[0].record(engine._stream)
            drawn = engine.render_poses(batch, skeleton_primitives(res, which, zoom), **kw)
            ev[1].record(engine._stream)
            host = [d.cpu().numpy() for d in drawn]
            ms += ev[0].elapsed_time(ev[1])
            out.extend(host)
    if timing is not None:
        timing.update(render_ms=ms)
    return out


# ------------------------------------------------------------------ the command line (main.py --predict)
def expand_paths(paths):
    """Files as given, directories expanded to their image files in sorted order."""
    files = []
    for p in paths:
        if os.path.isdir(p):
            files.extend(os.path.join(p, f) for f in sorted(os.listdir(p)) if f.lower().endswith(IMAGE_EXTENSIONS) and os.path.isfile(os.path.join(p, f)))
        else:
            files.append(p)
    if not files:
        raise SystemExit('--predict: no image file in %s' % (list(paths),))
    return files


def load_image(path):
    """uint8 [h,w,3].  .npy files are read by numpy; every other extension goes through PIL where it is installed (it is no requirement)."""
    if path.lower().endswith('.npy'):
        a = np.load(path)
        if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3:
            raise SystemExit('--predict: %s holds %s %s; a uint8 [h,w,3] array is expected' % (path, a.dtype, a.shape))
        return np.ascontiguousarray(a)
    try:
        from PIL import Image
    except ImportError:
        raise SystemExit('--predict: %s needs PIL to be decoded and PIL is not installed; pass the image as a .npy file holding uint8 [h,w,3]' % path)
    with Image.open(path) as im:
        return np.ascontiguousarray(np.asarray(im.convert('RGB'), dtype=np.uint8))


def _listed(v):
    """numpy / tuples -> what json.dump takes."""
    if isinstance(v, dict):
        return {k: _listed(x) for k, x in v.items()}
    if isinstance(v, np.ndarray):
        return _listed(v.tolist())
    if isinstance(v, (list, tuple)):
        return [_listed(x) for x in v]
    if isinstance(v, float) and not np.isfinite(v):
        return None
    if isinstance(v, (np.integer, np.floating, np.bool_)):
        return _listed(v.item())
    return v


def predictions_document(files, results):
    return {'joint_names': results[0]['joint_names'], 'frame': list(FRAME), 'stride': STRIDE,
            'images': [dict({'path': f}, **{k: _listed(v) for k, v in r.items() if k not in ('joint_names', 'maps')}) for f, r in zip(files, results)]}
