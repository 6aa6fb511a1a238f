"""From images of any size to joints in each image's own pixels: Engine.fit_images letterboxes a ragged batch of byte images
into the 480x720 frame the tower was built for, Engine.forward runs on the bytes -- with use_sm the torso map is inferred (torso='infer',
DESIGN.md 4.15): a photo has no annotation -- and evaluation.fit_to_source maps every coordinate back through the fit.

Black bars and a changed scale are inputs the network was not trained on; how well a FLIC-trained model does on letterboxed photos has not been
measured.  Multi-scale and mirrored evaluation are not offered here: the inferred torso is not defined under them (multiscale.py).

The zoom pass (predict_images(zoom=True)) answers the changed scale: a window around every person the first pass found, sized
so that the person's torso gets the length FLIC torsos have in a 480-row frame, is fitted by Engine.fit_windows and run through the tower
again, with the torso blob at the window's centre; evaluation.window_to_source maps the joints back.  What this buys with FLIC-trained weights
has not been measured either.  second_pass is the one copy of that pass: the zoomed clips of clips.py run it too."""
import numpy as np
import torch

from ..evaluation import fit_geometry, fit_to_source, peaks_to_pixels, pose_to_pixels, window_to_source

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


class DeviceTimer:
    """Device-event times of successive stages on the engine's stream: the constructor and mark() record an event where they stand; add(into, *slots)
    waits for the last mark and adds the milliseconds between mark i and mark i + 1 to into[slots[i]] (a list's index, or a dict's key, which starts at 0)."""

    def __init__(self, engine):
        self.stream, self.events = engine._stream, []
        self.mark()

    def mark(self):
        self.events.append(torch.cuda.Event(enable_timing=True))
        self.events[-1].record(self.stream)

    def add(self, into, *slots):
        self.events[-1].synchronize()
        for slot, a, b in zip(slots, self.events, self.events[1:]):
            into[slot] = (into.get(slot, 0.0) if isinstance(into, dict) else into[slot]) + a.elapsed_time(b)


def _coords_to_points(coords):
    """int32 [B,2,K] (row, col) cells, device -> host float64 [B,K,2] pixels of the fitted frame; -1 (an empty slot) stays -1."""
    c = coords.cpu().numpy().transpose(0, 2, 1).astype(np.float64)
    return np.where(c < 0, -1.0, c * STRIDE)


def predict_images(engine, images, use_sm=True, peaks=0, decode=False, people=1, batch_size=16, pad=0, timing=None, zoom=False, keep_maps=False,
                   torso_prob=False, keep_frames=False, keep_peaks=False):
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
      with keep_frames (needs keep_maps; every key above keeps its value): 'maps' also holds 'frame', device uint8 [480,720,3], the fitted byte
        frame the tower read, a view of the batch -- what Engine.frame_shift estimates the camera's motion from.
      with keep_peaks (needs keep_maps, use_sm, decode and people == 1; every key above keeps its value): 'maps' also holds 'torso', device float32
        [60,90,1], the inferred torso map, 'pd_peaks' = {'cells' int32 [K,P,2], 'count' int32 [K]} and 'pose_index' int32 [K], views of the batch's
        device results -- what the clip decode builds its tables from.
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
    if keep_frames and not keep_maps:
        raise ValueError('keep_frames=True needs keep_maps=True: the fitted frame is kept in \'maps\'')
    if keep_peaks and not (keep_maps and use_sm and decode and people == 1):
        raise ValueError('keep_peaks=True needs keep_maps=True, use_sm=True, decode=True and people=1: the candidates and the torso map are kept in \'maps\'')
    names = list(JOINT_NAMES[:engine.n_joints])
    out = []
    ms, zoom_ms = {'fit_ms': 0.0, 'forward_ms': 0.0}, [0.0, 0.0]
    with torch.cuda.stream(engine._stream):
        for lo in range(0, len(images), int(batch_size)):
            # host images go up first, so that the fit's time is the fit's; anything that is no byte image is left for fit_images to refuse
            batch = [_upload(im, engine.device) for im in images[lo:lo + int(batch_size)]]
            timer = DeviceTimer(engine)
            x, geom = engine.fit_images(batch, out_hw=FRAME, pad=pad)
            timer.mark()
            r = engine.forward(x, 'infer' if use_sm else None, use_sm=use_sm, want_prob=bool(keep_maps), peaks=peaks, decode=decode, people=people,
                               **({'want_torso_prob': True} if torso_prob else {}))
            timer.mark()
            timer.add(ms, 'fit_ms', 'forward_ms')
            res = _to_source(r, geom, names, use_sm, peaks, decode, people)
            if keep_maps:
                for b, e in enumerate(res):
                    e['maps'] = {key: r[key + '_prob'][b] for key in (('pd', 'sm') if use_sm else ('pd',))}
                    if torso_prob:
                        e['maps']['torso_prob'] = r['torso_prob'][b]
                    if keep_frames:
                        e['maps']['frame'] = x[b]
                    if keep_peaks:
                        e['maps'].update(torso=r['torso'][b], pd_peaks={f: r['pd_peaks'][f][b] for f in ('cells', 'count')}, pose_index=r['pose']['index'][b])
            if zoom:
                _zoom_pass(engine, batch, res, people, int(batch_size), pad, zoom_ms)
            out.extend(res)
    if timing is not None:
        timing.update(ms)
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


def second_pass(engine, images, windows, cells, batch_size, pad, want_prob, zoom_ms):
    """The second pass over N windows of the device `images`: windows int64 [N,5] = (image, wy0, wx0, wh, ww); cells int32 [N,2],
    where each window's torso blob goes.  Engine.fit_windows fits them all; batch_size at a time Engine.torso_infer(cells=) and Engine.forward run
    on them; evaluation.window_to_source maps the arg-max cells back.  Returns (points, geom2, maps): points['pd' / 'sm'] = (float64 [N,K,2], inside
    bool [N,K]) in the pixels of each window's image; geom2 int [N,6], the windows' fit; maps: with want_prob the 'sm' probabilities [N,60,90,K] on
    the device.  zoom_ms: two slots that gain the device times of the fit (fit_windows) and of the forward (torso_infer and forward)."""
    cells_dev = torch.from_numpy(np.ascontiguousarray(cells)).to(engine.device)
    timer = DeviceTimer(engine)
    x2, geom2 = engine.fit_windows(images, windows, out_hw=FRAME, pad=pad)
    timer.mark()
    coords, maps = {'pd': [], 'sm': []}, []
    for lo in range(0, len(windows), batch_size):
        torso = engine.torso_infer(None, cells=cells_dev[lo:lo + batch_size].contiguous())['torso']
        r2 = engine.forward(x2[lo:lo + batch_size], torso=torso, use_sm=True, want_prob=want_prob)
        for key in coords:
            coords[key].append(r2[key + '_coords'])
        if want_prob:
            maps.append(r2['sm_prob'])
    timer.mark()
    timer.add(zoom_ms, 0, 1)
    sizes = np.array([tuple(im.shape[:2]) for im in images], np.int64)
    points = {key: window_to_source(_coords_to_points(torch.cat(coords[key])), geom2, windows, sizes) for key in coords}
    return points, geom2, (torch.cat(maps).contiguous() if want_prob else None)


def zoom_entry(window, torso_len, first, second=None, i=None):
    """One person's entry of 'zoom', window (image, wy0, wx0, wh, ww): from row i of second_pass's points, or, not zoomed (second None), the pass-1 values of `first`."""
    e = {'zoomed': second is not None, 'window': tuple(int(v) for v in window[1:]), 'torso_len': float(torso_len)}
    for key in ('pd', 'sm'):
        e[key], e[key + '_inside'] = (first[key], first[key + '_inside']) if second is None else (second[key][0][i], second[key][1][i])
    return e


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
    second = second_pass(engine, batch, wins[keep], cells[keep], batch_size, pad, False, zoom_ms)[0] if len(keep) else {}
    at = {int(i): n for n, i in enumerate(keep)}
    for i, (b, sm_i, inside_i, _) in enumerate(who):
        first = {'pd': res[b]['pd'], 'pd_inside': res[b]['pd_inside'], 'sm': sm_i, 'sm_inside': inside_i}
        res[b]['zoom'].append(zoom_entry(wins[i], t[i], first, second if i in at else None, at.get(i)))


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
