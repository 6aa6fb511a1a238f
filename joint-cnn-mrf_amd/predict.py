"""From images of any size to joints in each image's own pixels: Engine.fit_images letterboxes a ragged batch of byte images
into the 480x720 frame the tower was built for, Engine.forward runs on the bytes -- with use_sm the torso map is inferred (torso='infer',
DESIGN.md 4.15): a photo has no annotation -- and evaluation.fit_to_source maps every coordinate back through the fit.

Black bars and a changed scale are inputs the network was not trained on; how well a FLIC-trained model does on letterboxed photos has not been
measured.  Multi-scale and mirrored evaluation are not offered here: the inferred torso is not defined under them (multiscale.py)."""
import os

import numpy as np
import torch

from .evaluation import fit_to_source, peaks_to_pixels, pose_to_pixels

JOINT_NAMES = ('lsho', 'lelb', 'lwri', 'rsho', 'relb', 'rwri', 'lhip', 'rhip', 'nose')      # main.py:18, without the torso channel
STRIDE = 8                      # heat-map cell -> pixel of the fitted frame (the reference's `coords * 8`, test.py)
FRAME = (480, 720)
IMAGE_EXTENSIONS = ('.npy', '.png', '.jpg', '.jpeg', '.bmp', '.gif', '.tif', '.tiff', '.webp', '.ppm')


def _coords_to_points(coords):
    """int32 [B,2,K] (row, col) cells, device -> host float64 [B,K,2] pixels of the fitted frame; -1 (an empty slot) stays -1."""
    c = coords.cpu().numpy().transpose(0, 2, 1).astype(np.float64)
    return np.where(c < 0, -1.0, c * STRIDE)


def predict_images(engine, images, use_sm=True, peaks=0, decode=False, people=1, batch_size=16, pad=0, timing=None):
    """images: a list of uint8 [h,w,3] arrays or tensors of mixed sizes (what Engine.fit_images takes).  They are fitted and run through
    engine.forward(x_u8, torso='infer' if use_sm else None, use_sm=use_sm, peaks=peaks, decode=decode, people=people) batch_size at a time.
    Returns one dict per image, everything in the image's own pixels (row, col), host numpy:
      'size' (h, w); 'joint_names'; 'geom' (y0, x0, ch, cw, h, w), the fit;
      'pd' float64 [K,2] and 'pd_inside' bool [K] (did the arg-max lie in the content rectangle, not in a bar?);
      with use_sm: 'sm', 'sm_inside', and 'torso_cell' (row, col) of the inferred torso in heat-map cells of the fitted frame;
      with peaks = P: 'pd_peaks' (and 'sm_peaks') float64 [K,P,3] = (row, col, score), filler slots (-1, -1, 0), and '*_peaks_inside' [K,P];
      with decode: 'pose' float64 [K,3] = (row, col, pose score) and 'pose_inside' [K] (people > 1: the pose of slot 0, the arg-max torso);
      with people = M > 1: 'people' = {'count', 'torso_cell' [M,2], 'torso_score' [M], 'sm' [M,K,2], 'sm_inside' [M,K]}, slots from count on -1.
    timing: a dict that receives 'fit_ms' and 'forward_ms', device-event times summed over the batches (the upload of host images is part of
    neither)."""
    if not isinstance(images, (list, tuple)) or len(images) == 0:
        raise ValueError('images must be a non-empty list of uint8 [h,w,3] images')
    if int(batch_size) < 1:
        raise ValueError('batch_size must be >= 1, got %r' % (batch_size,))
    names = list(JOINT_NAMES[:engine.n_joints])
    out = []
    fit_ms = fwd_ms = 0.0
    with torch.cuda.stream(engine._stream):
        for lo in range(0, len(images), int(batch_size)):
            # host images go up first, so that the fit's time is the fit's; anything that is no byte image is left for fit_images to refuse
            batch = [_upload(im, engine.device) for im in images[lo:lo + int(batch_size)]]
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
            ev[0].record(engine._stream)
            x, geom = engine.fit_images(batch, out_hw=FRAME, pad=pad)
            ev[1].record(engine._stream)
            r = engine.forward(x, 'infer' if use_sm else None, use_sm=use_sm, want_prob=False, peaks=peaks, decode=decode, people=people)
            ev[2].record(engine._stream)
            ev[2].synchronize()
            fit_ms += ev[0].elapsed_time(ev[1])
            fwd_ms += ev[1].elapsed_time(ev[2])
            out.extend(_to_source(r, geom, names, use_sm, peaks, decode, people))
    if timing is not None:
        timing.update(fit_ms=fit_ms, forward_ms=fwd_ms)
    return out


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
            'images': [dict({'path': f}, **{k: _listed(v) for k, v in r.items() if k != 'joint_names'}) for f, r in zip(files, results)]}
