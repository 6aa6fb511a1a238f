"""The files of the command line (main.py --predict): which paths are images, how one is read, and the JSON document of the results."""
import os

import numpy as np

from .images import FRAME, STRIDE

IMAGE_EXTENSIONS = ('.npy', '.png', '.jpg', '.jpeg', '.bmp', '.gif', '.tif', '.tiff', '.webp', '.ppm')


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
