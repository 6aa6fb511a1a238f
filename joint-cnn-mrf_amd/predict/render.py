"""Pictures of the result: skeleton_primitives turns results into capsules, render_images draws them -- and, with keep_maps,
the heat maps under them -- onto the images at their own size through Engine.render_poses."""
import numpy as np
import torch

from .images import STRIDE, DeviceTimer, _upload

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
    if which in ('track', 'track_zoom', 'track_pose'):
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
    if which not in ('sm', 'pd', 'track', 'track_zoom', 'track_pose'):      # 'track_pose': the clip decode of predict_sequence(pose=P), DESIGN.md 4.30
        raise ValueError("which must be 'sm', 'pd', 'track', 'track_zoom' or 'track_pose', got %r" % (which,))
    rows = []
    for i, r in enumerate(results):
        if which not in r:
            raise ValueError("results[%d] has no %r joints (%s makes them)" % (i, which, {'track': 'predict_sequence', 'track_zoom': 'predict_sequence_zoom', 'track_pose': 'predict_sequence(pose=P)'}.get(which, 'predict_images(use_sm=%s)' % (which == 'sm'))))
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
    out, ms = [], [0.0]
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
            timer = DeviceTimer(engine)
            drawn = engine.render_poses(batch, skeleton_primitives(res, which, zoom), **kw)
            timer.mark()
            out.extend(d.cpu().numpy() for d in drawn)
            timer.add(ms, 0)
    if timing is not None:
        timing.update(render_ms=ms[0])
    return out
