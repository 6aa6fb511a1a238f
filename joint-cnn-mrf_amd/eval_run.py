"""The evaluation run of the command line (the reference's main.py:668-675: predictions of the test set -> matlab/predictions.mat) and what the
three runs of main.py share: the data set, the parameters a run starts from, the model name.

run(args) loads the data, builds ONE set of engines, sends the test set through one of four feeds -- each returns a Result -- and hands that
record to the writers: the .mat file of --predictions, the JSON document of --det_curve, the JSON line on stdout.  main.py parses and refuses
flag combinations before anything here runs; nothing in this module looks at a combination main() refuses."""
import functools
import json
import os
import sys
import time
from dataclasses import dataclass

import numpy as np
import torch

from . import multiscale, synth
from .synth import JOINT_NAMES, N_JOINTS

# ------------------------------------------------------------------ data set, session files (main.py:286-299,604-612,666)
DATASET_FILES = ('x_train_flic.npy', 'y_train_flic.npy', 'x_test_flic.npy', 'y_test_flic.npy')     # main.py:290-293, written by data.py


def get_dataset(data_dir='.'):
    """main.py:286-294: the four arrays data.py prepares (x [N,480,720,3] fp32 in [0,1], y [N,60,90,10])."""
    missing = [f for f in DATASET_FILES if not os.path.exists(os.path.join(data_dir, f))]
    if missing:
        raise FileNotFoundError('%s not found in %r: run `python -m joint_cnn_mrf_amd.data` on the FLIC frames first (the reference\'s '
                                'data.py step), or pass --synthetic for generated data' % (', '.join(missing), data_dir))
    return tuple(np.load(os.path.join(data_dir, f), mmap_mode='r') for f in DATASET_FILES)


def get_pairwise_distr(data_dir='.'):
    """main.py:297-299: the pickle prepare_pairwise_distribution.py writes ({'<j>_<c>': [120,180] float64})."""
    import pickle
    with open(os.path.join(data_dir, 'pairwise_distribution.pickle'), 'rb') as handle:
        return pickle.load(handle)


def _synthetic_dataset(n_train, n_test):
    return (synth.make_images(n_train, seed=100), synth.make_targets(n_train, seed=200),
            synth.make_images(n_test, seed=300), synth.make_targets(n_test, seed=400))


def byte_grid(x):
    """--synthetic --u8_images: generated float images put on the byte grid, byte k = floor(x * 256) (255 at x = 1) standing for k / 255."""
    return np.minimum(np.floor(np.asarray(x, np.float32) * np.float32(256)), np.float32(255)).astype(np.uint8)


def people_split(n):
    """--synth_people: the first 80 % of n poses, in file order, are the training poses and the last 20 % the test poses -> (train, test) indices."""
    return np.arange(n * 4 // 5), np.arange(n * 4 // 5, n)


@functools.lru_cache(maxsize=8)
def poses_problem(path):
    """None if `path` holds what --synth_people takes (an [N,2,9] float64 array with at least five poses, finite), else what is wrong with it."""
    try:
        a = np.load(path, mmap_mode='r')
    except Exception as e:      # a missing or unreadable file is refused like a wrong one
        return 'cannot be read (%s)' % e
    if a.ndim != 3 or a.shape[1:] != (2, 9) or a.dtype != np.float64 or a.shape[0] < 5:
        return 'holds %s %s' % (a.dtype, tuple(a.shape))
    return None if np.isfinite(a).all() else 'holds values that are not finite'


def people_seed(args, epoch):
    """The generator seed of a rendered set: the test set is epoch 0, the training set of epoch e (the first one: 1) is seed + 2 + e."""
    return int(args.seed) + 2 + int(epoch)


def _people_dataset(args, extra):
    """--synth_people: rendered people in the poses of the file, the sets rendered on the first device of --gpus and downloaded."""
    from . import dataset, priors
    from .engine import Engine
    poses = np.asarray(np.load(args.synth_people), np.float64)
    tr, te = people_split(poses.shape[0])
    cap = args.synthetic_size if getattr(args, 'synthetic_size_given', False) else None      # not given: every training pose
    if args.train:
        tr = tr[:cap] if cap is not None else tr
    else:      # an evaluation run reads a batch of the training set, for the summaries
        tr = tr[:args.batch_size]
    kind = 'uint8' if args.u8_images and not (args.multiscale and not args.train) else 'float32'
    eng = Engine(device=args.gpus[0])
    try:
        x_train, y_train, c_train = dataset.render_people(eng, poses, tr, people_seed(args, 1), image_dtype=kind)
        x_test, y_test, c_test = dataset.render_people(eng, poses, te, people_seed(args, 0), image_dtype=kind)
        if getattr(args, 'synth_dump', None):      # the scenes are drawn one after the other: the first 16 of the set are the first 16 of its generator
            xy = synth.people_batch(np.random.RandomState(people_seed(args, 0)), poses, te[:16])[2]
            dump_people(eng, x_test[:16], xy, args.synth_dump)
    finally:
        eng.close()
    if extra is not None:
        extra.update(poses=poses, train_idx=tr, test_idx=te, cells_train=c_train, cells_test=c_test)
    return x_train, y_train, x_test, y_test, priors.build_pairwise_distributions(c_train)


def dump_people(eng, x, xy, out_dir):
    """--synth_dump: the images x (uint8, or float32 on the byte grid) as DIR/<index:05d>.png with a white disc of 3 pixels on every annotated joint
    xy [n,2,9] (x, y), to the sixteenth of a pixel, drawn by Engine.render_poses.  A way to look, not a measurement."""
    from .summary import encode_png
    x = np.asarray(x)
    x = x if x.dtype == np.uint8 else np.rint(x * np.float32(255)).astype(np.uint8)
    at = np.rint(np.asarray(xy, np.float64) * 16).astype(np.int64)
    prims = [(i, at[i, 1, k], at[i, 0, k], at[i, 1, k], at[i, 0, k], 16 * 3, 0xFFFFFF, 255) for i in range(x.shape[0]) for k in range(N_JOINTS)]
    pictures = eng.render_poses([im for im in x], np.array(prims, np.int32).reshape(-1, 8))
    os.makedirs(out_dir, exist_ok=True)
    for i, pic in enumerate(pictures):
        with open(os.path.join(out_dir, '%05d.png' % i), 'wb') as fh:
            fh.write(encode_png(pic.cpu().numpy()))


def load_data(args, extra=None):
    """x_train, y_train, x_test, y_test, pairwise: the FLIC files of --data_dir, or with --synthetic generated priors and sets (--train: --synthetic_size
    examples to train on and half as many, at least a batch, to test; an evaluation run: that many to test and a batch for the summaries), or with
    --synth_people rendered people (extra: a dict that receives the poses, the two index sets and the joint cells of the two sets)."""
    if getattr(args, 'synth_people', None):
        return _people_dataset(args, extra)
    if not args.synthetic:
        return get_dataset(args.data_dir) + (get_pairwise_distr(args.data_dir),)
    sizes = (args.synthetic_size, max(args.batch_size, args.synthetic_size // 2)) if args.train else (args.batch_size, args.synthetic_size)
    return _synthetic_dataset(*sizes) + (synth.synthetic_priors(),)


def initial_params(args, pairwise_distr):
    """tf.global_variables_initializer on the graph of main.py:474-487: He-initialised convolutions, identity BatchNorm,
    energies = the pairwise distributions, biases = 1e-5."""
    params = synth.make_pd_params(debug=args.debug)
    if args.use_sm:
        params.update(synth.make_sm_params(pairwise_distr, kind='init'))
    return params


def run_params(args, pairwise):
    """What a run starts from -> (params, state).  Without --restore: initial_params and None.  With it, saver.restore (main.py:612):
    --restore_path is a tf.train.Saver checkpoint prefix (P.index + P.data-00000-of-00001, read by tf_checkpoint.py) or an .npz keyed by the same
    variable names; state is every saved variable, optimizer slots included, params the validated model variables among them."""
    if not args.restore:
        return initial_params(args, pairwise), None
    from . import checkpoint, tf_checkpoint
    if args.restore_path.endswith('.npz'):
        with np.load(args.restore_path) as z:
            state = {k: z[k] for k in z.files}
    else:
        state = tf_checkpoint.load_checkpoint(args.restore_path)
    params = {k: v for k, v in state.items() if k in checkpoint.expected_shapes(args.debug, args.use_sm)}
    checkpoint.validate(params, args.debug, args.use_sm)
    return params, state


def model_name(args):
    """main.py:447."""
    return '{}_lr={}_lambda={}_bs={}'.format(time.strftime('%Y-%m-%d %H:%M:%S'), args.lr, args.lmbd, args.batch_size)


# ------------------------------------------------------------------ judging assembled predictions
DET_CURVE_CHUNK = 256      # images per upload of det_curves_of_predictions / pose_det_rate


def evaluated_indices(n_images, batch_size, n_towers, multiscale=False):
    """Which test image each column of the assembled predictions belongs to.  The multi-scale run evaluates every image in order.  The single-scale
    run walks whole batches only (the remainder n_images % batch_size is dropped) and gives tower i the slice [i * per, i * per + per) of every batch,
    per = batch_size // n_towers (dist.shard_bounds, main.py:511,516): the remainder batch_size % n_towers of EVERY batch is dropped too, so with
    --batch_size 14 on four towers column 12 is image 14, not image 12."""
    if multiscale:
        return np.arange(n_images, dtype=np.int64)
    per = batch_size // n_towers
    first = np.arange(0, (n_images // batch_size) * batch_size, batch_size, dtype=np.int64)
    return (first[:, None] + np.arange(n_towers * per, dtype=np.int64)[None, :]).reshape(-1)


def _chunks(eng, preds, y, index):
    """The predictions preds (each int [2,K,N]) and their targets y[index], DET_CURVE_CHUNK images at a time, on `eng`'s device:
    yields ([coords int32 [n,2,K] per entry of preds], y [n,...] fp32)."""
    N = int(preds[0].shape[2])
    for lo in range(0, N, DET_CURVE_CHUNK):
        hi = min(N, lo + DET_CURVE_CHUNK)
        yb = torch.as_tensor(np.ascontiguousarray(y[index[lo:hi]], dtype=np.float32), device=eng.device)
        yield [torch.as_tensor(np.ascontiguousarray(np.asarray(p)[:, :, lo:hi].transpose(2, 0, 1), dtype=np.int32), device=eng.device) for p in preds], yb


def det_curves_of_predictions(eng, pred_pd, pred_sm, y, radii=range(1, 21), index=None):
    """Detection-rate curves of assembled predictions: pred_* int [2,K,N] (row, col) as get_predictions returns them, y [.,60,90,>= K] targets;
    column i is judged against y[index[i]] (index None: y[i]; evaluated_indices gives the index of an evaluation run).  Uploaded in chunks of
    DET_CURVE_CHUNK images, counted on `eng`'s device, read back once.  Returns (DetCurve of the part detector, DetCurve of the spatial model)."""
    from .evaluation import DetCurve
    K, N = int(pred_pd.shape[1]), int(pred_pd.shape[2])
    index = np.arange(N, dtype=np.int64) if index is None else np.asarray(index, dtype=np.int64)
    if index.shape != (N,) or (N and (index.min() < 0 or index.max() >= len(y))):
        raise ValueError('%d predictions need %d target indices inside [0, %d); got %s' % (N, N, len(y), index.shape))
    curves = DetCurve(eng, radii, n_joints=K), DetCurve(eng, radii, n_joints=K)
    for coords, yb in _chunks(eng, (pred_pd, pred_sm), y, index):
        for curve, c in zip(curves, coords):
            curve.update(c, yb)
    return curves


def pose_det_rate(eng, pred_pose, y, index, joints=(2,), det_radius=10):
    """The reference's test_dr figure (evaluation.py:26-37: left wrist, radius 10) of decoded poses: pred_pose int [2,K,N] (row, col), column i judged
    against y[index[i]], through evaluation.det_rate_from_coords in chunks of DET_CURVE_CHUNK images on `eng`'s device.  An image without a pose
    (coordinates -1) is a miss wherever -1 is far from the target."""
    from .evaluation import det_rate_from_coords
    K, N = int(pred_pose.shape[1]), int(pred_pose.shape[2])
    acc = 0.0
    for (coords,), yb in _chunks(eng, (pred_pose,), y, index):
        acc += float(det_rate_from_coords(coords, eng.argmax_coords(yb[..., :K].contiguous()), det_radius, list(joints))) * coords.shape[0]
    return acc / N


# ------------------------------------------------------------------ the four feeds
@dataclass
class Result:
    """What a feed assembled over the evaluated images, in the order evaluated_indices names."""
    pred_pd: np.ndarray             # int [2,K,N] (row, col) stacked on the last axis, main.py:425
    pred_sm: np.ndarray             # (the part detector's without --use_sm, main.py:535)
    peaks_pd: dict = None           # --peaks: the dicts of Engine.hm_peaks, device tensors [N,K,P,...]
    peaks_sm: dict = None
    pose: dict = None               # --decode_pose: the dict of Engine.pose_decode, host arrays
    torso_cells: np.ndarray = None  # --infer_torso: int32 [N,2] (row, col)
    people: dict = None             # --people M > 1: 'sm_coords' [N,M,2,K] (-1 from 'count' on) and 'count' [N], host arrays
    fed: dict = None                # --u8_images: what the single-scale run moved to the devices


def _stack(coords):
    return torch.cat(coords).permute(1, 2, 0).cpu().numpy()


def _collect(parts):
    return {f: torch.cat([p[f] for p in parts]) for f in parts[0]}


def feed_multiscale(args, towers, x_test, y_test):
    """--multiscale: the 8-scale wrapper (get_predictions, main.py:382-425; main.py:674) on the first tower, every image in order."""
    return Result(*multiscale.get_predictions(towers.engines[0], np.asarray(x_test), np.asarray(y_test), use_sm=args.use_sm, peaks=args.peaks,
                                              flip_test=args.flip_test))


def feed_towers(args, towers, x_test, y_test):
    """Single scale, float batches sharded over the towers: the feed that knows --peaks, --decode_pose, --flip_test, --infer_torso and --people."""
    B, sm = args.batch_size, 'sm' if args.use_sm else 'pd'
    rs = []
    for lo in range(0, (x_test.shape[0] // B) * B, B):
        r = towers.forward(np.ascontiguousarray(x_test[lo:lo + B], np.float32),
                           'infer' if args.infer_torso else np.ascontiguousarray(y_test[lo:lo + B, :, :, N_JOINTS:], np.float32),
                           use_sm=args.use_sm, peaks=args.peaks, decode=args.decode_pose, flip_test=args.flip_test, people=args.people)
        if args.decode_pose and args.people > 1:      # the file holds one pose per image: slot 0, the arg-max torso
            r['pose'] = {f: v[:, 0].contiguous() for f, v in r['pose'].items()}
        rs.append({k: v for k, v in r.items() if k != 'torso'})      # (the inferred torso maps are not kept)
    res = Result(_stack([r['pd_coords'] for r in rs]), _stack([r[sm + '_coords'] for r in rs]))
    if args.peaks:
        res.peaks_pd, res.peaks_sm = _collect([r['pd_peaks'] for r in rs]), _collect([r[sm + '_peaks'] for r in rs])
    if args.decode_pose:
        res.pose = {f: v.cpu().numpy() for f, v in _collect([r['pose'] for r in rs]).items()}
    if args.infer_torso:
        res.torso_cells = torch.cat([r['torso_cell'] for r in rs]).cpu().numpy()
        if args.people > 1:
            res.people = {f: torch.cat([r['people'][f] for r in rs]).cpu().numpy() for f in ('sm_coords', 'count')}
    return res


def feed_stream_u8(args, towers, x_test, y_test):
    """--u8_images: the test images as bytes (converted once, the round trip checked), streamed from pinned memory, one
    stream.ForwardStream per tower."""
    from .dataset import to_u8_exact
    from .stream import ForwardStream
    B, sm = args.batch_size, 'sm_coords' if args.use_sm else 'pd_coords'
    xb = to_u8_exact(x_test)      # (works through a memory-mapped file in slices; float64 or other data is refused)
    tb = np.ascontiguousarray(y_test[:, :, :, N_JOINTS:], np.float32)
    fss = [ForwardStream(e, use_sm=args.use_sm) for e in towers.engines]

    def feed(lo, hi):      # one tower's slice of every whole batch (Towers.slices: the remainder B % n_gpus is dropped)
        for b0 in range(0, (xb.shape[0] // B) * B, B):
            yield xb[b0 + lo:b0 + hi], tb[b0 + lo:b0 + hi]
    pd, sm_ = [], []
    for parts in zip(*[fs.run(feed(lo, hi)) for fs, (lo, hi) in zip(fss, towers.slices(B))]):
        pd.append(torch.from_numpy(np.concatenate([p['pd_coords'] for p in parts])))
        sm_.append(torch.from_numpy(np.concatenate([p[sm] for p in parts])))
    return Result(_stack(pd), _stack(sm_), fed={'image_dtype': 'uint8', 'bytes_uploaded': int(sum(fs.bytes_uploaded for fs in fss))})


def feed_towers_u8_flip(args, towers, x_test, y_test):
    """--u8_images --flip_test: byte batches through the towers' byte forward (the streamed feed has no mirrored evaluation)."""
    from .dataset import to_u8_exact
    B, sm = args.batch_size, 'sm_coords' if args.use_sm else 'pd_coords'
    xb = to_u8_exact(x_test)
    pd, sm_, n_moved = [], [], 0
    for lo in range(0, (xb.shape[0] // B) * B, B):
        bx, bt = np.ascontiguousarray(xb[lo:lo + B]), np.ascontiguousarray(y_test[lo:lo + B, :, :, N_JOINTS:], np.float32)
        r = towers.forward(bx, bt, use_sm=args.use_sm, flip_test=True)
        pd.append(r['pd_coords'])
        sm_.append(r[sm])
        for a, b in towers.slices(B):      # what the towers took of the batch
            n_moved += bx[a:b].nbytes + (bt[a:b].nbytes if args.use_sm else 0)
    return Result(_stack(pd), _stack(sm_), fed={'image_dtype': 'uint8', 'bytes_uploaded': int(n_moved)})


# ------------------------------------------------------------------ what a run writes
def write_predictions(args, res):
    """--predictions: flic_pred_pd / flic_pred_sm (main.py:675) and what the modes add, to a .mat file."""
    import scipy.io
    os.makedirs(os.path.dirname(args.predictions) or '.', exist_ok=True)
    mat = {'flic_pred_pd': res.pred_pd, 'flic_pred_sm': res.pred_sm}
    if args.peaks:
        from .evaluation import peaks_to_pixels
        mat.update(flic_peaks_pd=peaks_to_pixels(res.peaks_pd), flic_peaks_sm=peaks_to_pixels(res.peaks_sm))
    if res.pose is not None:
        mat.update(flic_pred_pose=res.pose['coords'].transpose(1, 2, 0), flic_pose_score=np.stack([res.pose['score'], res.pose['score0']], axis=1))
    if res.torso_cells is not None:
        mat.update(flic_torso_cell=res.torso_cells)
    if res.people is not None:
        mat.update(flic_people_sm=res.people['sm_coords'], flic_people_count=res.people['count'])
    scipy.io.savemat(args.predictions, mat)


def write_det_curve(args, eng, res, y_test):
    """--det_curve, one place for every feed: the curves of the assembled predictions, counted on `eng`'s device, as a JSON document, and the
    reference's test_dr line (main.py:424: left wrist, radius 10)."""
    index = evaluated_indices(len(y_test), args.batch_size, len(args.gpus), multiscale=args.multiscale)      # towers drop batch_size % n_gpus of every batch
    c_pd, c_sm = det_curves_of_predictions(eng, res.pred_pd, res.pred_sm, y_test, index=index)
    names = [str(n) for n in JOINT_NAMES[:res.pred_pd.shape[1]]]
    d_pd, d_sm = c_pd.as_dict(names), c_sm.as_dict(names)
    doc = {'radii': d_pd['radii'], 'joint_names': names, 'n_images': d_pd['n_images'], 'multiscale': bool(args.multiscale), 'use_sm': bool(args.use_sm),
           'pd': {n: d_pd[n] for n in names}, 'sm': {n: d_sm[n] for n in names}}
    os.makedirs(os.path.dirname(args.det_curve) or '.', exist_ok=True)
    with open(args.det_curve, 'w') as fh:
        json.dump(doc, fh)
    print('test_dr: {} {}'.format(c_pd.rate(2, 10), c_sm.rate(2, 10)))


def write_scale_curve(args, eng, x_test, y_test, cells=None):
    """--eval_scale S [S ...] --scale_curve PATH: the test set through evaluation.eval_curves_affine on `eng` -- every image, the last
    batch partial, at each scale S about the centre with the antialiased sample -- as a JSON document: the curves per scale in the shape --det_curve
    gives a curve, and how many images each scale counted (those none of whose joints left the frame).  cells: the joint cells of the set where the
    run has them (--synth_people); else the arg-max cells of y_test, taken on the device batch by batch."""
    from .evaluation import eval_curves_affine
    B = args.batch_size
    if cells is None:
        cells = np.concatenate([eng.joint_cells(torch.as_tensor(np.ascontiguousarray(y_test[lo:lo + B], np.float32), device=eng.device)).cpu().numpy()
                                for lo in range(0, len(y_test), B)])
    scales = [float(s) for s in args.eval_scale]
    curves = eval_curves_affine(x_test, cells, eng, B, scales, use_sm=args.use_sm, antialias=True)
    names = [str(n) for n in JOINT_NAMES[:eng.n_joints]]
    per = lambda c: {n: v for n, v in c.as_dict(names).items() if n in names} if c.n_images else None      # (no image counted: no rates)
    doc = {'scales': scales, 'counted': [int(curves[s][0].n_images) for s in scales], 'pd': {str(s): per(curves[s][0]) for s in scales},
           'sm': {str(s): per(curves[s][1]) for s in scales}, 'antialias': True, 'radii': [float(r) for r in curves[scales[0]][0].radii],
           'joint_names': names, 'n_images': int(len(x_test)), 'use_sm': bool(args.use_sm)}
    os.makedirs(os.path.dirname(args.scale_curve) or '.', exist_ok=True)
    with open(args.scale_curve, 'w') as fh:
        json.dump(doc, fh)


def summary_line(args, res, dt, y_test):
    """The JSON line a run ends with."""
    n = int(res.pred_pd.shape[2])
    line = {'n_images': n, 'gpus': args.gpus, 'use_sm': bool(args.use_sm), 'debug': bool(args.debug), 'multiscale': bool(args.multiscale),
            'seconds': dt, 'images_per_sec': n / dt, 'coords_image0_pd': res.pred_pd[:, :, 0].tolist()}
    if res.fed is not None:
        line.update(res.fed)
    if args.flip_test:
        line['flip_test'] = True
    if getattr(args, 'eval_scale', None):
        line['eval_scale'] = [float(s) for s in args.eval_scale]
    if res.torso_cells is not None:      # how far the inferred cell lies from the arg-max of the annotated torso channel (first occurrence), in cells
        index = evaluated_indices(len(y_test), args.batch_size, len(args.gpus))
        ann = np.asarray(y_test)[index][:, :, :, N_JOINTS].reshape(len(index), -1).argmax(axis=1)
        got = res.torso_cells.astype(np.float64)
        line['infer_torso'] = True
        line['torso_cell_dist'] = float(np.sqrt((got[:, 0] - ann // 90) ** 2 + (got[:, 1] - ann % 90) ** 2).mean())
        if args.people > 1:
            line['people'] = int(args.people)
    if args.peaks:
        line['peaks'] = int(args.peaks)
    if res.pose is not None:      # the share of images whose decoded pose is not the all-peak-0 pose (the independent arg-maxes)
        line['pose_changed'] = float((res.pose['index'] != 0).any(axis=1).mean())
    print(json.dumps(line))


def step0_summaries(args, eng, params, train, test):
    """--tb_dir (main.py:668-673): the step-0 summaries of an evaluation run, without the gradient parts."""
    from . import summary
    from .main import tb_batch, tb_open, tb_summaries      # the writers of the training loop; resolved at call time, main imports this module
    tb = tb_open(args, model_name(args))
    flat, layout = summary.flat_params(eng, params)
    tb_summaries(tb, eng, layout, {'train': tb_batch(*train, args.batch_size), 'test': tb_batch(*test, args.batch_size)},
                 args.use_sm, 0, params_flat=flat, activations=args.tb_activations, n_towers=len(args.gpus))
    for w in tb.values():
        w.close()


def run(args):
    """The evaluation run (main.py:668-675): predictions of the test set, single scale sharded over the towers of --gpus or --multiscale on the
    first of them."""
    from .dist import Towers
    people = {}      # --synth_people: the joint cells of the rendered sets, which --eval_scale transforms
    x_train, y_train, x_test, y_test, pairwise = load_data(args, people)
    if args.synthetic and args.u8_images and not args.multiscale:
        x_test = byte_grid(x_test)
    params, _ = run_params(args, pairwise)
    t0 = time.time()
    if args.multiscale and args.u8_images:
        print('--u8_images: the multi-scale wrapper resizes float windows and is unchanged; the images stay float32', file=sys.stderr)
    if args.multiscale and len(args.gpus) > 1:
        print('--multiscale evaluates on device %d only; the other --gpus entries are not used' % args.gpus[0], file=sys.stderr)
    # one set of engines only (each fp32 engine caches multi-GB filter spectra): one tower per listed device for the single-scale run, one
    # tower for the multi-scale wrapper, which runs on one device
    towers = Towers(params, args.gpus[:1] if args.multiscale else args.gpus, precision=args.precision)
    eng = towers.engines[0]
    if args.tb_dir:
        step0_summaries(args, eng, params, (x_train, y_train), (x_test, y_test))
    feed = (feed_multiscale if args.multiscale else feed_towers_u8_flip if args.u8_images and args.flip_test
            else feed_stream_u8 if args.u8_images else feed_towers)
    res = feed(args, towers, x_test, y_test)
    torch.cuda.synchronize()
    dt = time.time() - t0
    if args.predictions:
        write_predictions(args, res)
    if args.det_curve:
        write_det_curve(args, eng, res, y_test)
    if res.pose is not None:
        index = evaluated_indices(len(y_test), args.batch_size, len(args.gpus))
        print('test_dr_pose: {}'.format(pose_det_rate(eng, res.pose['coords'].transpose(1, 2, 0), y_test, index)))
    if args.eval_scale:      # after the clock has stopped and the run's own outputs are written: they are what they are without the flags
        write_scale_curve(args, eng, x_test, y_test, people.get('cells_test'))
    summary_line(args, res, dt, y_test)
    towers.close()
