"""Host-side mirror of the reference's main.py for the joint-heat-map inference path.

Same function names, argument order and NHWC layouts as /root/reference/main.py, so a
caller of `model`, `conv_mrf`, `spatial_model`, `spatial_softmax` (graph at main.py:522-531)
switches by importing this module; tensors are torch-ROCm instead of tf.Tensor, and the
arithmetic runs in libjcm's HIP kernels (no TensorFlow, no CPU fallback).

Where the reference reads module globals (`hps`, `flag_train`, `pairwise_energies`,
`pairwise_biases`, `joint_names`, `joint_dependence`, `n_joints`, `hm_height`, `hm_width`)
this module keeps the same names; they are filled by `configure()` instead of at import
(the reference parses argv and loads `.npy` files at import time, main.py:440,459).

CLI (the reference's flags, main.py:428-439): `python -m joint_cnn_mrf_amd.main --gpus 0 1 --use_sm --batch_size 64`
evaluates the test split (single scale sharded over the listed devices, or `--multiscale`); `--train` runs the
reference's epoch loop (main.py:620-667) with one tower per device, eval_error after every epoch and tf.train.Saver
checkpoints; `--restore --restore_path P` resumes from one.  Data: the .npy files data.py prepares, or `--synthetic`.
"""
import argparse
import json
import os
import time

import numpy as np
import torch

from . import eval_run, multiscale, synth
from .engine import Engine
from .eval_run import (_synthetic_dataset, byte_grid, people_seed, poses_problem, det_curves_of_predictions, evaluated_indices, get_dataset, get_pairwise_distr,  # noqa: F401
                       initial_params, load_data, model_name, run_params)

# main.py:18-26
joint_names = np.array(['lsho', 'lelb', 'lwri', 'rsho', 'relb', 'rwri', 'lhip', 'rhip', 'nose', 'torso'])
joint_dependence = {}
for _joint in joint_names:
    joint_dependence[_joint] = [_c for _c in joint_names if _c != _joint]

n_joints = 9                      # main.py:458
in_height, in_width = 480, 720    # data.py:119
hm_height, hm_width = 60, 90      # data.py:180
flag_train = False                # inference only: BatchNorm uses moving statistics (main.py:406)

hps = argparse.Namespace(debug=False, train=False, gpus=[0], restore=False, use_sm=True, data_augm=False,
                         batch_size=14,            # defaults of main.py:428-439
                         render=None, render_heat=None)
pairwise_energies, pairwise_biases = {}, {}        # '<j>_<c>' -> tensor, main.py:478-487
_engine = None


class _StoreGiven(argparse.Action):
    """store, and note in <dest>_given that the flag was on the command line (its default stays what it was)."""

    def __call__(self, parser, namespace, values, option_string=None):
        setattr(namespace, self.dest, values)
        setattr(namespace, self.dest + '_given', True)


def build_parser():
    """The reference's eleven flags (main.py:428-439), same names, types and defaults (but --gpus, whose reference default
    [6] names a device of the authors' server), plus what the reference hard-codes in module globals: where the data and
    the checkpoints live, and an explicit switch for generated data."""
    parser = argparse.ArgumentParser(description='Define hyperparameters.')
    parser.add_argument('--debug', action='store_true', help='True if we want to debug.')
    parser.add_argument('--train', action='store_true', help='True if we want to train the model.')
    parser.add_argument('--gpus', nargs='+', type=int, default=[0], help='GPU indices.')
    parser.add_argument('--restore', action='store_true', help='True if we want to restore the model.')
    parser.add_argument('--use_sm', action='store_true', help='True if we want to use the Spatial Model.')
    parser.add_argument('--data_augm', action='store_true', help='True if we want to use data augmentation.')
    parser.add_argument('--n_epochs', type=int, default=30, help='Number of epochs.')
    parser.add_argument('--batch_size', type=int, default=14, help='Batch size.')
    parser.add_argument('--optimizer', type=str, default='adam', help='momentum or adam')
    parser.add_argument('--lr', type=float, default=0.001, help='Learning rate.')
    parser.add_argument('--lmbd', type=float, default=0.001, help='Regularization coefficient.')
    # not in the reference (module globals / hard-coded paths there)
    parser.add_argument('--data_dir', default='.', help='directory of x_*_flic.npy, y_*_flic.npy, pairwise_distribution.pickle (main.py:290-298).')
    parser.add_argument('--synthetic', action='store_true', help='generated images / targets / priors instead of the FLIC files.')
    parser.add_argument('--synthetic_size', type=int, default=56, action=_StoreGiven, help='number of generated training examples with --synthetic; with '
                        '--synth_people the most training poses that are rendered (there the default is all of them: synthetic_size_given tells).')
    parser.set_defaults(synthetic_size_given=False)
    parser.add_argument('--synth_people', default=None, metavar='POSES.npy', help='instead of the FLIC files: rendered people (DESIGN.md 4.22) in the poses of '
                        'this [N,2,9] float64 annotation array (data.py\'s xy), drawn on the device by Engine.synth_people -- the first 80 %% of the poses, in file '
                        'order, are the training set and the last 20 %% the test set; bytes under --u8_images, floats otherwise; the priors are those of the '
                        'training cells.  Figures, not photographs: nothing measured on them is a FLIC number.')
    parser.add_argument('--synth_fresh', action='store_true', help='with --train --device_data --u8_images --synth_people: draw the training set again, in place on '
                        'the device, at the start of every epoch after the first (DeviceDataset.rerender_people, RandomState(seed + 2 + epoch)): the same poses, '
                        'new scenes.  The batches are those of a run without it.')
    parser.add_argument('--synth_dump', default=None, metavar='DIR', help='with --synth_people: write the first 16 test images to DIR as PNG files with the annotated '
                        'joints marked at their annotated positions (Engine.render_poses).  A way to look, not a measurement.')
    parser.add_argument('--model_path', default=model_path, help='checkpoint directory (main.py:444).')
    parser.add_argument('--restore_path', default=None, help='checkpoint prefix (tf.train.Saver files) or .npz for --restore (main.py:443,612).')
    parser.add_argument('--precision', default='fp32', choices=['fp32', 'bf16'], help='arithmetic of the kernels.')
    parser.add_argument('--multiscale', action='store_true', help='evaluation run: 8-scale test-time evaluation (get_predictions, main.py:382-425).')
    parser.add_argument('--predictions', default=None, help='evaluation run: write flic_pred_pd / flic_pred_sm to this .mat file (main.py:675).')
    parser.add_argument('--det_curve', default=None, metavar='PATH', help='evaluation run: write the detection-rate curves of the predictions (every joint, radii '
                        '1..20 %% of the torso length, part detector and spatial model) to this JSON file and print the reference\'s test_dr line '
                        '(main.py:424; DESIGN.md 4.11).')
    parser.add_argument('--eval_scale', type=float, nargs='+', default=None, metavar='S', help='single-scale evaluation run, with --scale_curve: after the run\'s own '
                        'outputs, show the tower the whole test set at every person scale S in [0.25, 4] -- one antialiased affine sample about the centre, the '
                        'targets redrawn at the moved joints (evaluation.eval_curves_affine, DESIGN.md 4.27) -- and write one detection-rate curve per scale; an '
                        'image a joint of which leaves the frame is not counted at that scale.')
    parser.add_argument('--scale_curve', default=None, metavar='PATH', help='with --eval_scale: the JSON file the curves per scale go to.')
    parser.add_argument('--peaks', type=int, default=0, metavar='P', help='evaluation run with --predictions: also write flic_peaks_pd / flic_peaks_sm, [N,K,P,3] = '
                        '(row, col, score) in image pixels of the P highest local maxima of every heat map, refined by a quarter cell towards the higher '
                        'neighbour (evaluation.peaks_to_pixels; DESIGN.md 4.12).  1..8; 0 = off.')
    parser.add_argument('--decode_pose', action='store_true', help='evaluation run with --use_sm, --predictions and --peaks P <= 4: of the P peaks per joint of the '
                        'part detector, choose the ONE combination with the highest spatial-model energy (Engine.pose_decode; DESIGN.md 4.13); writes flic_pred_pose '
                        '/ flic_pose_score and prints test_dr_pose.')
    parser.add_argument('--infer_torso', action='store_true', help='single-scale evaluation run with --use_sm: the spatial model is fed the torso map INFERRED from the '
                        'part detector (Engine.forward(torso=\'infer\'), DESIGN.md 4.15) instead of the annotated channel y[..., 9]; the JSON line gains '
                        'infer_torso and torso_cell_dist (mean distance in cells to the arg-max of the annotated torso channel), --predictions gains flic_torso_cell.')
    parser.add_argument('--people', type=int, default=1, metavar='M', help='with --infer_torso: one spatial-model result per torso candidate, up to M in 1..4 per image '
                        '(Engine.forward(people=M)); --predictions gains flic_people_sm [N,M,2,K] and flic_people_count.')
    parser.add_argument('--flip_test', action='store_true', help='evaluation run: mirrored test-time evaluation -- every image goes through the tower in both '
                        'orientations and the maps of the mirror image, read back with the left/right joints exchanged, are averaged with the plain ones '
                        '(Engine.forward(flip_test=True); with --multiscale on top of the 8 scales, 16 copies per image; DESIGN.md 4.14).')
    parser.add_argument('--predict', nargs='+', default=None, metavar='PATH', help='instead of the evaluation run: image files of ANY size (or directories, expanded in '
                        'sorted order) -> the nine joints in each image\'s own pixels, written as JSON to the file of --predictions (predict.predict_images, DESIGN.md '
                        '4.16): the images are letterboxed into 480x720 on the device, with --use_sm the torso is inferred; --peaks, --decode_pose, --people and '
                        '--batch_size apply.  .npy files holding uint8 [h,w,3] are always read; other formats need PIL.  Runs on the first device of --gpus.')
    parser.add_argument('--zoom', action='store_true', help='with --predict and --use_sm: a second pass -- a window around every person of the first pass, sized so '
                        'that the torso has the length FLIC torsos have in a 480-row frame, is fitted and run through the tower again (DESIGN.md 4.17); every '
                        'image of the document gains "zoom", one entry per person.  What it buys with FLIC-trained weights has not been measured.')
    parser.add_argument('--render', default=None, metavar='DIR', help='with --predict: draw the predicted skeleton on every input, on the device at the input\'s '
                        'own size (Engine.render_poses, DESIGN.md 4.18), and write DIR/<index:05d>_<basename>.png, one per input; the spatial model\'s '
                        'joints with --use_sm (a zoomed person\'s from the second pass), the part detector\'s otherwise.  The JSON line gains render_ms.')
    parser.add_argument('--render_heat', default=None, choices=['pd', 'sm'], help='with --render: tint the images with the heat maps of the part detector (pd) or '
                        'of the spatial model (sm, needs --use_sm) under the skeleton, every joint in the colour the reference\'s overlays give it.')
    parser.add_argument('--sequence', default=None, choices=['filter', 'viterbi', 'marginal', 'lag'], help='with --predict: the expanded paths, in their sorted order, are the frames '
                        'of ONE clip (all of one size); every image of the document gains "track", one position per joint that is consistent over the clip '
                        '(predict.predict_sequence, DESIGN.md 4.19): filter = the causal forward filter, viterbi = the most probable track, marginal = the arg-max of every frame\'s '
                        'smoothed posterior given all frames, with its confidence (DESIGN.md 4.23; not with --seq_people), lag = that posterior given the next --seq_lag L frames only, '
                        'what an online caller can have L frames late (DESIGN.md 4.25; not with --seq_people or --seq_zoom).  With --render the tracked '
                        'skeleton is drawn.  What tracking buys has been measured on rendered clips only (DESIGN.md 4.23).')
    parser.add_argument('--seq_sigma', type=float, nargs='+', default=None, metavar='CELLS', help='with --sequence: the standard deviation of a joint\'s motion per '
                        'frame in heat-map cells, one value or one per joint (default 1.5, an untuned placeholder), for filter, viterbi and marginal alike; --seq_fit starts from it.')
    parser.add_argument('--seq_rho', type=float, default=None, metavar='RHO', help='with --sequence: the mass in [0,1] of the uniform "anywhere" term that absorbs '
                        'misses and scene cuts (default 0.05, an untuned placeholder), for filter, viterbi and marginal alike; --seq_fit starts from it.')
    parser.add_argument('--seq_fit', type=int, default=None, metavar='ITERS', help='with --sequence: first fit the motion model to the clip\'s own heat maps, without '
                        'annotations -- ITERS (1..100) iterations of EM on the smoothed posteriors (predict.seq_fit, DESIGN.md 4.23), starting from --seq_sigma / '
                        '--seq_rho or their defaults -- then run the chosen mode with the fitted sigma per joint and rho; the JSON line gains seq_fit.  Not with '
                        '--seq_people.')
    parser.add_argument('--seq_lag', type=int, default=None, metavar='L', help='with --sequence lag: the frames of future every position is given, L >= 1 (there is no '
                        'default: none has been tuned); the JSON line gains seq_lag.')
    parser.add_argument('--seq_people', type=int, default=None, metavar='M', help='with --sequence, --predict and --use_sm: a clip with up to M (1..4) people in it '
                        '(predict.predict_sequence_people, DESIGN.md 4.21): M consistent torso tracks are pulled out of the frames\' torso maps, the spatial model '
                        'runs once per frame and track, and every person\'s joints are tracked; every image of the document gains "tracks" ("track" is track 0) '
                        'and --render draws one skeleton per track present in the frame.  What this buys with trained weights has not been measured.')
    parser.add_argument('--seq_zoom', action='store_true', help='with --sequence filter or viterbi, --predict and --use_sm: track the person a second time at the scale '
                        'the tower was trained on (predict.predict_sequence_zoom, DESIGN.md 4.24): one zoom window per frame around the torso track, all on one '
                        'cell lattice, and the temporal scan with a whole-cell shift per frame; the document gains "zoom" and "track_zoom" per file, the JSON '
                        'line seq_zoom, seq_zoom_pitch, zoom_fit_ms and zoom_forward_ms.  Not with --sequence marginal, --seq_fit or --seq_people.')
    parser.add_argument('--seq_camera', action='store_true', help='with --sequence filter or viterbi: a camera that pans (DESIGN.md 4.26): the translation between '
                        'consecutive fitted frames is estimated on the device (Engine.frame_shift), turned into whole-cell shifts (motion.camera_shifts) and given to '
                        'the temporal scan, so that its motion kernel follows the camera; the document gains "camera" per file (disp, shift, sad).  Global '
                        'translation only, no cut detection.  Not with --seq_zoom, --seq_people, --seq_fit or --sequence marginal / lag.')
    parser.add_argument('--seq_camera_search', type=int, default=None, metavar='D', help='with --seq_camera: the coarse search radius in 1..16, reaching 4 D + 3 fitted '
                        'pixels a frame (default 8, an untuned placeholder).')
    parser.add_argument('--seq_flow', type=int, default=None, metavar='N', help='with --sequence filter, viterbi or marginal: pool every frame\'s heat maps with those of '
                        'the N (1..4, no default: none has been tuned) frames before and after it, each warped onto the frame by one displacement per heat-map cell '
                        '(Engine.frame_flow, Engine.hm_flow_pool, DESIGN.md 4.28), and run the mode on the pooled maps; the document gains "flow" per file, the JSON '
                        'line seq_flow and seq_flow_search.  Block matching on luma, whole pixels, no occlusion reasoning.  Not with --sequence lag, --seq_zoom or '
                        '--seq_people.')
    parser.add_argument('--seq_flow_search', type=int, default=None, metavar='D', help='with --seq_flow or --seq_flow_centre: the search radius in 1..16 fitted pixels a '
                        'frame (default 8, an untuned placeholder).')
    parser.add_argument('--seq_flow_centre', action='store_true', help='with --sequence filter or viterbi: centre every cell\'s motion kernel on where the cell\'s own '
                        'content was in the frame before (DESIGN.md 4.29): one displacement per heat-map cell against the frame before (Engine.frame_flow), rounded '
                        'to whole cells, fed to the scans as centre= (Engine.seq_filter / seq_viterbi).  With --seq_flow N as well the pooling\'s own matching is '
                        'reused and the scan runs on the pooled maps.  The document gains "flow_centre" per file, the JSON line seq_flow_centre, the search radius; '
                        'with --render the drawn track is the centred one.  Not with --seq_camera, --seq_zoom, --seq_people, --seq_fit or --sequence marginal / lag.')
    parser.add_argument('--seq_pose', type=int, default=None, metavar='P', help='with --sequence viterbi and --use_sm: also decode ONE skeleton per frame over the '
                        'whole clip (DESIGN.md 4.30): the P in 1..4 heat-map peaks per joint of every frame, the spatial model\'s energy of each of the P^9 poses '
                        '(Engine.pose_decode) and the motion model between the candidates of consecutive frames (Engine.seq_pose_viterbi), the exact MAP over the '
                        'sequence of poses.  The document gains "track_pose" per file, the JSON line seq_pose and seq_pose_weight; with --render the skeleton of '
                        'track_pose is drawn in place of the track.  Not with --seq_people, --seq_zoom, --seq_camera, --seq_flow, --seq_flow_centre or --seq_fit.')
    parser.add_argument('--seq_pose_weight', type=float, default=None, metavar='W', help='with --seq_pose: the weight of the motion term against the pose energy, '
                        'finite and >= 0 (default 1.0, an untuned placeholder: the two log-scores are of different origin).')
    parser.add_argument('--seq_torso_sigma', type=float, default=None, metavar='CELLS', help='with --seq_people: the standard deviation of a torso\'s motion per '
                        'frame in heat-map cells (default 1.5, an untuned placeholder).')
    parser.add_argument('--seq_exclude', type=int, default=None, metavar='CELLS', help='with --seq_people: the half-width in 0..64 heat-map cells of the square '
                        'around an earlier track\'s torso cell that a later track may not use in that frame (default 4, an untuned placeholder).')
    parser.add_argument('--augm_affine', action='store_true', help='--train: augment every batch on the device with one composed affine sample of the image -- '
                        'flip, brightness, contrast, a rotation of up to 20 degrees, scale and shift -- and targets redrawn as 3x3 blobs at the transformed joint '
                        'cells (Engine.augment_affine, DESIGN.md 4.20; drawn from --seed + 1).  Not the reference\'s --data_augm.  What it buys in detection rate '
                        'has not been measured.')
    parser.add_argument('--augm_antialias', action='store_true', help='with --augm_affine: sample through a triangle filter as wide as the picture is shrunk '
                        '(Engine.augment_affine(width=), DESIGN.md 4.27) instead of four bilinear taps, which alias below scale 1; scales >= 1 are sampled as '
                        'without it.  The scale range must start at 0.25 or above')
    parser.add_argument('--augm_scale', type=float, nargs=2, default=None, metavar=('LO', 'HI'), help='with --augm_affine: the scale is uniform in [LO, HI], '
                        '0 < LO <= HI (default 0.5 1.5, the range of the reference\'s docstring: an untuned placeholder).')
    parser.add_argument('--augm_shift', type=float, default=None, metavar='F', help='with --augm_affine: the shift is uniform in +-F of the frame width and height, '
                        '0 <= F < 0.5 (default 0, an untuned placeholder).')
    parser.add_argument('--augm_pad', type=float, default=None, metavar='V', help='with --augm_affine: the value of the pixels outside the source image, 0 <= V <= 1 '
                        '(default 0).')
    parser.add_argument('--seed', type=int, default=0, help='shuffling seed.')
    parser.add_argument('--device_data', action='store_true', help='--train: upload the train and test sets to device memory once and gather the batches there '
                        '(DESIGN.md 4.9); an error if they do not fit.')
    parser.add_argument('--u8_images', action='store_true', help='hold and move the images as the bytes they were made from (DESIGN.md 4.10; same results bit for '
                        'bit): the evaluation run streams byte batches from pinned memory (single scale; --multiscale is unchanged), --train needs '
                        '--device_data and keeps the sets as uint8 on the device.')
    parser.add_argument('--tb_dir', default=None, help='write TensorBoard summaries to DIR/<model_name>/{train,test} (main.py:448-450; off by default).')
    parser.add_argument('--tb_log_iters', action='store_true', help='with --tb_dir: histograms and scalars after every step to DIR/<model_name>/train_iter '
                        '(tb_log_iters, main.py:452,642-645).')
    parser.add_argument('--tb_activations', action='store_true', help='with --tb_dir: add the per-layer activation summaries of conv_layer (main.py:167-168) to the '
                        'epoch summaries of --train and the step-0 summaries of the evaluation run: tower_<i>/pre_activ_<layer>/{max,mean,min,std,n_pos,'
                        'histogram} and tower_<i>/f_activ_<layer>/image/<k> for all 15 layers, one tower per --gpus entry (fp32 only; DESIGN.md 4.8).')
    return parser


def configure(params, device=0, precision='fp32', debug=None):
    """Create the engine for `device` and load `params` (dict keyed by TF variable names).
    Replaces graph construction + tf.Session + Saver.restore (main.py:474-487,606-612)."""
    global _engine, pairwise_energies, pairwise_biases
    if debug is not None:
        hps.debug = bool(debug)
    if _engine is not None:
        _engine.close()
    _engine = Engine(device=device, precision=precision, n_joints=n_joints).load_params(params)
    dev = _engine.device
    pairwise_energies = {k[len('energy_'):]: torch.as_tensor(np.asarray(v), device=dev) for k, v in params.items() if k.startswith('energy_')}
    pairwise_biases = {k[len('bias_'):]: torch.as_tensor(np.asarray(v), device=dev) for k, v in params.items() if k.startswith('bias_')}
    return _engine


def engine():
    if _engine is None:
        raise RuntimeError('call joint_cnn_mrf_amd.main.configure(params) first (replaces sess.run setup)')
    return _engine


# ------------------------------------------------------------------ layer wrappers (main.py:128-181)
def conv_layer(x, size, stride, n_in, n_out, name, last_layer=False):
    """main.py:156-169."""
    if x.shape[-1] != n_in:
        raise ValueError('conv_layer %s: input has %d channels, n_in=%d' % (name, x.shape[-1], n_in))
    return engine().conv_layer(x, name, stride, last_layer=last_layer, n_out=n_out)


def max_pool_layer(x, size, stride):
    """main.py:172-174 (the model only uses 2x2/2)."""
    if (size, stride) != (2, 2):
        raise ValueError('only the 2x2 stride-2 SAME pool of the reference model is implemented')
    return engine().max_pool(x)


def resize_images(x, size):
    """tf.image.resize_images(x, [h, w]) with TF-1.x defaults (main.py:51,58,60,67)."""
    return engine().resize_bilinear(x, int(size[0]), int(size[1]))


# ------------------------------------------------------------------ model graph
def model(x, n_joints):
    """main.py:29-74.  x [B,480,720,3] -> logits [B,60,90,n_joints] (one fused C call)."""
    if n_joints != engine().n_joints:
        raise ValueError('engine was configured for %d joints' % engine().n_joints)
    return engine().model(x)


def model_layerwise(x, n_joints):
    """The same graph composed op by op through the per-layer entry points, line for line
    with main.py:38-74; used by the tests to cross-check the fused `model`."""
    n_filters = np.array([64, 128, 256, 512, 512])
    if hps.debug:
        n_filters = n_filters // 4
    n_filters = [int(f) for f in n_filters]

    x1 = x
    x1 = conv_layer(x1, 5, 2, 3, n_filters[0], 'conv1_fullres')
    x1 = max_pool_layer(x1, 2, 2)
    x1 = conv_layer(x1, 5, 1, n_filters[0], n_filters[1], 'conv2_fullres')
    x1 = max_pool_layer(x1, 2, 2)
    x1 = conv_layer(x1, 5, 1, n_filters[1], n_filters[2], 'conv3_fullres')
    x1 = conv_layer(x1, 9, 1, n_filters[2], n_filters[3], 'conv4_fullres')

    x2 = resize_images(x, [int(x.shape[1]) // 2, int(x.shape[2]) // 2])
    x2 = conv_layer(x2, 5, 2, 3, n_filters[0], 'conv1_halfres')
    x2 = max_pool_layer(x2, 2, 2)
    x2 = conv_layer(x2, 5, 1, n_filters[0], n_filters[1], 'conv2_halfres')
    x2 = max_pool_layer(x2, 2, 2)
    x2 = conv_layer(x2, 5, 1, n_filters[1], n_filters[2], 'conv3_halfres')
    x2 = conv_layer(x2, 9, 1, n_filters[2], n_filters[3], 'conv4_halfres')
    x2 = resize_images(x2, [int(x1.shape[1]), int(x1.shape[2])])

    x3 = resize_images(x, [int(x.shape[1]) // 4, int(x.shape[2]) // 4])
    x3 = conv_layer(x3, 5, 2, 3, n_filters[0], 'conv1_quarterres')
    x3 = max_pool_layer(x3, 2, 2)
    x3 = conv_layer(x3, 5, 1, n_filters[0], n_filters[1], 'conv2_quarterres')
    x3 = max_pool_layer(x3, 2, 2)
    x3 = conv_layer(x3, 5, 1, n_filters[1], n_filters[2], 'conv3_quarterres')
    x3 = conv_layer(x3, 9, 1, n_filters[2], n_filters[3], 'conv4_quarterres')
    x3 = resize_images(x3, [int(x1.shape[1]), int(x1.shape[2])])

    x = x1 + x2 + x3
    x = x / 3
    x = conv_layer(x, 9, 1, n_filters[3], n_filters[4], 'conv5')
    x = conv_layer(x, 9, 1, n_filters[4], n_joints, 'conv6', last_layer=True)
    return x


def conv_mrf(A, B):
    """main.py:77-91.  A [1,120,180,1] prior, B [b,60,90,1] likelihood -> [b,60,90,1]."""
    return engine().conv_mrf(A, B)


def spatial_model(heat_map):
    """main.py:94-125.  heat_map [B,60,90,10] -> [B,60,90,9]."""
    return engine().spatial_model(heat_map)


def spatial_softmax(hm):
    """main.py:212-217."""
    return engine().spatial_softmax(hm)


def get_joints_coords(hm):
    """evaluation.py:15-24 / main.py:389-397: int32 [B,2,K] (row, col)."""
    return engine().argmax_coords(hm)


def tower(x, hm_target, use_sm=None):
    """One tower of main.py:522-531: returns (hm_pred_pd, hm_pred_sm)."""
    use_sm = hps.use_sm if use_sm is None else use_sm
    hm_pred_pd_logit = model(x, n_joints)
    hm_pred_pd = spatial_softmax(hm_pred_pd_logit)
    if use_sm:
        hm_pred_pd_with_torso = torch.cat([hm_pred_pd, hm_target[:, :, :, n_joints:]], dim=3).contiguous()
        hm_pred_sm_logit = spatial_model(hm_pred_pd_with_torso)
        hm_pred_sm = spatial_softmax(hm_pred_sm_logit)
    else:
        hm_pred_sm = hm_pred_pd                      # main.py:535
    return hm_pred_pd, hm_pred_sm


def get_different_scales(x, pad_array, crop_array, orig_h, orig_w):
    """main.py:326-348: the 4 padded + 4 cropped copies of an image, resized back to orig_h x orig_w."""
    return multiscale.get_different_scales(engine(), x, pad_array, crop_array, orig_h, orig_w)


def scale_hm_back(hms, pad_array, crop_array, orig_h, orig_w):
    """main.py:351-379: undo the pad / crop on the 8 heat maps of an image."""
    return multiscale.scale_hm_back(engine(), hms, pad_array, crop_array, orig_h, orig_w)


def get_predictions(X_np, Y_np, sess=None):
    """main.py:382-425 (multi-scale test-time evaluation) -> (pred_coords_pd, pred_coords_sm), each
    [2, n_joints, N]; `sess` is accepted for signature compatibility and ignored."""
    return multiscale.get_predictions(engine(), X_np, Y_np, use_sm=hps.use_sm, flip_test=bool(getattr(hps, 'flip_test', False)))


model_path = 'models_ex'                                                                            # main.py:444


# ------------------------------------------------------------------ what main() refuses, and why (FLAG_RULES, above main(), has the order)
RESTORE_NEEDS_RESTORE_PATH = '--restore needs --restore_path <checkpoint prefix or .npz> (the reference hard-codes best_model_name, main.py:443)'
DET_CURVE_IS_EVALUATION_ONLY = ('--det_curve belongs to the evaluation run (it measures the predictions of the test set that run assembles); '
                                'it cannot be combined with --train')
PEAKS_IS_EVALUATION_ONLY = ('--peaks belongs to the evaluation run (it describes the heat maps of the test set that run predicts from); '
                            'it cannot be combined with --train')
PEAKS_NEEDS_PREDICTIONS = '--peaks writes flic_peaks_pd / flic_peaks_sm into the file of --predictions: give --predictions PATH as well'
PEAKS_NOT_WITH_U8_IMAGES = ('--peaks cannot be combined with --u8_images: the streamed byte feed (stream.ForwardStream) returns coordinates only; '
                            'run it on the float feed')
DECODE_POSE_IS_EVALUATION_ONLY = ('--decode_pose belongs to the evaluation run (it chooses among the peaks of the test set that run predicts from); '
                                  'it cannot be combined with --train')
DECODE_POSE_NEEDS_USE_SM = '--decode_pose scores poses with the spatial model: give --use_sm as well'
DECODE_POSE_NEEDS_PREDICTIONS = '--decode_pose writes flic_pred_pose / flic_pose_score into the file of --predictions: give --predictions PATH as well'
DECODE_POSE_NEEDS_PEAKS = '--decode_pose chooses among the peaks of --peaks P: give --peaks P with 1 <= P <= 4 as well'
DECODE_POSE_NOT_WITH_U8_IMAGES = ('--decode_pose cannot be combined with --u8_images: the streamed byte feed (stream.ForwardStream) returns coordinates only; '
                                  'run it on the float feed')
DECODE_POSE_NOT_WITH_MULTISCALE = ('--decode_pose cannot be combined with --multiscale: the multi-scale average has no per-scale candidates; '
                                   'run it on the single-scale path')
INFER_TORSO_IS_EVALUATION_ONLY = ('--infer_torso belongs to the evaluation run (training with an inferred torso map is not defined: the step reads the '
                                  'annotated channel); drop --train')
INFER_TORSO_NEEDS_USE_SM = '--infer_torso infers the torso map the spatial model reads: give --use_sm as well'
INFER_TORSO_SINGLE_SCALE_ONLY = ('--infer_torso cannot be combined with --multiscale, --flip_test or --u8_images: the torso under multi-scale and mirrored '
                                 'evaluation is not defined, and the streamed byte feed returns coordinates only')
PEOPLE_NEEDS_INFER_TORSO = '--people M (1 <= M <= 4) asks for one result per INFERRED torso candidate: give --infer_torso as well'
FLIP_TEST_IS_EVALUATION_ONLY = ('--flip_test belongs to the evaluation run (it averages the heat maps of a test image and of its mirror image); '
                                'it cannot be combined with --train')
PREDICT_NEEDS_PREDICTIONS = '--predict writes its JSON document to the file of --predictions: give --predictions OUT.json as well'
PREDICT_NOT_WITH_TRAIN = '--predict runs the tower on the named images and is no training run: drop --train'
PREDICT_NOT_WITH_MULTISCALE = ('--predict cannot be combined with --multiscale: with --use_sm the torso is inferred, and the inferred torso under multi-scale '
                               'evaluation is not defined')
PREDICT_NOT_WITH_FLIP_TEST = ('--predict cannot be combined with --flip_test: with --use_sm the torso is inferred, and the inferred torso under mirrored '
                              'evaluation is not defined')
PREDICT_NOT_WITH_DET_CURVE = '--predict cannot be combined with --det_curve: the named images have no annotation to measure a detection rate against'
PREDICT_NOT_WITH_DEVICE_DATA = '--predict cannot be combined with --device_data: that flag places the training sets of --train'
ZOOM_NEEDS_PREDICT = '--zoom is the second pass of --predict (a window around every person the first pass found): give --predict PATH as well'
ZOOM_NEEDS_USE_SM = ('--zoom needs --use_sm: the windows are placed at the inferred torso and sized by the shoulders and hips of the spatial model, '
                     'and the second pass runs the spatial model at the torso cell it is given')
RENDER_NEEDS_PREDICT = '--render draws the result of --predict onto its input images: give --predict PATH as well'
RENDER_HEAT_NEEDS_RENDER = '--render_heat tints the pictures --render writes: give --render DIR as well'
RENDER_HEAT_SM_NEEDS_USE_SM = '--render_heat sm tints with the maps of the spatial model: give --use_sm as well, or ask for --render_heat pd'
SEQUENCE_NEEDS_PREDICT = '--sequence tracks the joints over the frames --predict names: give --predict PATH as well'
SEQUENCE_NO_ZOOM = '--sequence cannot be combined with --zoom: the windows of the second pass would move from frame to frame, which is out of scope'
SEQUENCE_ONE_PERSON = '--sequence tracks one person: --people M > 1 would need an association of people across frames, which is out of scope'
SEQ_OPTION_NEEDS_SEQUENCE = '--seq_sigma and --seq_rho set the motion model of --sequence: give --sequence filter or --sequence viterbi as well'
SEQ_PEOPLE_NEEDS_SEQUENCE = '--seq_people tracks the people of the clip --sequence names: give --sequence filter or --sequence viterbi as well'
SEQ_PEOPLE_NEEDS_USE_SM = '--seq_people needs --use_sm: the torso tracks come from the inferred torso map and every person is one run of the spatial model'
SEQ_MARGINAL_NO_PEOPLE = '--sequence marginal cannot be combined with --seq_people: the torso tracks have the filter and Viterbi only'
SEQ_FIT_NEEDS_SEQUENCE = '--seq_fit fits the motion model of --sequence to the clip: give --sequence filter, viterbi or marginal as well'
SEQ_FIT_NO_PEOPLE = '--seq_fit cannot be combined with --seq_people: the fit is that of one person\'s joint maps'
SEQ_ZOOM_NEEDS_SEQUENCE = '--seq_zoom zooms into the clip --sequence names: give --sequence filter or --sequence viterbi as well'
SEQ_ZOOM_NEEDS_USE_SM = '--seq_zoom needs --use_sm: the windows are placed on the torso track and sized by the spatial model\'s shoulders and hips'
SEQ_ZOOM_NO_MARGINAL = '--seq_zoom cannot be combined with --sequence marginal: the smoother has no form for windows that move from frame to frame'
SEQ_ZOOM_NO_FIT = '--seq_zoom cannot be combined with --seq_fit: the fit runs on the smoother, which has no form for windows that move from frame to frame'
SEQ_ZOOM_NO_PEOPLE = '--seq_zoom cannot be combined with --seq_people: a zoom pass per track is out of scope'
SEQ_LAG_NEEDS_SEQUENCE_LAG = '--seq_lag sets the lag of --sequence lag: give --sequence lag as well'
SEQ_LAG_NEEDS_SEQ_LAG = '--sequence lag needs its lag: give --seq_lag L as well (there is no default: none has been tuned)'
SEQ_LAG_NO_PEOPLE = '--sequence lag cannot be combined with --seq_people: the torso tracks have the filter and Viterbi only'
SEQ_LAG_NO_ZOOM = '--sequence lag cannot be combined with --seq_zoom: the smoother has no form for windows that move from frame to frame'
SEQ_CAMERA_NEEDS_SEQUENCE = '--seq_camera follows the camera through the clip --sequence names: give --sequence filter or --sequence viterbi as well'
SEQ_CAMERA_NO_SMOOTHER = '--seq_camera cannot be combined with --sequence marginal or lag: the smoother has no form for a lattice that moves from frame to frame'
SEQ_CAMERA_NO_FIT = '--seq_camera cannot be combined with --seq_fit: the fit runs on the smoother, which has no form for a lattice that moves from frame to frame'
SEQ_CAMERA_NO_ZOOM = '--seq_camera cannot be combined with --seq_zoom: the zoom windows already move with the person'
SEQ_CAMERA_NO_PEOPLE = '--seq_camera cannot be combined with --seq_people: the torso passes have no form for a lattice that moves from frame to frame'
SEQ_CAMERA_SEARCH_NEEDS_SEQ_CAMERA = '--seq_camera_search sets the search radius of --seq_camera: give --seq_camera as well'
SEQ_FLOW_NEEDS_SEQUENCE = '--seq_flow pools the heat maps of the clip --sequence names: give --sequence filter, viterbi or marginal as well'
SEQ_FLOW_NO_LAG = '--seq_flow cannot be combined with --sequence lag: two-sided pooling reads frames that the lag has not yet seen'
SEQ_FLOW_NO_ZOOM = '--seq_flow cannot be combined with --seq_zoom: the zoom windows move the lattice from frame to frame'
SEQ_FLOW_NO_PEOPLE = '--seq_flow cannot be combined with --seq_people: every track has maps of its own, and pooling per track is out of scope'
SEQ_FLOW_SEARCH_NEEDS_SEQ_FLOW = '--seq_flow_search sets the search radius of --seq_flow: give --seq_flow N as well'
SEQ_FLOW_CENTRE_NEEDS_SEQUENCE = '--seq_flow_centre centres the scan of the clip --sequence names: give --sequence filter or --sequence viterbi as well'
SEQ_FLOW_CENTRE_NO_SMOOTHER = '--seq_flow_centre cannot be combined with --sequence marginal or lag: the smoother has no form for a shift per cell'
SEQ_FLOW_CENTRE_NO_FIT = '--seq_flow_centre cannot be combined with --seq_fit: the fit runs on the smoother, which has no form for a shift per cell'
SEQ_FLOW_CENTRE_NO_CAMERA = '--seq_flow_centre cannot be combined with --seq_camera: the flow of a cell already contains the pan'
SEQ_FLOW_CENTRE_NO_ZOOM = '--seq_flow_centre cannot be combined with --seq_zoom: the zoom windows move the lattice from frame to frame'
SEQ_FLOW_CENTRE_NO_PEOPLE = '--seq_flow_centre cannot be combined with --seq_people: the torso passes have no form for a shift per cell'
SEQ_POSE_NEEDS_PREDICT = '--seq_pose decodes the poses of the clip --predict names: give --predict as well'
SEQ_POSE_NEEDS_USE_SM = '--seq_pose needs --use_sm: the pose energy is the spatial model\'s'
SEQ_POSE_NEEDS_VITERBI = '--seq_pose is an offline MAP over the clip: give --sequence viterbi as well'
SEQ_POSE_WEIGHT_NEEDS_SEQ_POSE = '--seq_pose_weight weighs the motion term of --seq_pose: give --seq_pose P as well'
SEQ_POSE_NO_PEOPLE = '--seq_pose cannot be combined with --seq_people: the clip decode picks one skeleton per frame'
SEQ_POSE_NO_ZOOM = '--seq_pose cannot be combined with --seq_zoom: the zoom windows move the lattice from frame to frame'
SEQ_POSE_NO_CAMERA = '--seq_pose cannot be combined with --seq_camera: the transition between candidates has no moving form'
SEQ_POSE_NO_FLOW = '--seq_pose cannot be combined with --seq_flow: the candidates are the peaks of the frames\' own maps, not of pooled ones'
SEQ_POSE_NO_FLOW_CENTRE = '--seq_pose cannot be combined with --seq_flow_centre: the transition between candidates has no centred form'
SEQ_POSE_NO_FIT = '--seq_pose cannot be combined with --seq_fit: the fitted sigma and rho belong to the per-joint scans'
SEQ_PEOPLE_OPTION_NEEDS_SEQ_PEOPLE = '--seq_torso_sigma and --seq_exclude set the torso passes of --seq_people: give --seq_people M as well'
U8_TRAIN_NEEDS_DEVICE_DATA = ('--train --u8_images needs --device_data: byte images are held on the device and widened by the gather / the augmentation; '
                              'host-fed training steps take float batches')
AUGM_AFFINE_NEEDS_TRAIN = '--augm_affine augments the batches of a training run: give --train as well'
AUGM_ANTIALIAS_NEEDS_AUGM_AFFINE = '--augm_antialias chooses the sampler of --augm_affine: give --augm_affine as well'
AUGM_ANTIALIAS_SCALE_FLOOR = '--augm_antialias: the widest filter is 9 x 9 taps, scale 0.25: give --augm_scale LO HI with LO >= 0.25'
EVAL_SCALE_NEEDS_SCALE_CURVE = '--eval_scale sweeps the test set over person scales and writes the curves: give --scale_curve PATH as well'
SCALE_CURVE_NEEDS_EVAL_SCALE = '--scale_curve is where the curves of --eval_scale go: give --eval_scale S [S ...] as well'
EVAL_SCALE_IS_EVALUATION_ONLY = '--eval_scale belongs to the evaluation run (the run without --train and without --predict)'
EVAL_SCALE_SINGLE_SCALE_ONLY = ('--eval_scale cannot be combined with --multiscale, --flip_test, --infer_torso or --u8_images: the sweep sends float batches '
                                'through the single-scale forward with the redrawn torso map')
AUGM_OPTION_NEEDS_AUGM_AFFINE = '--augm_scale, --augm_shift and --augm_pad set the ranges of --augm_affine: give --augm_affine as well'
SYNTH_PEOPLE_NOT_WITH_SYNTHETIC = '--synth_people and --synthetic both replace the data set: give one of them'
SYNTH_PEOPLE_NOT_WITH_PREDICT = '--synth_people replaces the data of --train and of the evaluation run; --predict reads the images it names: drop one of them'
SYNTH_FRESH_NEEDS_COMPANIONS = ('--synth_fresh draws the device-resident byte training set of rendered people again every epoch: give --train, --device_data, '
                                '--u8_images and --synth_people POSES.npy as well')
SYNTH_DUMP_NEEDS_SYNTH_PEOPLE = '--synth_dump writes pictures of the test set --synth_people renders: give --synth_people POSES.npy as well'
TB_ACTIVATIONS_NEEDS_TB_DIR ='--tb_activations adds tags to the summaries --tb_dir writes: give --tb_dir DIR as well'
TB_ACTIVATIONS_IS_FP32 = ('--tb_activations: the pre-activation summaries are taken in fp32, as the reference takes them, and the bf16 kernels have no '
                          'linear epilogue; run it with --precision fp32')


def predict_main(args):
    """--predict PATH [PATH ...]: the named images through predict.predict_images on the first listed device; the JSON document goes to
    --predictions, one JSON line with the image count and the device times of the fit and of the forwards to stdout.  With --render DIR the
    images come back with the result drawn on them (predict.render_images) and go to DIR as PNG files; the line gains render_ms.  With --sequence
    the images are the frames of one clip (predict.predict_sequence): the document gains "track" per file, the pictures show the tracked skeleton; with --seq_people M
    (predict.predict_sequence_people) also "tracks", one skeleton per person, and the line gains seq_people, seq_torso_ms and seq_people_sm_ms; with --seq_zoom
    (predict.predict_sequence_zoom) "zoom" and "track_zoom", the pictures show the skeleton tracked through the windows where the clip was zoomed, and the line
    gains seq_zoom, seq_zoom_pitch, zoom_fit_ms and zoom_forward_ms; with --sequence lag --seq_lag L the line gains seq_lag; with --seq_camera the document gains
    "camera" per file and the line seq_camera, the search radius; with --seq_flow N the document gains "flow" per file and the line seq_flow
    and seq_flow_search; with --seq_flow_centre the document gains "flow_centre" per file and the line seq_flow_centre, the search radius --
    'track', which --render draws, is the centred one; with --seq_pose P the document gains "track_pose" per file and the line seq_pose
    and seq_pose_weight -- --render draws the skeleton of track_pose."""
    from . import predict
    files = predict.expand_paths(args.predict)
    images = [predict.load_image(f) for f in files]
    pairwise = None if args.restore else synth.synthetic_priors() if args.synthetic else get_pairwise_distr(args.data_dir) if args.use_sm else None
    params, _ = run_params(args, pairwise)
    hps.debug = bool(args.debug)
    eng = Engine(device=args.gpus[0], precision=args.precision, n_joints=n_joints).load_params(params)
    try:
        timing = {}
        if args.sequence:
            sigma = predict.SEQ_SIGMA if args.seq_sigma is None else args.seq_sigma
            seq = dict(mode=args.sequence, sigma=sigma[0] if isinstance(sigma, list) and len(sigma) == 1 else sigma,
                       rho=predict.SEQ_RHO if args.seq_rho is None else args.seq_rho, batch_size=args.batch_size, keep_maps=bool(args.render_heat),
                       peaks=args.peaks, decode=args.decode_pose, timing=timing)
            if args.seq_fit is not None:
                seq.update(fit_iters=args.seq_fit)
            if args.seq_lag is not None:
                seq.update(lag=args.seq_lag)
            if args.seq_zoom:
                results = predict.predict_sequence_zoom(eng, images, **seq)
            elif args.seq_people is not None:
                results = predict.predict_sequence_people(eng, images, args.seq_people, exclude=predict.SEQ_EXCLUDE if args.seq_exclude is None else args.seq_exclude,
                                                          torso_sigma=predict.SEQ_TORSO_SIGMA if args.seq_torso_sigma is None else args.seq_torso_sigma, **seq)
            else:
                if args.seq_camera:
                    seq.update(camera=True, camera_search=predict.SEQ_CAMERA_SEARCH if args.seq_camera_search is None else args.seq_camera_search)
                if args.seq_flow is not None:
                    seq.update(flow=args.seq_flow, flow_search=predict.SEQ_FLOW_SEARCH if args.seq_flow_search is None else args.seq_flow_search)
                if args.seq_flow_centre:
                    seq.update(flow_centre=True, flow_search=predict.SEQ_FLOW_SEARCH if args.seq_flow_search is None else args.seq_flow_search)
                if args.seq_pose is not None:
                    seq.update(pose=args.seq_pose, pose_weight=1.0 if args.seq_pose_weight is None else args.seq_pose_weight)
                results = predict.predict_sequence(eng, images, use_sm=args.use_sm, **seq)
        else:
            results = predict.predict_images(eng, images, use_sm=args.use_sm, peaks=args.peaks, decode=args.decode_pose, people=args.people,
                                             batch_size=args.batch_size, timing=timing, zoom=args.zoom, keep_maps=bool(args.render_heat))
        if args.render:
            pictures = predict.render_images(eng, images, results, heat=args.render_heat, which=('track_zoom' if args.seq_zoom and 'track_zoom' in results[0] else 'track_pose' if args.seq_pose is not None else 'track') if args.sequence else None,
                                             batch_size=args.batch_size, timing=timing)
    finally:
        eng.close()
    os.makedirs(os.path.dirname(args.predictions) or '.', exist_ok=True)
    with open(args.predictions, 'w') as fh:
        json.dump(predict.predictions_document(files, results), fh)
    line = {'predict': True, 'n_images': len(files), 'fit_ms': timing['fit_ms'], 'forward_ms': timing['forward_ms'], 'gpu': args.gpus[0],
            'use_sm': bool(args.use_sm), 'debug': bool(args.debug)}
    if args.sequence:
        line.update(sequence=args.sequence)
    if args.seq_lag is not None:
        line.update(seq_lag=args.seq_lag)
    if args.seq_fit is not None:
        fit = results[0]['seq_fit']
        line.update(seq_fit={'sigma': fit['sigma'].tolist(), 'rho': fit['rho'], 'loglik': fit['loglik'].tolist(), 'clamped': fit['clamped'].tolist()})
    if args.seq_camera:
        line.update(seq_camera=predict.SEQ_CAMERA_SEARCH if args.seq_camera_search is None else args.seq_camera_search)
    if args.seq_flow is not None:
        line.update(seq_flow=args.seq_flow, seq_flow_search=predict.SEQ_FLOW_SEARCH if args.seq_flow_search is None else args.seq_flow_search)
    if args.seq_flow_centre:
        line.update(seq_flow_centre=predict.SEQ_FLOW_SEARCH if args.seq_flow_search is None else args.seq_flow_search)
    if args.seq_pose is not None:
        line.update(seq_pose=args.seq_pose, seq_pose_weight=1.0 if args.seq_pose_weight is None else args.seq_pose_weight)
    if args.seq_people is not None:
        line.update(seq_people=args.seq_people, seq_torso_ms=timing['seq_torso_ms'], seq_people_sm_ms=timing['seq_people_sm_ms'])
    if args.seq_zoom:
        line.update(seq_zoom=True, seq_zoom_pitch=timing['seq_zoom_pitch'], zoom_fit_ms=timing['zoom_fit_ms'], zoom_forward_ms=timing['zoom_forward_ms'])
    if args.zoom:
        line.update(zoom=True, zoom_fit_ms=timing['zoom_fit_ms'], zoom_forward_ms=timing['zoom_forward_ms'])
    if args.render:
        from .summary import encode_png
        os.makedirs(args.render, exist_ok=True)
        for i, (f, picture) in enumerate(zip(files, pictures)):
            with open(os.path.join(args.render, '%05d_%s.png' % (i, os.path.splitext(os.path.basename(f))[0])), 'wb') as fh:
                fh.write(encode_png(picture))
        line.update(render_ms=timing['render_ms'])
    print(json.dumps(line))


class TowerTrainer:
    """The training side of the in-process towers (main.py:509-577): every listed device runs compute_gradients on its
    slice of the batch, the tower gradients are averaged (average_gradients, main.py:243-267: here a sum on the first
    device divided by the tower count) and the same clipped update is applied to every replica.  The BatchNorm moving
    statistics are shared variables in the reference and the towers' update ops (main.py:557) run on them one after the
    other, tower 0 first: moving <- 0.9 * moving + 0.1 * stat_i for i = 0, 1, ...  Each replica here did that once from the
    common start, so the composition is rebuilt from the per-replica results and written to every replica."""
    BN_DECAY = 0.9          # decay=0.9 of the reference's tf.contrib.layers.batch_norm calls (main.py:113,129)

    def __init__(self, towers, params, augment_rng=None, augment_kind='reference', affine_kw=None, **trainer_kw):
        from .train import Trainer
        if augment_kind not in ('reference', 'affine'):
            raise ValueError("augment_kind must be 'reference' or 'affine', got %r" % (augment_kind,))
        if affine_kw and augment_kind != 'affine':
            raise ValueError("affine_kw belongs to augment_kind='affine'")
        self.towers = towers
        self.augment_rng = augment_rng      # numpy RandomState: augment every step (main.py:494-497), parameters drawn for the global batch
        self.augment_kind = augment_kind    # 'reference': augmentation.draw_params; 'affine': augmentation.draw_affine
        self.affine_kw = dict(affine_kw or {})      # pad, scale, max_angle, shift, antialias of augmentation.draw_affine
        self.trainers = [Trainer(e, **trainer_kw) for e in towers.engines]
        self.moving = {k: np.asarray(v, np.float32).reshape(-1).copy() for k, v in params.items()
                       if k.endswith('moving_mean') or k.endswith('moving_variance')}

    def _draw(self, B, H, W):
        """The augmentation draw of one global batch, or None: made before the towers slice the batch, so the images are the same for any tower count."""
        if self.augment_rng is None:
            return None
        from .augmentation import draw_affine, draw_params
        return draw_affine(self.augment_rng, B, H, W, **self.affine_kw) if self.augment_kind == 'affine' else draw_params(self.augment_rng, B)

    def train_step(self, x, y):
        tw = self.towers
        aug = self._draw(x.shape[0], x.shape[1], x.shape[2])
        for tr, eng, (lo, hi) in zip(self.trainers, tw.engines, tw.slices(x.shape[0])):
            xs = torch.as_tensor(x[lo:hi]).to(eng.device, non_blocking=True).contiguous()
            ys = torch.as_tensor(y[lo:hi]).to(eng.device, non_blocking=True).contiguous()
            with torch.cuda.device(eng.device):
                tr.loss_and_grads(xs, ys, augment=None if aug is None else aug[lo:hi])
        return self._average_and_apply()

    def train_step_indexed(self, datasets, idx):
        """train_step on the batch `idx` (host integers, one global batch) of device-resident data: `datasets` is a DeviceDataset or
        {device: DeviceDataset} (DeviceDataset.for_towers: one copy per distinct device).  Every tower gathers its slice idx[lo:hi] on its
        own device -- with augment_rng through the indexed augmentation, the parameters drawn for the global batch as in train_step."""
        tw = self.towers
        idx = np.asarray(idx).reshape(-1)
        ds0 = next(iter(datasets.values())) if isinstance(datasets, dict) else datasets
        aug = self._draw(idx.shape[0], ds0.x.shape[1], ds0.x.shape[2])
        for tr, eng, (lo, hi) in zip(self.trainers, tw.engines, tw.slices(idx.shape[0])):
            ds = datasets[eng.device] if isinstance(datasets, dict) else datasets
            if ds.device != eng.device:
                raise ValueError('the data set is on %s, the tower on %s' % (ds.device, eng.device))
            with torch.cuda.device(eng.device):
                tr.loss_and_grads_indexed(ds, idx[lo:hi], augment=None if aug is None else aug[lo:hi])
        return self._average_and_apply()

    def _average_and_apply(self):
        """The tower average, the clipped update on every replica and the composed moving statistics (the tail of a step)."""
        tw = self.towers
        dev0 = tw.engines[0].device
        if tw.n > 1:
            total = self.trainers[0].grads
            for tr in self.trainers[1:]:
                total += tr.grads.to(dev0)
            total /= tw.n
            for tr in self.trainers[1:]:
                tr.grads.copy_(total)
        for tr, eng in zip(self.trainers, tw.engines):
            with torch.cuda.device(eng.device):
                tr.apply()
        if tw.n == 1:                                              # one tower: its own moving statistics are the result, nothing to compose or read back
            return self.trainers[0].losses
        names = sorted(self.moving)
        for i, name in enumerate(names):
            start = self.moving[name]
            cur = start.astype(np.float64)
            for tr in self.trainers:                               # r_i = d * start + (1 - d) * stat_i  ->  cur = d * cur + (r_i - d * start)
                cur = self.BN_DECAY * cur + (tr.get_tensor(name, start.shape).astype(np.float64) - self.BN_DECAY * start)
            self.moving[name] = cur.astype(np.float32)
            for eng in tw.engines:
                eng.update_tensor(name, self.moving[name], refresh=i == len(names) - 1)
        return self.trainers[0].losses


TB_SCALARS = ['main/mse_pd', 'main/mse_sm', 'main/det_rate_pd', 'main/det_rate_sm']      # main.py:632-635
IMG_TB_FROM = 450                                                                           # main.py:470


def tb_batch(x, y, batch_size):
    """The summary batch (main.py:470-471,621-626): batch_size images from image 450, or the first batch_size when the split is
    shorter."""
    lo = IMG_TB_FROM if x.shape[0] >= IMG_TB_FROM + batch_size else 0
    bx = np.asarray(x[lo:lo + batch_size])
    bx = bx.astype(np.float32) / np.float32(255) if bx.dtype == np.uint8 else bx      # (byte images: the floats they stand for)
    return np.ascontiguousarray(bx, np.float32), np.ascontiguousarray(y[lo:lo + batch_size], np.float32)


def tb_open(args, model_name):
    """tf.summary.FileWriter(tb/<model_name>/{train,test,train_iter}, flush_secs=30) (main.py:448-450,599-601)."""
    from . import summary
    root = os.path.join(args.tb_dir, model_name)
    w = {k: summary.FileWriter(os.path.join(root, k), flush_secs=30) for k in ('train', 'test')}
    if getattr(args, 'tb_log_iters', False):
        w['train_iter'] = summary.FileWriter(os.path.join(root, 'train_iter'), flush_secs=30)
    return w


def tb_summaries(writers, eng, layout, batches, use_sm, step, grads=None, params_flat=None, activations=False, n_towers=1):
    """run_summary of the merged summary for the train and the test batch (main.py:621-626,650-653); activations: with the per-layer
    activation summaries (--tb_activations), the batch cut into n_towers tower slices."""
    from . import summary
    for split, (bx, by) in batches.items():
        x = torch.as_tensor(bx).to(eng.device)
        y = torch.as_tensor(by).to(eng.device)
        summary.run_summary(writers[split], summary.merged_summary(eng, layout, x, y, use_sm, n_joints, grads=grads, params_flat=params_flat,
                                                                       activations=activations, n_towers=n_towers), step)


def train_main(args):
    """`--train` (main.py:620-667): the reference's epoch loop -- shuffled whole batches (get_next_batch), eval_error on
    the first n_eval_ex train / test examples after every epoch, the reference's progress line, a checkpoint per epoch once
    half of the epochs are done (tf.train.Saver format) -- on one tower per device of --gpus."""
    from . import checkpoint, evaluation, tf_checkpoint
    from .dist import Towers
    from .train import Trainer
    if args.data_augm:
        raise NotImplementedError('--data_augm: the augmentation pipeline (augmentation.py: flips, rotations, crops on the TF input '
                                  'queue) is outside the hot path this build covers; train without it')
    t_start = time.time()
    people = {}      # --synth_people: the poses, the index sets and the joint cells of the rendered sets
    x_train, y_train, x_test, y_test, pairwise = load_data(args, people)
    if args.synthetic and args.u8_images:
        x_train, x_test = byte_grid(x_train), byte_grid(x_test)
    n_train, n_test = x_train.shape[0], x_test.shape[0]
    rng = np.random.RandomState(args.seed)
    n_eval_ex = 512 if args.debug else 1100                              # main.py:453
    if args.debug and not args.synthetic and not args.synth_people:      # main.py:459-462 (a rendered set is sized by --synthetic_size)
        n_train, n_test = min(1024, n_train), min(512, n_test)
        tr_idx, te_idx = np.sort(rng.permutation(x_train.shape[0])[:n_train]), np.sort(rng.permutation(x_test.shape[0])[:n_test])
        x_train, y_train, x_test, y_test = x_train[tr_idx], y_train[tr_idx], x_test[te_idx], y_test[te_idx]
    n_updates_total = args.n_epochs * n_train // args.batch_size        # main.py:466
    params, state = run_params(args, pairwise)
    towers = Towers(params, args.gpus, precision=args.precision)
    augm = {}
    if args.augm_affine:      # drawn from a generator of its own: the batches are those of the run without it
        kw = {'scale': args.augm_scale, 'shift': args.augm_shift, 'pad': args.augm_pad, 'antialias': True if args.augm_antialias else None}
        augm = dict(augment_rng=np.random.RandomState(args.seed + 1), augment_kind='affine', affine_kw={k: v for k, v in kw.items() if v is not None})
    tt = TowerTrainer(towers, params, optimizer=args.optimizer, lr=args.lr, lmbd=args.lmbd, use_sm=args.use_sm, n_updates_total=n_updates_total, **augm)
    if state:
        for tr in tt.trainers:
            checkpoint.restore_session_state(tr, state)
    eng = towers.engines[0]
    run_name = model_name(args)
    joints_to_eval, det_radius = [2], 10                                 # main.py:455-456
    tb = tb_open(args, run_name) if args.tb_dir else None
    tb_batches = {'train': tb_batch(x_train, y_train, args.batch_size), 'test': tb_batch(x_test, y_test, args.batch_size)} if tb else None

    ds_train = ds_test = None
    ev_train, ev_test = (x_train, y_train), (x_test, y_test)
    if args.device_data:      # the (debug-subset) sets live on the towers' devices; eval_error reads the first tower's copy
        from .dataset import DeviceDataset
        # room the engines have not claimed yet: a full-width fp32 engine's filter-spectra cache and workspace grow to 64 GB on first use
        reserve = len(towers.engines) * ((2 << 30) if args.debug else (64 << 30))
        kind = 'uint8' if args.u8_images else 'float32'     # uint8: float files are converted chunk by chunk, the round trip checked (NotByteExact)
        ds_test = DeviceDataset(x_test, y_test, device=eng.device, reserve_bytes=reserve, image_dtype=kind, cells=people.get('cells_test'))
        ds_train = DeviceDataset.for_towers(towers, x_train, y_train, reserve_bytes=reserve, image_dtype=kind, cells=people.get('cells_train'))
        if args.u8_images:
            for name, d in [('test', ds_test)] + [('train', d) for d in ds_train.values()]:
                print('device data (%s, images as uint8): %d bytes held on %s, uploaded in %.2f s' % (name, d.nbytes, d.device, d.upload_seconds), flush=True)
        ev_train, ev_test = (ds_train[eng.device].x, ds_train[eng.device].y), (ds_test.x, ds_test.y)

    def report(epoch):
        if tb:      # gradients of the epoch's last update (none before the first)
            tb_summaries(tb, eng, tt.trainers[0].layout, tb_batches, args.use_sm, epoch, grads=tt.trainers[0].grads if epoch > 0 else None,
                         activations=args.tb_activations, n_towers=len(args.gpus))
        tr_e = evaluation.eval_error(ev_train[0][:n_eval_ex], ev_train[1][:n_eval_ex], eng, args.batch_size, args.use_sm, joints_to_eval, det_radius)
        te_e = evaluation.eval_error(ev_test[0][:n_eval_ex], ev_test[1][:n_eval_ex], eng, args.batch_size, args.use_sm, joints_to_eval, det_radius)
        print('Epoch {:d}  test_dr {:.3f} {:.3f}  train_dr {:.3f} {:.3f}  test_mse {:.5f} {:.5f}  train_mse {:.5f} {:.5f}'.format(
            epoch, te_e[2], te_e[3], tr_e[2], tr_e[3], te_e[0], te_e[1], tr_e[0], tr_e[1]), flush=True)      # main.py:628-631,656-657
        if tb:
            from . import summary
            summary.write_summary(tb['test'], [float(v) for v in te_e[:4]], TB_SCALARS, epoch)
            summary.write_summary(tb['train'], [float(v) for v in tr_e[:4]], TB_SCALARS, epoch)

    def steps(epoch):      # one epoch of updates (main.py:641): the same permutation from `rng` on either route
        if args.synth_fresh and epoch > 1:      # new scenes of the same poses, from a generator of their own: `rng` draws the batches of a run without it
            for e in towers.engines:
                ds_train[e.device].rerender_people(e, people['poses'], people['train_idx'], people_seed(args, epoch))
        if ds_train is not None:
            for batch_idx in ds_train[eng.device].epoch_indices(rng, args.batch_size, shuffle=True):
                yield tt.train_step_indexed(ds_train, batch_idx)
        else:
            for bx, by in evaluation.get_next_batch(x_train, y_train, args.batch_size, shuffle=True, rng=rng):
                yield tt.train_step(np.ascontiguousarray(bx, np.float32), np.ascontiguousarray(by, np.float32))

    report(0)
    global_iter = 0
    for epoch in range(1, args.n_epochs + 1):
        for _ in steps(epoch):
            global_iter += 1
            if tb and 'train_iter' in tb:       # main.py:642-645, without the images and without the activation summaries
                from . import summary
                tr0 = tt.trainers[0]
                summary.run_summary(tb['train_iter'], summary.merged_summary(eng, tr0.layout, use_sm=args.use_sm, n_joints=n_joints,
                                                                             grads=tr0.grads, images=False), global_iter)
        report(epoch)
        if epoch > args.n_epochs // 2:                                   # main.py:663-666
            tf_checkpoint.save_checkpoint('{}/{}-{}'.format(args.model_path, run_name, epoch), checkpoint.session_state(tt.trainers[0], params))
    for w in (tb or {}).values():
        w.close()
    print('Done in {:.2f} min\n\n'.format((time.time() - t_start) / 60))
    return tt


# What main() refuses: (holds for these flags, message or function of the flags giving it), in the order of precedence -- the first rule
# that holds ends the run with its message, so a rule may rely on every rule above it having passed.
FLAG_RULES = (
    (lambda a: a.restore and not a.restore_path, RESTORE_NEEDS_RESTORE_PATH),
    (lambda a: a.predict and a.train, PREDICT_NOT_WITH_TRAIN),
    (lambda a: a.predict and a.multiscale, PREDICT_NOT_WITH_MULTISCALE),
    (lambda a: a.predict and a.flip_test, PREDICT_NOT_WITH_FLIP_TEST),
    (lambda a: a.predict and a.det_curve, PREDICT_NOT_WITH_DET_CURVE),
    (lambda a: a.predict and a.device_data, PREDICT_NOT_WITH_DEVICE_DATA),
    (lambda a: a.predict and not a.predictions, PREDICT_NEEDS_PREDICTIONS),
    (lambda a: a.zoom and not a.predict, ZOOM_NEEDS_PREDICT),
    (lambda a: a.zoom and not a.use_sm, ZOOM_NEEDS_USE_SM),
    (lambda a: a.train and a.det_curve, DET_CURVE_IS_EVALUATION_ONLY),
    (lambda a: a.train and a.flip_test, FLIP_TEST_IS_EVALUATION_ONLY),
    (lambda a: a.train and a.u8_images and not a.device_data, U8_TRAIN_NEEDS_DEVICE_DATA),
    (lambda a: a.infer_torso and a.train, INFER_TORSO_IS_EVALUATION_ONLY),
    (lambda a: a.infer_torso and not a.use_sm, INFER_TORSO_NEEDS_USE_SM),
    (lambda a: a.infer_torso and (a.multiscale or a.flip_test or a.u8_images), INFER_TORSO_SINGLE_SCALE_ONLY),
    (lambda a: a.people != 1 and not ((a.infer_torso or (a.predict and a.use_sm)) and 1 <= a.people <= 4), PEOPLE_NEEDS_INFER_TORSO),
    (lambda a: a.decode_pose and a.train, DECODE_POSE_IS_EVALUATION_ONLY),
    (lambda a: a.decode_pose and not a.use_sm, DECODE_POSE_NEEDS_USE_SM),
    (lambda a: a.decode_pose and not a.predictions, DECODE_POSE_NEEDS_PREDICTIONS),
    (lambda a: a.decode_pose and not 1 <= a.peaks <= 4, DECODE_POSE_NEEDS_PEAKS),
    (lambda a: a.decode_pose and a.u8_images, DECODE_POSE_NOT_WITH_U8_IMAGES),
    (lambda a: a.decode_pose and a.multiscale, DECODE_POSE_NOT_WITH_MULTISCALE),
    (lambda a: a.peaks and a.train, PEAKS_IS_EVALUATION_ONLY),
    (lambda a: a.peaks and not a.predictions, PEAKS_NEEDS_PREDICTIONS),
    (lambda a: a.peaks and a.u8_images, PEAKS_NOT_WITH_U8_IMAGES),
    (lambda a: a.peaks and not 1 <= a.peaks <= 8, lambda a: '--peaks %d: 1 <= P <= 8' % a.peaks),
    (lambda a: a.tb_activations and not a.tb_dir, TB_ACTIVATIONS_NEEDS_TB_DIR),
    (lambda a: a.tb_activations and a.precision != 'fp32', TB_ACTIVATIONS_IS_FP32),
    (lambda a: a.render and not a.predict, RENDER_NEEDS_PREDICT),
    (lambda a: a.render_heat and not a.render, RENDER_HEAT_NEEDS_RENDER),
    (lambda a: a.render_heat == 'sm' and not a.use_sm, RENDER_HEAT_SM_NEEDS_USE_SM),
)
# The rules of --sequence, walked behind FLAG_RULES: a table of their own, so that the table above ends where the tests of earlier flags expect it to.
SEQUENCE_RULES = (
    (lambda a: a.sequence and not a.predict, SEQUENCE_NEEDS_PREDICT),
    (lambda a: a.sequence and a.zoom, SEQUENCE_NO_ZOOM),
    (lambda a: a.sequence and a.people != 1, SEQUENCE_ONE_PERSON),
    (lambda a: (a.seq_sigma is not None or a.seq_rho is not None) and not a.sequence, SEQ_OPTION_NEEDS_SEQUENCE),
)
# The rules of --augm_affine, walked behind SEQUENCE_RULES (a table of their own for the same reason).  --data_augm stays refused where it always was, in train_main.
AUGM_RULES = (
    (lambda a: a.augm_affine and not a.train, AUGM_AFFINE_NEEDS_TRAIN),
    (lambda a: (a.augm_scale is not None or a.augm_shift is not None or a.augm_pad is not None) and not a.augm_affine, AUGM_OPTION_NEEDS_AUGM_AFFINE),
    (lambda a: a.augm_scale is not None and not 0 < a.augm_scale[0] <= a.augm_scale[1] < float('inf'),
     lambda a: '--augm_scale %g %g: 0 < LO <= HI' % tuple(a.augm_scale)),
    (lambda a: a.augm_shift is not None and not 0 <= a.augm_shift < 0.5, lambda a: '--augm_shift %g: 0 <= F < 0.5' % a.augm_shift),
    (lambda a: a.augm_pad is not None and not 0 <= a.augm_pad <= 1, lambda a: '--augm_pad %g: 0 <= V <= 1' % a.augm_pad),
)
# The rules of --seq_people, walked behind AUGM_RULES (a table of their own for the same reason).  --people with --sequence stays refused above.
SEQ_PEOPLE_RULES = (
    (lambda a: a.seq_people is not None and not a.sequence, SEQ_PEOPLE_NEEDS_SEQUENCE),
    (lambda a: a.seq_people is not None and not a.use_sm, SEQ_PEOPLE_NEEDS_USE_SM),
    (lambda a: a.seq_people is not None and not 1 <= a.seq_people <= 4, lambda a: '--seq_people %d: 1 <= M <= 4' % a.seq_people),
    (lambda a: (a.seq_torso_sigma is not None or a.seq_exclude is not None) and a.seq_people is None, SEQ_PEOPLE_OPTION_NEEDS_SEQ_PEOPLE),
    (lambda a: a.seq_torso_sigma is not None and not 0 < a.seq_torso_sigma < float('inf'), lambda a: '--seq_torso_sigma %g: CELLS > 0' % a.seq_torso_sigma),
    (lambda a: a.seq_exclude is not None and not 0 <= a.seq_exclude <= 64, lambda a: '--seq_exclude %d: 0 <= CELLS <= 64' % a.seq_exclude),
)
# The rules of --synth_people, walked behind SEQ_PEOPLE_RULES (a table of their own for the same reason).
SYNTH_PEOPLE_RULES = (
    (lambda a: a.synth_people and a.synthetic, SYNTH_PEOPLE_NOT_WITH_SYNTHETIC),
    (lambda a: a.synth_people and a.predict, SYNTH_PEOPLE_NOT_WITH_PREDICT),
    (lambda a: a.synth_fresh and not (a.train and a.device_data and a.u8_images and a.synth_people), SYNTH_FRESH_NEEDS_COMPANIONS),
    (lambda a: a.synth_dump and not a.synth_people, SYNTH_DUMP_NEEDS_SYNTH_PEOPLE),
    (lambda a: a.synth_people and poses_problem(a.synth_people) is not None,      # (poses_problem remembers its answer per path)
     lambda a: '--synth_people %s: an [N,2,9] float64 array of at least five poses (data.py\'s xy) is expected; the file %s' % (a.synth_people, poses_problem(a.synth_people))),
)
# The rules of --sequence marginal and --seq_fit, walked behind SYNTH_PEOPLE_RULES (a table of their own for the same reason).
SEQ_SMOOTH_RULES = (
    (lambda a: a.seq_fit is not None and not a.sequence, SEQ_FIT_NEEDS_SEQUENCE),
    (lambda a: a.seq_fit is not None and not 1 <= a.seq_fit <= 100, lambda a: '--seq_fit %d: 1 <= ITERS <= 100' % a.seq_fit),
    (lambda a: a.seq_fit is not None and a.seq_people is not None, SEQ_FIT_NO_PEOPLE),
    (lambda a: a.sequence == 'marginal' and a.seq_people is not None, SEQ_MARGINAL_NO_PEOPLE),
)
# The rules of --seq_zoom, walked behind SEQ_SMOOTH_RULES (a table of their own for the same reason).  --zoom with --sequence stays refused above.
SEQ_ZOOM_RULES = (
    (lambda a: a.seq_zoom and not a.sequence, SEQ_ZOOM_NEEDS_SEQUENCE),
    (lambda a: a.seq_zoom and not a.use_sm, SEQ_ZOOM_NEEDS_USE_SM),
    (lambda a: a.seq_zoom and a.sequence == 'marginal', SEQ_ZOOM_NO_MARGINAL),
    (lambda a: a.seq_zoom and a.seq_fit is not None, SEQ_ZOOM_NO_FIT),
    (lambda a: a.seq_zoom and a.seq_people is not None, SEQ_ZOOM_NO_PEOPLE),
)
# The rules of --sequence lag and --seq_lag, walked behind SEQ_ZOOM_RULES (a table of their own for the same reason).
SEQ_LAG_RULES = (
    (lambda a: a.seq_lag is not None and a.sequence != 'lag', SEQ_LAG_NEEDS_SEQUENCE_LAG),
    (lambda a: a.sequence == 'lag' and a.seq_lag is None, SEQ_LAG_NEEDS_SEQ_LAG),
    (lambda a: a.seq_lag is not None and a.seq_lag < 1, lambda a: '--seq_lag %d: L >= 1 (lag 0 is --sequence filter)' % a.seq_lag),
    (lambda a: a.sequence == 'lag' and a.seq_people is not None, SEQ_LAG_NO_PEOPLE),
    (lambda a: a.sequence == 'lag' and a.seq_zoom, SEQ_LAG_NO_ZOOM),
)
# The rules of --seq_camera, walked behind SEQ_LAG_RULES (a table of their own for the same reason).
SEQ_CAMERA_RULES = (
    (lambda a: a.seq_camera_search is not None and not a.seq_camera, SEQ_CAMERA_SEARCH_NEEDS_SEQ_CAMERA),
    (lambda a: a.seq_camera and not a.sequence, SEQ_CAMERA_NEEDS_SEQUENCE),
    (lambda a: a.seq_camera and a.sequence in ('marginal', 'lag'), SEQ_CAMERA_NO_SMOOTHER),
    (lambda a: a.seq_camera and a.seq_fit is not None, SEQ_CAMERA_NO_FIT),
    (lambda a: a.seq_camera and a.seq_zoom, SEQ_CAMERA_NO_ZOOM),
    (lambda a: a.seq_camera and a.seq_people is not None, SEQ_CAMERA_NO_PEOPLE),
    (lambda a: a.seq_camera_search is not None and not 1 <= a.seq_camera_search <= 16, lambda a: '--seq_camera_search %d: 1 <= D <= 16' % a.seq_camera_search),
)
# The rules of --eval_scale / --scale_curve and of --augm_antialias, walked behind SEQ_CAMERA_RULES (a table of their own for the same reason).
EVAL_SCALE_RULES = (
    (lambda a: a.eval_scale is not None and not a.scale_curve, EVAL_SCALE_NEEDS_SCALE_CURVE),
    (lambda a: a.scale_curve and a.eval_scale is None, SCALE_CURVE_NEEDS_EVAL_SCALE),
    (lambda a: a.eval_scale is not None and (a.train or a.predict), EVAL_SCALE_IS_EVALUATION_ONLY),
    (lambda a: a.eval_scale is not None and (a.multiscale or a.flip_test or a.infer_torso or a.u8_images), EVAL_SCALE_SINGLE_SCALE_ONLY),
    (lambda a: a.eval_scale is not None and not all(0.25 <= s <= 4 for s in a.eval_scale),
     lambda a: '--eval_scale %s: 0.25 <= S <= 4' % ' '.join('%g' % s for s in a.eval_scale)),
    (lambda a: a.augm_antialias and not a.augm_affine, AUGM_ANTIALIAS_NEEDS_AUGM_AFFINE),
    (lambda a: a.augm_antialias and a.augm_scale is not None and a.augm_scale[0] < 0.25, AUGM_ANTIALIAS_SCALE_FLOOR),
)
# The rules of --seq_flow, walked behind EVAL_SCALE_RULES (a table of their own for the same reason).
SEQ_FLOW_RULES = (
    (lambda a: a.seq_flow_search is not None and a.seq_flow is None and not a.seq_flow_centre, SEQ_FLOW_SEARCH_NEEDS_SEQ_FLOW),
    (lambda a: a.seq_flow is not None and not a.sequence, SEQ_FLOW_NEEDS_SEQUENCE),
    (lambda a: a.seq_flow is not None and a.sequence == 'lag', SEQ_FLOW_NO_LAG),
    (lambda a: a.seq_flow is not None and a.seq_zoom, SEQ_FLOW_NO_ZOOM),
    (lambda a: a.seq_flow is not None and a.seq_people is not None, SEQ_FLOW_NO_PEOPLE),
    (lambda a: a.seq_flow is not None and not 1 <= a.seq_flow <= 4, lambda a: '--seq_flow %d: 1 <= N <= 4' % a.seq_flow),
    (lambda a: a.seq_flow_search is not None and not 1 <= a.seq_flow_search <= 16, lambda a: '--seq_flow_search %d: 1 <= D <= 16' % a.seq_flow_search),
)
# The rules of --seq_flow_centre, walked behind SEQ_FLOW_RULES (a table of their own for the same reason).
SEQ_FLOW_CENTRE_RULES = (
    (lambda a: a.seq_flow_centre and not a.sequence, SEQ_FLOW_CENTRE_NEEDS_SEQUENCE),
    (lambda a: a.seq_flow_centre and a.sequence in ('marginal', 'lag'), SEQ_FLOW_CENTRE_NO_SMOOTHER),
    (lambda a: a.seq_flow_centre and a.seq_fit is not None, SEQ_FLOW_CENTRE_NO_FIT),
    (lambda a: a.seq_flow_centre and a.seq_camera, SEQ_FLOW_CENTRE_NO_CAMERA),
    (lambda a: a.seq_flow_centre and a.seq_zoom, SEQ_FLOW_CENTRE_NO_ZOOM),
    (lambda a: a.seq_flow_centre and a.seq_people is not None, SEQ_FLOW_CENTRE_NO_PEOPLE),
)
# The rules of --seq_pose, walked behind SEQ_FLOW_CENTRE_RULES (a table of their own for the same reason).
SEQ_POSE_RULES = (
    (lambda a: a.seq_pose_weight is not None and a.seq_pose is None, SEQ_POSE_WEIGHT_NEEDS_SEQ_POSE),
    (lambda a: a.seq_pose is not None and not a.predict, SEQ_POSE_NEEDS_PREDICT),
    (lambda a: a.seq_pose is not None and not a.use_sm, SEQ_POSE_NEEDS_USE_SM),
    (lambda a: a.seq_pose is not None and a.sequence != 'viterbi', SEQ_POSE_NEEDS_VITERBI),
    (lambda a: a.seq_pose is not None and not 1 <= a.seq_pose <= 4, lambda a: '--seq_pose %d: 1 <= P <= 4' % a.seq_pose),
    (lambda a: a.seq_pose_weight is not None and not (np.isfinite(a.seq_pose_weight) and a.seq_pose_weight >= 0),
     lambda a: '--seq_pose_weight %r: W is finite and >= 0' % a.seq_pose_weight),
    (lambda a: a.seq_pose is not None and a.seq_people is not None, SEQ_POSE_NO_PEOPLE),
    (lambda a: a.seq_pose is not None and a.seq_zoom, SEQ_POSE_NO_ZOOM),
    (lambda a: a.seq_pose is not None and a.seq_camera, SEQ_POSE_NO_CAMERA),
    (lambda a: a.seq_pose is not None and a.seq_flow is not None, SEQ_POSE_NO_FLOW),
    (lambda a: a.seq_pose is not None and a.seq_flow_centre, SEQ_POSE_NO_FLOW_CENTRE),
    (lambda a: a.seq_pose is not None and a.seq_fit is not None, SEQ_POSE_NO_FIT),
)


def main(argv=None):
    global hps
    args = build_parser().parse_args(argv)
    hps = args
    for holds, message in FLAG_RULES + SEQUENCE_RULES + AUGM_RULES + SEQ_PEOPLE_RULES + SYNTH_PEOPLE_RULES + SEQ_SMOOTH_RULES + SEQ_ZOOM_RULES + SEQ_LAG_RULES + SEQ_CAMERA_RULES + EVAL_SCALE_RULES + SEQ_FLOW_RULES + SEQ_FLOW_CENTRE_RULES + SEQ_POSE_RULES:
        if holds(args):
            raise SystemExit(message(args) if callable(message) else message)
    for g in args.gpus:      # after the rules: a refused combination is reported as such on a machine without the device too
        if g < 0 or g >= torch.cuda.device_count():
            raise SystemExit('--gpus %s: device %d does not exist (%d visible)' % (args.gpus, g, torch.cuda.device_count()))
    if args.predict:
        predict_main(args)
    elif args.train:
        train_main(args)
    else:
        eval_run.run(args)


if __name__ == '__main__':
    main()
