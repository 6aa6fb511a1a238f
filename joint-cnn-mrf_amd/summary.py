"""TensorBoard summaries of the training run (reference: tensorboard.py; main.py:586-601,620-660), without TensorFlow.

Event files are TFRecord files of hand-encoded `Event` protobuf messages (the same kind of job as tf_checkpoint.py);
PNG images are written with the stdlib zlib on a small thread pool.  The tensor work runs in libjcm's HIP kernels
(csrc/summary.hip): histogram statistics of the parameters and gradients are taken in place on the device, the heat-map
overlays and every image are quantised there, and only the finished uint8 pictures and the per-tensor counts reach the host.

The function names mirror tensorboard.py (colorize, var_summary, main_summaries, show_img_plus_hm, run_summary,
write_summary); the tags follow TF-1.x's rules (DESIGN.md 4.8 lists them all).
"""
import os
import socket
import struct
import threading
import time
import zlib
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from . import _lib
from .tf_checkpoint import crc32c, mask_crc

N_IMG_TO_SHOW = 20          # tensorboard.py:3
N_INPUT_TO_SHOW = 30        # main.py:583,586-587
PNG_LEVEL = 1               # zlib level: the decoded pictures do not depend on it; 1 keeps the per-epoch pass short
MAX_PNG_THREADS = 16
DBL_MAX = np.finfo(np.float64).max
JOINT_NAMES = ('lsho', 'lelb', 'lwri', 'rsho', 'relb', 'rwri', 'lhip', 'rhip', 'nose')
# colorize (tensorboard.py:6-19): which of R, G, B carry a joint's heat map
COLOR_CHANNELS = {'nose': (1, 0, 0), 'lsho': (0, 1, 0), 'rsho': (0, 1, 0), 'lelb': (0, 0, 1), 'relb': (0, 0, 1),
                  'lwri': (1, 1, 0), 'rwri': (1, 1, 0), 'lhip': (1, 0, 1), 'rhip': (1, 0, 1)}


# ------------------------------------------------------------------ TF-1.x histogram buckets (core/lib/histogram/histogram.cc)
def bucket_limits():
    """InitDefaultBucketsInner: 1e-12 * 1.1^k below 1e20, then DBL_MAX, mirrored, 0.0 in the middle (1551 limits)."""
    pos = []
    v = 1.0e-12
    while v < 1.0e20:
        pos.append(v)
        v *= 1.1
    pos.append(DBL_MAX)
    return np.array([-p for p in reversed(pos)] + [0.0] + pos, np.float64)


_LIMITS = bucket_limits()


def encode_histogram(hmin, hmax, num, hsum, hsum_sq, buckets, limits=_LIMITS):
    """Histogram::EncodeToProto(preserve_zero_buckets=false) -> HistogramProto bytes: every run of empty buckets becomes one
    entry that carries the run's last limit."""
    b = np.asarray(buckets, np.float64)
    z = b <= 0
    keep = ~z | np.append(~z[1:], True)
    lim, cnt = limits[keep], b[keep]
    if lim.size == 0:
        lim, cnt = np.array([DBL_MAX]), np.array([0.0])
    return histogram_proto(hmin, hmax, num, hsum, hsum_sq, lim, cnt)


# ------------------------------------------------------------------ protobuf wire format
def _varint(n):
    n &= 0xffffffffffffffff
    out = bytearray()
    while True:
        b = n & 0x7f
        n >>= 7
        if n:
            out.append(b | 0x80)
        else:
            out.append(b)
            return bytes(out)


def _key(field, wire):
    return _varint((field << 3) | wire)


def _f_bytes(field, data):
    return _key(field, 2) + _varint(len(data)) + data


def _f_double(field, v):
    return _key(field, 1) + struct.pack('<d', float(v))


def _f_float(field, v):
    return _key(field, 5) + struct.pack('<f', float(v))


def _f_int(field, v):
    return _key(field, 0) + _varint(int(v))


def histogram_proto(hmin, hmax, num, hsum, hsum_sq, bucket_limit, bucket):
    """HistogramProto: min 1, max 2, num 3, sum 4, sum_squares 5 (double); bucket_limit 6, bucket 7 (packed double)."""
    bl = np.ascontiguousarray(bucket_limit, '<f8').tobytes()
    bc = np.ascontiguousarray(bucket, '<f8').tobytes()
    return (_f_double(1, hmin) + _f_double(2, hmax) + _f_double(3, num) + _f_double(4, hsum) + _f_double(5, hsum_sq)
            + _f_bytes(6, bl) + _f_bytes(7, bc))


def image_proto(height, width, colorspace, png):
    """Summary.Image: height 1, width 2, colorspace 3, encoded_image_string 4."""
    return _f_int(1, height) + _f_int(2, width) + _f_int(3, colorspace) + _f_bytes(4, png)


def value_simple(tag, v):
    """Summary.Value: tag 1, simple_value 2 (float)."""
    return _f_bytes(1, tag.encode()) + _f_float(2, v)


def value_image(tag, img):
    return _f_bytes(1, tag.encode()) + _f_bytes(4, img)


def value_histo(tag, histo):
    return _f_bytes(1, tag.encode()) + _f_bytes(5, histo)


def summary_proto(values):
    """Summary: repeated Value value = 1."""
    return b''.join(_f_bytes(1, v) for v in values)


def event_proto(wall_time, step, file_version=None, summary=None):
    """Event: wall_time 1 (double), step 2 (int64), file_version 3, summary 5."""
    out = _f_double(1, wall_time) + _f_int(2, step)
    if file_version is not None:
        out += _f_bytes(3, file_version.encode())
    if summary is not None:
        out += _f_bytes(5, summary)
    return out


def tfrecord(data):
    """TFRecord framing: u64 length, masked CRC-32C of the length, data, masked CRC-32C of the data."""
    header = struct.pack('<Q', len(data))
    return header + struct.pack('<I', mask_crc(crc32c(header))) + data + struct.pack('<I', mask_crc(crc32c(data)))


class FileWriter:
    """tf.summary.FileWriter(logdir, flush_secs=30): events.out.tfevents.<time>.<hostname>, first record file_version
    'brain.Event:2'; the file is flushed at least every flush_secs seconds and on close."""

    def __init__(self, logdir, flush_secs=30):
        os.makedirs(logdir, exist_ok=True)
        now = time.time()
        self.path = os.path.join(logdir, 'events.out.tfevents.%010d.%s' % (int(now), socket.gethostname()))
        self._f = open(self.path, 'wb')
        self._lock = threading.Lock()
        self._write(event_proto(now, 0, file_version='brain.Event:2'))
        self.flush()
        self._stop = threading.Event()
        self._flusher = threading.Thread(target=self._flush_loop, args=(float(flush_secs),), daemon=True)
        self._flusher.start()

    def _write(self, event):
        with self._lock:
            self._f.write(tfrecord(event))

    def _flush_loop(self, secs):
        while not self._stop.wait(secs):
            self.flush()

    def add_event(self, event):
        self._write(event)

    def add_summary(self, summary, global_step):
        self._write(event_proto(time.time(), int(global_step), summary=summary))

    def flush(self):
        with self._lock:
            if not self._f.closed:
                self._f.flush()

    def close(self):
        self._stop.set()
        with self._lock:
            if not self._f.closed:
                self._f.close()


# ------------------------------------------------------------------ PNG (stdlib zlib)
def _png_chunk(kind, data):
    return struct.pack('>I', len(data)) + kind + data + struct.pack('>I', zlib.crc32(kind + data) & 0xffffffff)


def encode_png(img, level=PNG_LEVEL):
    """uint8 [H,W,C], C = 1 (gray) or 3 (RGB) -> PNG bytes (8 bit, every row with the Sub filter)."""
    img = np.ascontiguousarray(img, np.uint8)
    h, w, c = img.shape
    raw = img.reshape(h, w * c)
    rows = np.empty((h, w * c + 1), np.uint8)
    rows[:, 0] = 1
    rows[:, 1:1 + c] = raw[:, :c]
    np.subtract(raw[:, c:], raw[:, :-c], out=rows[:, 1 + c:])
    ihdr = struct.pack('>IIBBBBB', w, h, 8, {1: 0, 3: 2}[c], 0, 0, 0)
    return (b'\x89PNG\r\n\x1a\n' + _png_chunk(b'IHDR', ihdr) + _png_chunk(b'IDAT', zlib.compress(rows.tobytes(), level))
            + _png_chunk(b'IEND', b''))


_pool = None


def png_pool():
    global _pool
    if _pool is None:
        _pool = ThreadPoolExecutor(max_workers=max(1, min(MAX_PNG_THREADS, os.cpu_count() or 1)))
    return _pool


def _image_values(tag, u8, max_outputs):
    """tf.summary.image(tag, ., max_outputs) on a quantised host batch u8 [N,H,W,C] -> futures of Summary.Value bytes."""
    n = min(u8.shape[0], max_outputs)

    def one(i):
        t = '%s/image/%d' % (tag, i) if max_outputs > 1 else tag + '/image'
        return value_image(t, image_proto(u8.shape[1], u8.shape[2], u8.shape[3], encode_png(u8[i])))
    return [png_pool().submit(one, i) for i in range(n)]


def _host(eng, t):
    torch.cuda.current_stream(eng.device).wait_stream(eng._stream)
    return t.cpu().numpy()


# ------------------------------------------------------------------ mirrors of tensorboard.py
def colorize(hm, joint_name):
    """tensorboard.py:6-19 on a numpy [..., 1] heat map."""
    z = np.zeros_like(hm)
    return np.concatenate([hm if m else z for m in COLOR_CHANNELS[joint_name]], axis=-1)


def check_finite(tag, counts_row):
    if int(counts_row[2]):
        raise ValueError('Nan in summary histogram for: %s (%d non-finite values)' % (tag, int(counts_row[2])))


def histogram_value(tag, stats_row, counts_row):
    """tf.summary.histogram(tag, .) from one row of Engine.tensor_stats."""
    check_finite(tag, counts_row)
    return value_histo(tag, encode_histogram(stats_row[0], stats_row[1], float(counts_row[0]), stats_row[2], stats_row[3], counts_row[3:]))


def var_summary(stats_row, counts_row, size, name, baisc_name='pre_activ_'):
    """tensorboard.py:22-34: max, mean, min, std, n_pos (fraction > 0) and the histogram under the scope baisc_name + name."""
    scope = baisc_name + name
    check_finite(scope + '/histogram', counts_row)
    n = max(int(counts_row[0]), 1)
    mean = stats_row[2] / n
    std = np.sqrt(max(stats_row[3] / n - mean * mean, 0.0))
    return [value_simple(scope + '/max', stats_row[1]), value_simple(scope + '/mean', mean), value_simple(scope + '/min', stats_row[0]),
            value_simple(scope + '/std', std), value_simple(scope + '/n_pos', float(counts_row[1]) / max(size, 1)),
            histogram_value(scope + '/histogram', stats_row, counts_row)]


def main_summaries(eng, layout, grads=None, params_flat=None, clip_norm=4.0, images=True):
    """tensorboard.py:37-57.  layout: [(name, offset, count)] of the trainable tensors (jcm_train_param_info order).
    grads: the flat tower-averaged gradient buffer of the last update (None: no gradient summaries), histogrammed after the
    clip factor of that update; params_flat: the parameters as one flat device buffer, or None to read the engine's stored
    trainable tensors in place.  Returns Summary.Value bytes and futures (images)."""
    out = []
    if grads is not None:
        sel = [(n, o, c) for n, o, c in layout if 'weights' in n or 'energy' in n]
        st, cn = eng.tensor_stats(grads, [(o, c) for _, o, c in sel], clip_norm=clip_norm)
        for (n, _, _), s, c in zip(sel, st, cn):
            out.append(histogram_value('grads/%s/gradients' % n, s, c))
            out.append(value_simple('grads/%s/gradients_1' % n, np.sqrt(s[3])))        # tf.norm; the scope name is taken: '_1'
    st, cn = eng.tensor_stats(params_flat, [(o, c) for _, o, c in layout])
    for (n, _, _), s, c in zip(layout, st, cn):
        out.append(histogram_value('grads/' + n, s, c))
    if images:
        off, cnt = next((o, c) for n, o, c in layout if n == 'conv1_fullres/weights')
        w = _param_tensor(eng, 'conv1_fullres/weights', cnt, params_flat, off).view(5, 5, 3, cnt // 75).permute(3, 0, 1, 2).contiguous()
        out += _image_values('conv_filters_1/w_conv1', _host(eng, eng.image_u8(w)), N_IMG_TO_SHOW)
    return out


def _param_tensor(eng, name, count, params_flat=None, offset=0):
    if params_flat is not None:
        return params_flat[offset:offset + count]
    buf = torch.empty(count, dtype=torch.float32, device=eng.device)
    _lib.check(eng._lib.jcm_get_tensor(eng._h, name.encode(), eng._p(buf), count), 'jcm_get_tensor(%s)' % name)
    return buf


def show_img_plus_hm(eng, x, hm, joint_names, in_height, in_width, hm_name):
    """tensorboard.py:60-71: x [B,H,W,3], hm [B,h,w,9] device tensors -> image values 'hm_<hm_name>_<joint>' and
    'img_plus_all_joints_<hm_name>' for the first N_IMG_TO_SHOW images."""
    if list(joint_names) != list(JOINT_NAMES) or tuple(x.shape[1:3]) != (in_height, in_width):
        raise ValueError('show_img_plus_hm: the overlay kernel knows the reference joints %s at the image size of x' % (JOINT_NAMES,))
    u8 = _host(eng, eng.hm_overlay(x, hm.contiguous(), min(x.shape[0], N_IMG_TO_SHOW)))      # [n,10,H,W,3]
    out = []
    for j, name in enumerate(joint_names):
        out += _image_values('hm_{}_{}'.format(hm_name, name), u8[:, j], N_IMG_TO_SHOW)
    out += _image_values('img_plus_all_joints_' + hm_name, u8[:, len(joint_names)], N_IMG_TO_SHOW)
    return out


def pairwise_summaries(eng, layout, params_flat=None, images=True):
    """main.py:588-593: the images of every pairwise energy and bias and their var_summary (scope 'pre_activ_pairwise_...')."""
    keys = [n[len('energy_'):] for n, _, _ in layout if n.startswith('energy_')]
    where = {n: (o, c) for n, o, c in layout}
    out = []
    if not keys:
        return out
    segs = []
    for k in keys:
        segs += [where['energy_' + k], where['bias_' + k]]
    st, cn = eng.tensor_stats(params_flat, segs)
    if not images:
        for i, k in enumerate(keys):
            out += var_summary(st[2 * i], cn[2 * i], segs[2 * i][1], 'pairwise_energies_' + k)
            out += var_summary(st[2 * i + 1], cn[2 * i + 1], segs[2 * i + 1][1], 'pairwise_biases_' + k)
        return out
    e = torch.stack([_param_tensor(eng, 'energy_' + k, where['energy_' + k][1], params_flat, where['energy_' + k][0]) for k in keys])
    b = torch.stack([_param_tensor(eng, 'bias_' + k, where['bias_' + k][1], params_flat, where['bias_' + k][0]) for k in keys])
    eu8 = _host(eng, eng.image_u8(e.view(len(keys), 120, 180, 1)))
    bu8 = _host(eng, eng.image_u8(b.view(len(keys), 60, 90, 1)))
    for i, k in enumerate(keys):
        out += _image_values('pairwise_potential_' + k, eu8[i:i + 1], N_INPUT_TO_SHOW)
        out += _image_values('pairwise_biases_' + k, bu8[i:i + 1], N_INPUT_TO_SHOW)
        out += var_summary(st[2 * i], cn[2 * i], segs[2 * i][1], 'pairwise_energies_' + k)
        out += var_summary(st[2 * i + 1], cn[2 * i + 1], segs[2 * i + 1][1], 'pairwise_biases_' + k)
    return out


# the order in which model (main.py:43-72) calls conv_layer
ACTIV_SCOPES = tuple('conv%d_%s' % (i, r) for r in ('fullres', 'halfres', 'quarterres') for i in (1, 2, 3, 4)) + ('conv5', 'conv6')
ACTIV_CHANNEL = 7           # main.py:168: activ[:, :, :, 7:8]
N_ACTIV_TO_SHOW = 3         # ... max_outputs = 3


def tower_slices(n_images, n_towers):
    """(images per tower, images used): tower i takes images [i * per, (i + 1) * per) of the batch; the n_images % n_towers
    trailing images are left out, as the reference's tower loop leaves them out (main.py:511,516)."""
    if n_towers < 1 or n_images < n_towers:
        raise ValueError('%d images do not fill %d towers' % (n_images, n_towers))
    per = n_images // n_towers
    return per, per * n_towers


def activ_tags(n_towers, n_per_tower, scopes=ACTIV_SCOPES):
    """Every tag activation_summaries emits, in its order: tower by tower, scope by scope, var_summary's six then the pictures."""
    tags = []
    for i in range(n_towers):
        for s in scopes:
            tags += ['tower_%d/pre_activ_%s/%s' % (i, s, k) for k in ('max', 'mean', 'min', 'std', 'n_pos', 'histogram')]
            tags += ['tower_%d/f_activ_%s/image/%d' % (i, s, k) for k in range(min(N_ACTIV_TO_SHOW, n_per_tower))]
    return tags


def activation_summaries(eng, x, n_towers=1, taps=None):
    """tb.var_summary(pre_activ, name) and tf.summary.image('f_activ_' + name, activ[:, :, :, 7:8], 3) of every conv_layer of model
    (main.py:167-168) inside tf.name_scope('tower_%d') (main.py:519): x [B,H,W,3] float32, the summary batch (device); tower i is the
    slice [i * per, (i + 1) * per) of it, per = B // n_towers.  The graph of model is composed line for line as main.model_layerwise
    composes it, every conv_layer as Engine.conv_layer_pre followed by Engine.act_summary; one layer's tensors live at a time.
    taps: a dict whose keys name scopes -- it receives those scopes' pre-activations (device).  Returns Summary.Value bytes and
    futures (pictures), tower by tower, in the order in which model calls conv_layer."""
    eng._chk(x, 4, 'x')
    per, used = tower_slices(x.shape[0], n_towers)
    n_pics = min(N_ACTIV_TO_SHOW, per)
    x = x[:used]
    found = {}

    def conv_layer(t, stride, name):
        n_out = _conv_out_channels(eng, name)
        z = eng.conv_layer_pre(t, name, stride, n_out)
        if taps is not None and name in taps:
            taps[name] = z
        r = eng.act_summary(z, name, n_groups=n_towers, pic_channel=ACTIV_CHANNEL, n_pics=n_pics)
        u8 = _host(eng, eng.image_u8(r['pics'].view(n_towers * n_pics, z.shape[1], z.shape[2], 1)))
        found[name] = (r['stats'], r['counts'], per * z.shape[1] * z.shape[2] * z.shape[3], u8)
        return r['activ']

    def branch(t, res):
        t = conv_layer(t, 2, 'conv1_' + res)
        t = eng.max_pool(t)
        t = conv_layer(t, 1, 'conv2_' + res)
        t = eng.max_pool(t)
        t = conv_layer(t, 1, 'conv3_' + res)
        return conv_layer(t, 1, 'conv4_' + res)

    H, W = int(x.shape[1]), int(x.shape[2])
    x1 = branch(x, 'fullres')
    x2 = branch(eng.resize_bilinear(x, H // 2, W // 2), 'halfres')
    x2 = eng.resize_bilinear(x2, int(x1.shape[1]), int(x1.shape[2]))
    x3 = branch(eng.resize_bilinear(x, H // 4, W // 4), 'quarterres')
    x3 = eng.resize_bilinear(x3, int(x1.shape[1]), int(x1.shape[2]))
    with torch.cuda.stream(eng._stream):
        t = x1 + x2 + x3
        t /= 3
    del x1, x2, x3
    t = conv_layer(t, 1, 'conv5')
    conv_layer(t, 1, 'conv6')
    out = []
    for i in range(n_towers):
        for name in ACTIV_SCOPES:
            st, cn, size, u8 = found[name]
            out += var_summary(st[i], cn[i], size, name, baisc_name='tower_%d/pre_activ_' % i)
            out += _image_values('tower_%d/f_activ_%s' % (i, name), u8[i * n_pics:(i + 1) * n_pics], N_ACTIV_TO_SHOW)
    return out


def _conv_out_channels(eng, name):
    shape = eng._shapes.get(name + '/weights')
    if shape is None or len(shape) != 4:
        raise ValueError("no conv layer '%s' among the engine's parameters" % name)
    return shape[3]


def merged_summary(eng, layout, x=None, y=None, use_sm=True, n_joints=9, grads=None, params_flat=None, clip_norm=4.0, images=True,
                   activations=False, n_towers=1):
    """tf.summary.merge_all() of the reference graph (main.py:586-597) -> Summary bytes.  x [B,H,W,3], y [B,h,w,K+1]: the
    summary batch (device); images=False leaves out every image (the per-iteration summaries).  The heat maps are the
    inference-mode tower's (flag_train=False); without the spatial model its pictures repeat the part detector's.
    activations=True appends activation_summaries(eng, x, n_towers) -- the per-layer tags of main.py:167-168 -- behind the other
    values; off (the default), the bytes are what they were without the switch."""
    vals = []
    if images:
        vals += _image_values('input', _host(eng, eng.image_u8(x)), N_INPUT_TO_SHOW)
    if use_sm:
        vals += pairwise_summaries(eng, layout, params_flat, images)
    vals += main_summaries(eng, layout, grads, params_flat, clip_norm, images)
    if images:
        r = eng.eval_forward(x, y, use_sm=use_sm, want_prob=True)
        H, W = x.shape[1], x.shape[2]
        vals += show_img_plus_hm(eng, x, y[..., :n_joints], JOINT_NAMES, H, W, 'target')
        vals += show_img_plus_hm(eng, x, r['pd_prob'], JOINT_NAMES, H, W, 'pred_part_detector')
        vals += show_img_plus_hm(eng, x, r['sm_prob'] if use_sm else r['pd_prob'], JOINT_NAMES, H, W, 'pred_spatial_model')
    if activations:
        if x is None:
            raise ValueError('activations=True needs the summary batch x')
        vals += activation_summaries(eng, x, n_towers)
    return summary_proto([v.result() if hasattr(v, 'result') else v for v in vals])


def run_summary(writer, summary, cur_iter):
    """tensorboard.py:37-39: one event with the merged summary at step cur_iter."""
    writer.add_summary(summary, cur_iter)


def write_summary(writer, vals, names, cur_iter):
    """tensorboard.py:74-78: one event per scalar."""
    for val, name in zip(vals, names):
        writer.add_summary(summary_proto([value_simple(name, val)]), cur_iter)


def flat_params(eng, params):
    """Evaluation runs (no training state): the trainable tensors -- every parameter but the BatchNorm moving statistics, in
    ascending name order, the library's layout -- as one flat device buffer and its [(name, offset, count)] layout."""
    names = sorted(k for k in params if not (k.endswith('moving_mean') or k.endswith('moving_variance')))
    layout, off = [], 0
    for n in names:
        c = int(np.asarray(params[n]).size)
        layout.append((n, off, c))
        off += c
    buf = torch.empty(off, dtype=torch.float32, device=eng.device)
    for n, o, c in layout:
        _lib.check(eng._lib.jcm_get_tensor(eng._h, n.encode(), eng._p(buf[o:o + c]), c), 'jcm_get_tensor(%s)' % n)
    return buf, layout
