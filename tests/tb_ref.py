"""Independent readers and numpy restatements for the summary tests (shares no code with joint_cnn_mrf_amd/summary.py).

- a TFRecord reader and a protobuf wire decoder for Event / Summary / HistogramProto / Image;
- TF-1.x's default histogram bucket table and Histogram::EncodeToProto;
- NormalizeFloatImage (summary_image_op.cc) and show_img_plus_hm (tensorboard.py:60-71), the latter in a float32
  step-by-step version (the kernel's operation order) and a float64 version, on oracle.resize_bilinear_tf1.
"""
import struct
import sys

import numpy as np

# ------------------------------------------------------------------ CRC-32C, bitwise (no table shared with the writer)
_POLY = 0x82F63B78


def crc32c(data):
    c = 0xffffffff
    for b in bytes(data):
        c ^= b
        for _ in range(8):
            c = (c >> 1) ^ (_POLY if c & 1 else 0)
    return c ^ 0xffffffff


def masked(crc):
    return ((((crc >> 15) | (crc << 17)) & 0xffffffff) + 0xa282ead8) & 0xffffffff


def read_records(path, check_crc=True):
    """TFRecord file -> list of payloads; checks both masked CRCs (the data CRC only on payloads < 64 KB, bitwise is slow)."""
    out = []
    with open(path, 'rb') as f:
        buf = f.read()
    pos = 0
    while pos < len(buf):
        header = buf[pos:pos + 8]
        (n,) = struct.unpack('<Q', header)
        (hcrc,) = struct.unpack('<I', buf[pos + 8:pos + 12])
        data = buf[pos + 12:pos + 12 + n]
        (dcrc,) = struct.unpack('<I', buf[pos + 12 + n:pos + 16 + n])
        if check_crc:
            assert hcrc == masked(crc32c(header)), 'length CRC mismatch at %d' % pos
            if n < 65536:
                assert dcrc == masked(crc32c(data)), 'data CRC mismatch at %d' % pos
        assert len(data) == n
        out.append(data)
        pos += 16 + n
    return out


# ------------------------------------------------------------------ protobuf wire decoder
def _varint(b, i):
    r = s = 0
    while True:
        c = b[i]
        i += 1
        r |= (c & 0x7f) << s
        s += 7
        if not c & 0x80:
            return r, i


def fields(b):
    """message bytes -> list of (field number, wire type, value); value = int (0), bytes (2), raw 8 / 4 bytes (1 / 5)."""
    out, i = [], 0
    while i < len(b):
        k, i = _varint(b, i)
        f, w = k >> 3, k & 7
        if w == 0:
            v, i = _varint(b, i)
        elif w == 1:
            v, i = b[i:i + 8], i + 8
        elif w == 5:
            v, i = b[i:i + 4], i + 4
        elif w == 2:
            n, i = _varint(b, i)
            v, i = b[i:i + n], i + n
        else:
            raise ValueError('wire type %d' % w)
        out.append((f, w, v))
    return out


def _d(v):
    return struct.unpack('<d', v)[0]


def parse_histo(b):
    h = {'min': 0.0, 'max': 0.0, 'num': 0.0, 'sum': 0.0, 'sum_squares': 0.0, 'bucket_limit': [], 'bucket': []}
    for f, w, v in fields(b):
        if f in (1, 2, 3, 4, 5):
            h[['min', 'max', 'num', 'sum', 'sum_squares'][f - 1]] = _d(v)
        elif f in (6, 7):
            key = 'bucket_limit' if f == 6 else 'bucket'
            if w == 2:
                h[key] += list(struct.unpack('<%dd' % (len(v) // 8), v))
            else:
                h[key].append(_d(v))
    return h


def parse_image(b):
    im = {'height': 0, 'width': 0, 'colorspace': 0, 'png': b''}
    for f, w, v in fields(b):
        if f == 1:
            im['height'] = v
        elif f == 2:
            im['width'] = v
        elif f == 3:
            im['colorspace'] = v
        elif f == 4:
            im['png'] = v
    return im


def parse_value(b):
    val = {}
    for f, w, v in fields(b):
        if f == 1:
            val['tag'] = v.decode()
        elif f == 2:
            val['simple_value'] = struct.unpack('<f', v)[0]
        elif f == 4:
            val['image'] = parse_image(v)
        elif f == 5:
            val['histo'] = parse_histo(v)
    return val


def parse_event(b):
    ev = {'wall_time': 0.0, 'step': 0, 'values': []}
    for f, w, v in fields(b):
        if f == 1:
            ev['wall_time'] = _d(v)
        elif f == 2:
            ev['step'] = v if v < 1 << 63 else v - (1 << 64)
        elif f == 3:
            ev['file_version'] = v.decode()
        elif f == 5:
            ev['values'] += [parse_value(x) for ff, _, x in fields(v) if ff == 1]
    return ev


def read_events(path, check_crc=True):
    return [parse_event(r) for r in read_records(path, check_crc)]


# ------------------------------------------------------------------ histogram.cc
def default_limits():
    pos, v = [], 1.0e-12
    while v < 1.0e20:
        pos.append(v)
        v = v * 1.1
    pos.append(sys.float_info.max)
    return np.array([-p for p in pos[::-1]] + [0.0] + pos)


def histogram(values, limits=None):
    """Histogram::Add over float64 values: (min, max, num, sum, sum_squares, bucket counts)."""
    limits = default_limits() if limits is None else limits
    v = np.asarray(values, np.float64).reshape(-1)
    counts = np.bincount(np.searchsorted(limits, v, side='right'), minlength=limits.size)
    mn = v.min() if v.size else sys.float_info.max
    mx = v.max() if v.size else -sys.float_info.max
    return mn, mx, float(v.size), float(v.sum()), float((v * v).sum()), counts


def encode_to_proto(counts, limits=None):
    """Histogram::EncodeToProto(preserve_zero_buckets=false): the (bucket_limit, bucket) lists, loop as written in TF."""
    limits = default_limits() if limits is None else limits
    bl, bc = [], []
    i = 0
    while i < len(counts):
        end, cnt = limits[i], counts[i]
        i += 1
        if cnt <= 0:
            while i < len(counts) and counts[i] <= 0:
                end, cnt = limits[i], counts[i]
                i += 1
        bl.append(float(end))
        bc.append(float(cnt))
    if not bl:
        bl, bc = [sys.float_info.max], [0.0]
    return bl, bc


# ------------------------------------------------------------------ summary_image_op.cc
def normalize_float_image(img):
    """NormalizeFloatImage for one float32 [H,W,C] image -> uint8 [H,W,C]."""
    img = np.asarray(img, np.float32)
    fin = np.isfinite(img).all(axis=-1)
    vals = img[fin]
    mn = np.float32(vals.min()) if vals.size else np.float32(np.inf)
    mx = np.float32(vals.max()) if vals.size else np.float32(-np.inf)
    if mn < 0:
        mv = max(abs(mn), abs(mx))
        scale = np.float32(0) if mv < np.float32(1e-6) else np.float32(127) / np.float32(mv)
        offset = np.float32(128)
    else:
        scale = np.float32(0) if mx < np.float32(1e-6) else np.float32(255) / mx
        offset = np.float32(0)
    with np.errstate(invalid='ignore', over='ignore'):
        q = (img * scale).astype(np.float32) + offset
        out = np.clip(np.nan_to_num(q, nan=0.0), 0, 255).astype(np.uint8)
    bad = np.zeros(img.shape[-1], np.uint8)
    bad[0] = 255
    out[~fin] = bad
    return out


# ------------------------------------------------------------------ tensorboard.py:60-71
COLOR = [(0, 1, 0), (0, 0, 1), (1, 1, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (1, 0, 1), (1, 0, 0)]


def show_img_plus_hm(x, hm, dtype=np.float32):
    """The ten float pictures per image: [B,10,H,W,3]; dtype float32 = the kernel's operation order, float64 = the exact values."""
    from oracle.jcm_oracle import resize_bilinear_tf1
    x = np.asarray(x, dtype)
    hm = np.asarray(hm, dtype)
    B, H, W, _ = x.shape
    with np.errstate(divide='ignore', invalid='ignore'):
        cx = (dtype(1) / np.max(np.where(np.isnan(x), -np.inf, x), axis=(1, 2, 3), keepdims=True)).astype(dtype)
        chm = (dtype(1) / np.max(np.where(np.isnan(hm), -np.inf, hm), axis=(1, 2), keepdims=True)).astype(dtype)
        large = (chm * resize_bilinear_tf1(hm, H, W)).astype(dtype)
        pics = np.empty((B, 10, H, W, 3), dtype)
        acc = (cx * x).astype(dtype)
        for j in range(9):
            c = np.concatenate([large[..., j:j + 1] if m else np.zeros_like(large[..., :1]) for m in COLOR[j]], axis=-1)
            pics[:, j] = np.minimum(x + c, dtype(1))
            acc = np.minimum(acc + c, dtype(1))
        pics[:, 9] = acc
    return pics


def overlay_u8(x, hm, dtype=np.float32):
    pics = show_img_plus_hm(x, hm, dtype)
    out = np.empty(pics.shape, np.uint8)
    for b in range(pics.shape[0]):
        for p in range(pics.shape[1]):
            out[b, p] = normalize_float_image(pics[b, p].astype(np.float32) if dtype == np.float32 else pics[b, p])
    return out
