"""CPU checks of the TensorBoard event writer (joint_cnn_mrf_amd/summary.py) against the independent decoder of tests/tb_ref.py."""
import io
import os
import struct
import sys

import numpy as np
import pytest

import joint_cnn_mrf_amd  # noqa: F401
from joint_cnn_mrf_amd import summary as S

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tb_ref as R  # noqa: E402


def test_bucket_table():
    lim = S.bucket_limits()
    assert lim.size == 1551
    assert np.array_equal(lim, R.default_limits())
    mid = lim.size // 2
    assert lim[mid] == 0.0
    assert lim[mid + 1] == 1e-12 and lim[mid - 1] == -1e-12
    assert lim[-1] == sys.float_info.max and lim[0] == -sys.float_info.max
    assert np.array_equal(lim, -lim[::-1])
    assert np.all(np.diff(lim) > 0)


def test_library_bucket_table_matches():
    import ctypes
    from joint_cnn_mrf_amd import _lib
    lib = _lib.load()
    n = lib.jcm_hist_bucket_limits(None, 0)
    assert n == _lib.JCM_HIST_BUCKETS == 1551
    out = (ctypes.c_double * n)()
    assert lib.jcm_hist_bucket_limits(out, n) == n
    assert np.array_equal(np.frombuffer(out, np.float64), R.default_limits())
    assert lib.jcm_hist_bucket_limits(out, n - 1) == -1


def test_tfrecord_framing_crcs(tmp_path):
    w = S.FileWriter(str(tmp_path / 'run'))
    w.add_summary(S.summary_proto([S.value_simple('a/b', 1.5)]), 7)
    w.add_summary(S.summary_proto([S.value_simple('c', -2.0)]), 8)
    w.close()
    files = os.listdir(str(tmp_path / 'run'))
    assert len(files) == 1 and files[0].startswith('events.out.tfevents.')
    evs = R.read_events(str(tmp_path / 'run' / files[0]))
    assert evs[0]['file_version'] == 'brain.Event:2'
    assert [e['step'] for e in evs[1:]] == [7, 8]
    assert evs[1]['values'] == [{'tag': 'a/b', 'simple_value': 1.5}]
    assert evs[2]['values'] == [{'tag': 'c', 'simple_value': -2.0}]


def test_record_crc_detects_corruption(tmp_path):
    rec = S.tfrecord(b'hello summary')
    p = tmp_path / 'f'
    p.write_bytes(rec)
    assert R.read_records(str(p)) == [b'hello summary']
    bad = bytearray(rec)
    bad[14] ^= 1
    p.write_bytes(bytes(bad))
    with pytest.raises(AssertionError):
        R.read_records(str(p))


def test_protobuf_round_trips():
    h = S.histogram_proto(-1.25, 3.5, 10.0, 4.0, 20.5, [-1.0, 0.0, 4.0], [2.0, 0.0, 8.0])
    d = R.parse_histo(h)
    assert (d['min'], d['max'], d['num'], d['sum'], d['sum_squares']) == (-1.25, 3.5, 10.0, 4.0, 20.5)
    assert d['bucket_limit'] == [-1.0, 0.0, 4.0] and d['bucket'] == [2.0, 0.0, 8.0]
    im = R.parse_image(S.image_proto(480, 720, 3, b'\x89PNGxyz'))
    assert im == {'height': 480, 'width': 720, 'colorspace': 3, 'png': b'\x89PNGxyz'}
    vals = [S.value_simple('s', 0.25), S.value_histo('h', h), S.value_image('i/image/0', S.image_proto(2, 3, 1, b'p'))]
    ev = R.parse_event(S.event_proto(1234.5, 2 ** 40, summary=S.summary_proto(vals)))
    assert ev['wall_time'] == 1234.5 and ev['step'] == 2 ** 40
    assert [v['tag'] for v in ev['values']] == ['s', 'h', 'i/image/0']
    assert ev['values'][0]['simple_value'] == 0.25
    assert ev['values'][1]['histo']['bucket'] == [2.0, 0.0, 8.0]
    assert ev['values'][2]['image']['width'] == 3
    ev0 = R.parse_event(S.event_proto(1.0, 0, file_version='brain.Event:2'))
    assert ev0['file_version'] == 'brain.Event:2' and ev0['step'] == 0


@pytest.mark.parametrize('shape', [(7, 5, 3), (4, 9, 1), (480, 720, 3)])
def test_png_round_trip(shape):
    from PIL import Image
    rng = np.random.RandomState(sum(shape))
    img = rng.randint(0, 256, size=shape).astype(np.uint8)
    img[: shape[0] // 2] = 17          # a flat region: the Sub filter's zero run
    png = S.encode_png(img)
    back = np.asarray(Image.open(io.BytesIO(png)))
    assert back.reshape(shape).tolist() == img.tolist()


def test_histogram_encoding_of_known_values():
    lim = R.default_limits()
    mid = lim.size // 2
    vals = np.array([0.0, 0.0, 1.0, 1.0, 1.0, -2.0, 5e-13, 1e30], np.float64)
    mn, mx, num, s, ss, counts = R.histogram(vals)
    assert counts[mid + 1] == 3                  # 0.0 (twice) and 5e-13 go to (0, 1e-12]
    proto = R.parse_histo(S.encode_histogram(mn, mx, num, s, ss, counts))
    bl, bc = R.encode_to_proto(counts)
    assert proto['bucket_limit'] == bl and proto['bucket'] == bc
    # expected structure: zero runs collapsed into the last limit of the run
    nz = np.nonzero(counts)[0]
    assert sum(proto['bucket']) == vals.size
    assert [b for b in proto['bucket'] if b > 0] == [float(counts[i]) for i in nz]
    assert proto['bucket_limit'][-1] == sys.float_info.max and proto['bucket'][-1] == 1.0     # 1e30 lies beyond 1e20
    for i, b in zip(nz, [float(counts[i]) for i in nz]):
        k = proto['bucket_limit'].index(lim[i])
        assert proto['bucket'][k] == b
        assert k == 0 or proto['bucket'][k - 1] == 0.0 or lim[i - 1] in proto['bucket_limit']
    empty = R.parse_histo(S.encode_histogram(0, 0, 0, 0, 0, np.zeros(lim.size)))
    assert empty['bucket_limit'] == [sys.float_info.max] and empty['bucket'] == [0.0]


def test_colorize_and_quantiser_restatement():
    hm = np.arange(4, dtype=np.float32).reshape(1, 2, 2, 1)
    c = S.colorize(hm, 'lwri')
    assert c.shape == (1, 2, 2, 3) and np.array_equal(c[..., 0], hm[..., 0]) and np.array_equal(c[..., 1], hm[..., 0]) and not c[..., 2].any()
    img = np.array([[[-1.0], [0.5]], [[np.nan], [1.0]]], np.float32)
    u = R.normalize_float_image(img)
    assert u[1, 0, 0] == 255 and u[0, 0, 0] == 1 and u[1, 1, 0] == 255     # 128 - 127 = 1; 128 + 127 = 255
    assert not R.normalize_float_image(np.zeros((2, 2, 3), np.float32)).any()


def test_file_writer_flushes(tmp_path):
    w = S.FileWriter(str(tmp_path), flush_secs=0.05)
    w.add_summary(S.summary_proto([S.value_simple('x', 3.0)]), 1)
    import time
    time.sleep(0.3)
    evs = R.read_events(w.path)          # readable before close: the background flush ran
    assert evs[-1]['values'][0]['simple_value'] == 3.0
    w.close()
    hdr = open(w.path, 'rb').read(8)
    assert struct.unpack('<Q', hdr)[0] > 0
