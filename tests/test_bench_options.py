"""bench.py's options that need no GPU: the --dump-outputs writer (float32 files, a size limit) and --layer-times refused without --full."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dump_outputs_writes_float32_and_refuses_too_much(tmp_path):
    import bench
    out = tmp_path / 'out'
    coords = np.arange(36, dtype=np.int32).reshape(2, 2, 9)
    bench.dump_outputs(str(out), {'sm_coords': coords, 'losses': torch.tensor([0.5, 0.25])})
    assert sorted(os.listdir(out)) == ['losses.npy', 'sm_coords.npy']
    got = np.load(out / 'sm_coords.npy')
    assert got.dtype == np.float32 and got.shape == (2, 2, 9)
    np.testing.assert_array_equal(got, coords)
    np.testing.assert_array_equal(np.load(out / 'losses.npy'), np.array([0.5, 0.25], np.float32))
    big = tmp_path / 'big'
    with pytest.raises(SystemExit, match='exceed'):
        bench.dump_outputs(str(big), {'x': np.zeros(bench.DUMP_MAX_BYTES // 4 + 1, np.float32)})
    assert not big.exists() or not os.listdir(big)


def test_layer_times_needs_full():
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--layer-times'], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 2 and '--layer-times needs --full' in r.stderr, (r.returncode, r.stderr[-2000:])
