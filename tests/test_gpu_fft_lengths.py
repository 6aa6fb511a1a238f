"""The frequency-domain convolution (conv_fft.hip and the kernels it launches) against the float64 oracle at EVERY transform length, as the
column length NY and as the row length NX, for both kernel sizes: the map that fills its transform (the wrap-around of the circular convolution
lands in the first row / column nobody reads, so an off-by-one in padding, wrap, the Nyquist bin or the output offset shows here first), the odd
map one short of it (the row pass packs two real rows into one complex transform: the last row is unpaired), and the first map that needs the
length (the most zero padding).  The cases come from tests/fft_lengths_ref.py; tests/test_fft_lengths_cpu.py holds them to the source.

Which kernel family runs each pass, read from the launchers (conv_fft.hip: the five pass functions pass_rows_fwd .. pass_rows_inv; conv_fft_reg_fwd.hip, conv_fft_reg_inv.hip,
conv_fft_rows_*.hip, conv_fft_cols.hip).  'LDS' = the kernels CFFT_BY_SIZE instantiates for all 14 lengths, 'reg' = register-resident transforms.

  pass            | fp32 handle                    | fp32, fft_reg = 0 | bf16 handle (one fp16 part, 16-bit T) | bf16, fft_single = 0 (fp32 T)
  ----------------+--------------------------------+-------------------+---------------------------------------+------------------------------
  rows forward    | LDS, every NX                  | LDS               | reg at NX 28, 50, 96; LDS elsewhere   | LDS, every NX
  columns forward | LDS, every NY (no reg kernel)  | LDS               | LDS, every NY                         | LDS, every NY
  channel GEMM    | cgemm_split, two fp16 parts    | same              | one fp16 part                         | two bf16 parts
  columns inverse | reg at NY 20, 32, 36, 64; LDS  | LDS, every NY     | reg at NY 20, 32, 36, 64; LDS         | reg at NY 20, 32, 36, 64; LDS
                  | elsewhere (NY 128, 192: 32-channel blocks, every arm)
  rows inverse    | reg at NX 28, 32, 50, 96 (even | LDS, every NX     | reg at NX 28, 50, 96; LDS elsewhere   | reg at NX 28, 50, 96; LDS
                  | Cout); LDS elsewhere           |                   | (32 included)                         | elsewhere

  The fft_reg = 0 run puts the LDS inverse kernels through the eight lengths that also have register kernels (elsewhere only the tower does, at
  the model's three geometries); at every other (NY, NX) it launches the very same kernels: the two results must be bit-identical there.
  The NY sweep keeps W = 16 (NX = 20: LDS rows), the NX sweep H = 16 (NY = 20: register inverse columns at fft_reg = 1, LDS at 0).

  Matrix cores: rows_inv_mfma_kernel (conv_fft_rows_mfma.hip) is the 96-point inverse row pass of a bf16 handle writing the PLANAR bf16 layout from a
  16-bit T'.  jcm_conv_layer keeps NHWC on both sides of the layer, so a stand-alone layer never reaches it (the tower does:
  test_bf16_rows_on_matrix_cores_vs_register_kernels).  The fft_rows_mfma = 0 runs below therefore launch the same kernels as the default and must
  be bit-identical to it; they are kept so that the day jcm_conv_layer reaches the matrix-core kernel, that kernel meets every length's cases."""
import zlib

import numpy as np
import pytest
import torch

import joint_cnn_mrf_amd  # noqa: F401
import fft_lengths_ref as R
from oracle import jcm_oracle as O
from test_gpu_random_shapes import check_bf16_layer, layer_params

pytestmark = pytest.mark.gpu

F32_BAR = 2e-5      # test_conv_layer_random_shape: max |got - ref| / max |ref|
BF16_ARMS = (('bf16', dict(), dict(slack_rel=1e-3, flips=0.12, rms_rel=4e-4)),      # the default handle: one fp16 part, 16-bit T
             ('bf16_strict', dict(fft_single=False), dict()))                         # two bf16 parts, fp32 T: the one-ulp bar


class Engines:
    """One engine per (arm, kernel size, channels), made at first use and shared by every case: all 64 -> 64 cases of a kernel size run on the
    same weights, the map size changes per call."""

    def __init__(self):
        self.params, self.engines = {}, {}

    def params_of(self, c):
        key = (c.ks, c.cin, c.cout)
        if key not in self.params:
            self.params[key] = layer_params(np.random.RandomState(1000 * c.ks + c.cin + c.cout), c.cin, c.cout, c.ks)
        return self.params[key]

    def get(self, arm, c):
        from joint_cnn_mrf_amd.engine import Engine
        key = (arm, c.ks, c.cin, c.cout)
        if key not in self.engines:
            kw = dict(f32_conv='exact') if arm == 'fp32' else dict(precision='bf16', **dict((a, k) for a, k, _ in BF16_ARMS)[arm])
            self.engines[key] = Engine(device=0, **kw).load_params(self.params_of(c))
        return self.engines[key]

    def close(self):
        for e in self.engines.values():
            e.close()


@pytest.fixture(scope='module')
def engines():
    e = Engines()
    yield e
    e.close()


def case_input(c):
    rs = np.random.RandomState(zlib.crc32(R.case_id(c).encode()) & 0x7fffffff)
    return rs.standard_normal((c.B, c.H, c.W, c.cin)).astype(np.float32)


def run(eng, xd, c):
    return eng.conv_layer(xd, 'c', 1, n_out=c.cout).cpu().numpy()


@pytest.mark.parametrize('c', R.cases(), ids=R.case_id)
def test_fp32_layer_at_every_length(c, engines):
    """The default fp32 handle, then the same handle with fft_reg = 0 (the LDS kernels at the lengths that have register kernels): both within
    2e-5 of the float64 reference's largest entry, and bit-identical where no register kernel exists for the case's lengths."""
    ny, nx = R.sizes_of(c.H, c.W, c.ks)
    x = case_input(c)
    ref = O.conv_layer(x.astype(np.float64), engines.params_of(c), c.ks, 1, 'c')
    eng = engines.get('fp32', c)
    assert eng.get_option('fft_reg') == 1
    assert eng.conv_kernel_name('c', c.B, c.H, c.W).startswith('conv_fft')
    xd = torch.as_tensor(x, device='cuda:0')
    got = {1: run(eng, xd, c)}
    eng.set_option('fft_reg', 0)
    try:
        got[0] = run(eng, xd, c)
    finally:
        eng.set_option('fft_reg', 1)
    scale = np.abs(ref).max()
    err = {k: float(np.abs(v - ref).max() / scale) for k, v in got.items()}
    same = np.array_equal(got[0].view(np.int32), got[1].view(np.int32))
    print('FFTLEN fp32 %s NY %d NX %d  fft_reg=1 %.3e  fft_reg=0 %.3e  identical %s' % (R.case_id(c), ny, nx, err[1], err[0], same))
    assert err[1] <= F32_BAR, 'fft_reg = 1: %.2e' % err[1]
    assert err[0] <= F32_BAR, 'fft_reg = 0: %.2e' % err[0]
    if not R.has_register_kernel(c):
        assert same, 'fft_reg = 0 changed the result of a layer with no register kernel (NY %d, NX %d)' % (ny, nx)


def bf16_figures(got, ref, slack_rel=1e-5, **_):
    """The three figures check_bf16_layer bounds: worst distance in bf16 ulps beyond the slack, share of entries rounded differently, rms / scale."""
    ulp = 2.0 ** (np.floor(np.log2(np.maximum(np.abs(ref), 1e-30))) - 7)
    diff = np.abs(got - ref)
    scale = np.abs(ref).max()
    return float(((diff - slack_rel * scale) / ulp).max()), float((diff > 0).mean()), float(np.sqrt(np.mean(diff ** 2)) / scale)


@pytest.mark.parametrize('c', [c for c in R.cases() if c.ks == 9 and c.cout % 8 == 0], ids=R.case_id)
def test_bf16_layer_at_every_length(c, engines):
    """The 9x9 cases on bf16 handles against the oracle in their arithmetic (operands rounded to bf16, wide accumulation, result rounded to bf16):
    the default handle under the looser bar of the 11-bit intermediates, fft_single = 0 under the strict one-ulp bar
    (test_conv_layer_random_shape's), each again with fft_rows_mfma = 0 on the same handle (bit-identical: the table above)."""
    ny, nx = R.sizes_of(c.H, c.W, c.ks)
    x = case_input(c)
    refb = O.conv_layer(x.astype(np.float64), engines.params_of(c), c.ks, 1, 'c', emulate='bf16')
    xd = torch.as_tensor(x, device='cuda:0')
    for arm, _, bars in BF16_ARMS:
        eng = engines.get(arm, c)
        assert eng.get_option('fft_rows_mfma') == 1
        assert eng.conv_kernel_name('c', c.B, c.H, c.W).startswith('conv_fft')
        got = {1: run(eng, xd, c).astype(np.float64)}
        eng.set_option('fft_rows_mfma', 0)
        try:
            got[0] = run(eng, xd, c).astype(np.float64)
        finally:
            eng.set_option('fft_rows_mfma', 1)
        for bits in (1, 0):
            print('FFTLEN %s %s NY %d NX %d  fft_rows_mfma=%d  ulps beyond slack %.3f  flips %.4f  rms/scale %.3e'
                  % ((arm, R.case_id(c), ny, nx, bits) + bf16_figures(got[bits], refb, **bars)))
        for bits in (1, 0):
            check_bf16_layer(got[bits], refb, **bars)
        assert np.array_equal(got[0], got[1]), 'fft_rows_mfma changed a stand-alone NHWC layer (%s)' % arm


@pytest.mark.parametrize('shape', [(1, 185, 16), (1, 16, 185)], ids=lambda s: 'B%d_%dx%d' % s)
def test_refused_sizes_leave_the_route(shape, engines):
    """H + ks - 1 = 193: one past the limit.  The 9x9 layer must not name conv_fft, and whatever kernel takes it matches the oracle (the bars of
    the direct kernels in test_conv_layer_random_shape: 2e-5 fp32, one bf16 ulp)."""
    B, H, W = shape
    assert R.sizes_of(H, W, 9) is None and R.sizes_of(min(H, 184), min(W, 184), 9) == tuple(192 if v == 185 else 20 for v in (H, W))
    c = R.Case('refused', 192, 'pad', B, H, W, 64, 64, 9)
    x = case_input(c)
    p = engines.params_of(c)
    xd = torch.as_tensor(x, device='cuda:0')
    eng = engines.get('fp32', c)
    name = eng.conv_kernel_name('c', B, H, W)
    assert 'conv_fft' not in name, name
    ref = O.conv_layer(x.astype(np.float64), p, 9, 1, 'c')
    err = float(np.abs(run(eng, xd, c) - ref).max() / np.abs(ref).max())
    print('FFTLEN refused fp32 %dx%d on %s: %.3e' % (H, W, name, err))
    assert err <= F32_BAR
    eng = engines.get('bf16', c)
    name = eng.conv_kernel_name('c', B, H, W)
    assert 'conv_fft' not in name, name
    refb = O.conv_layer(x.astype(np.float64), p, 9, 1, 'c', emulate='bf16')
    gotb = run(eng, xd, c).astype(np.float64)
    print('FFTLEN refused bf16 %dx%d on %s: ulps beyond slack %.3f  flips %.4f  rms/scale %.3e' % ((H, W, name) + bf16_figures(gotb, refb)))
    check_bf16_layer(gotb, refb)
