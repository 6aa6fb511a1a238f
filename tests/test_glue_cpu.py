"""The references and case tables of test_gpu_glue.py (glue_ref.py) held to themselves, without a GPU: what the GPU tests assume about their inputs, their
float32 / float64 references and the kernels' work distribution is checked here, so that a GPU failure speaks about a kernel."""
import numpy as np
import pytest

import glue_ref as R
from oracle import jcm_oracle as O
from oracle import multiscale_oracle as MO

f32, f64 = np.float32, np.float64
BF16_KERNELS = ('bf16x4', 'bf16x8', 'planar')


def test_planar_round_trip():
    x = np.arange(2 * 3 * 5 * 24, dtype=f32).reshape(2, 3, 5, 24)
    p = R.nhwc_to_planar(x)
    assert p.shape == (2, 3, 3, 5, 8) and p.flags['C_CONTIGUOUS']
    assert p[1, 2, 1, 4, 3] == x[1, 1, 4, 2 * 8 + 3]      # [b][c / 8][y][x][c % 8]
    assert np.array_equal(R.planar_to_nhwc(p), x)
    assert np.array_equal(R.nhwc_to_planar(R.planar_to_nhwc(p)), p)


def test_merge_tables_say_what_the_launcher_does():
    """Which kernel a channel count takes, and the unit, block and lap counts the block-count and grid-cap cases are there for (grid_for, upsample_merge3)."""
    assert all(C % 4 == 0 for C in R.MERGE_CHANNELS['f32'])
    assert all(C % 8 == 4 for C in R.MERGE_CHANNELS['bf16x4']) and R.LAP_CHANNELS['bf16x4'] % 8 == 4
    assert all(C % 8 == 0 for k in ('bf16x8', 'planar') for C in R.MERGE_CHANNELS[k] + (R.LAP_CHANNELS[k],))
    for c in R.BLOCK_CASES:
        n = R.units('bf16x8', c['shape'], 8)
        assert n == c['units'] and R.grid_for(n) == c['blocks'] and (c['blocks'] % 8 == 0) == c['remap'] and (n % R.BLOCK != 0) == c['partial']
    cap = R.GRID_CAP * R.BLOCK
    for k, C in R.LAP_CHANNELS.items():
        n = R.units(k, R.LAP_SHAPE, C)
        assert cap < n < 2 * cap and R.grid_for(n) == R.GRID_CAP and n < 2 ** 32      # a second lap, and a partial one
        assert R.units(k, (R.LAP_SHAPE[0] - 1,) + R.LAP_SHAPE[1:], C) <= cap      # one image less stays within one lap
    assert R.units('bf16x8', R.LAP_SHAPE, 480) == 4212000 and R.units('f32', R.LAP_SHAPE, 240) == 4212000


def test_merge_inputs_are_what_the_tests_say():
    for shape, _ in R.MERGE_SHAPES:
        for bf in (False, True):
            xs = R.merge_inputs(shape, 12, bf)
            B, H, W, H2, W2, H3, W3 = shape
            assert [x.shape for x in xs] == [(B, H, W, 12), (B, H2, W2, 12), (B, H3, W3, 12)] and all(x.dtype == f32 for x in xs)
            assert all((x >= 0).all() for x in xs) and (xs[0] == 0).any() and (xs[0] > 0).any()      # relu(N(0,1))
            sg = R.merge_inputs(shape, 12, bf, signed=True)
            assert (sg[0] < 0).any() and (sg[0] > 0).any()
            if bf:
                assert all(np.array_equal(O.bf16_round(x), x) for x in xs + sg)
            assert 0 < R.input_max(xs) < 8


def _merge_cases():
    for shape, _ in R.MERGE_SHAPES:
        for C in sorted({C for v in R.MERGE_CHANNELS.values() for C in v}):
            yield shape, C
    for c in R.BLOCK_CASES:
        yield c['shape'], 8


@pytest.mark.parametrize('signed', [False, True], ids=['relu', 'signed'])
def test_merge_ref_float32_within_the_bound_of_float64(signed):
    """The float32 evaluation the kernels are compared with bit for bit lies within 12 * 2^-24 * M of the float64 one on every case (the bound of
    test_gpu_glue.py, derived there) -- so the two assertions of the GPU test cannot contradict each other."""
    worst = 0.0
    for shape, C in _merge_cases():
        xs = R.merge_inputs(shape, C, False, signed)
        r32, r64 = R.merge3_ref(*xs, f32), R.merge3_ref(*xs, f64)
        assert r32.dtype == f32 and r64.dtype == f64 and r32.shape == xs[0].shape
        err = float(np.abs(r32.astype(f64) - r64).max()) / (R.U32 * R.input_max(xs))
        worst = max(worst, err)
        assert err <= 12, (shape, C, err)
    print('merge3_ref float32 against float64, worst: %.2f x 2^-24 M' % worst)


@pytest.mark.parametrize('signed', [False, True], ids=['relu', 'signed'])
def test_bf16_references_differ_on_less_than_a_thousandth(signed):
    """bf16_round of the float32 evaluation against bf16_round of the float64 one: the share of entries that round differently is below 0.1 % on every
    case, at most one bf16 ulp each.  The GPU test caps the kernels' differing share at 4 x this share, so the cap leaves no room for a wrong tap."""
    worst = 0.0
    cases = list(_merge_cases()) + [((1,) + R.LAP_SHAPE[1:], C) for C in sorted(set(R.LAP_CHANNELS.values()))]
    for shape, C in cases:
        xs = R.merge_inputs(shape, C, True, signed)
        r32, r64, share = R.bf16_refs(xs)
        worst = max(worst, share)
        assert share < 1e-3, (shape, C, share)
        assert R.one_bf16_ulp_apart(r32, r64, R.bf16_slack(xs, signed)), (shape, C)
    print('bf16 references, worst differing share: %.3e' % worst)


def test_merge_of_one_constant_is_the_constant():
    """x1 = x2 = x3 = c: every lerp is c + (c - c) * t = c exactly, at the clamped last row and column as anywhere; c + c is exact, so the result carries
    the rounding of 3c and that of the third: within 2^-23 |c|, at every entry."""
    for shape, _ in R.MERGE_SHAPES:
        B, H, W, H2, W2, H3, W3 = shape
        for c in (f32(0.7), f32(-1.3e-3), f32(1.0), f32(12345.678)):
            got = R.merge3_ref(np.full((B, H, W, 4), c, f32), np.full((B, H2, W2, 4), c, f32), np.full((B, H3, W3, 4), c, f32), f32)
            assert np.abs(got.astype(f64) - f64(c)).max() <= 2.0 ** -23 * abs(f64(c)), (shape, c)
    lo, hi, t = O.resize_weights_tf1(60, 30)      # the table's edge: the last output row reads lo = hi = in - 1 with a weight that is not 0
    assert lo[-1] == hi[-1] == 29 and t[-1] == f32(0.5) and hi.max() == 29
    lo, hi, t = O.resize_weights_tf1(5, 10)       # scales > 1: no clamp is reached, every second source row is skipped
    assert list(lo) == [0, 2, 4, 6, 8] and list(hi) == [1, 3, 5, 7, 9] and not t.any()
    lo, hi, t = O.resize_weights_tf1(12, 1)
    assert not lo.any() and not hi.any() and t.any()


def test_resize_oracle_float32_within_the_bound_of_float64():
    """One lerp: at most 10 roundings of size 2^-24 M (test_gpu_glue.py)."""
    for (B, H, W, C, OH, OW), _ in R.RESIZE_SHAPES:
        x = np.random.RandomState(H + OW).standard_normal((B, H, W, C)).astype(f32)
        r32, r64 = O.resize_bilinear_tf1(x, OH, OW), O.resize_bilinear_tf1(x.astype(f64), OH, OW)
        assert r32.dtype == f32 and r32.shape == (B, OH, OW, C)
        assert np.abs(r32.astype(f64) - r64).max() <= 10 * R.U32 * float(np.abs(x).max())
    assert {s[3] % 4 == 0 for s, _ in R.RESIZE_SHAPES} == {True, False}      # both resize_kernel_c4 and resize_kernel_c1


def test_softmax_quad_layout():
    """The quad counts the fused maps are chosen by, and where register sets, waves and threads meet."""
    assert tuple(h * w // 4 for h, w in R.FUSED_MAPS) == R.FUSED_QUADS
    assert all(R.takes_fused(h * w, 9) for h, w in R.FUSED_MAPS)
    assert not any(R.takes_fused(h * w, k) for h, w, k in R.GENERAL_MAPS)
    assert 60 * 94 > R.SA_MAX_HW == 5632 and (74 * 73) % 4 == 2 and 3 * 5 < 256 < 15 * 23 and 20 * 13 > 256 and 1 * 1 == 1
    assert R.owner(R.LAST_OF_J0) == (703, 0, 3) and R.owner(R.FIRST_OF_J1) == (0, 1, 0) and R.owner(2819) == (0, 1, 3)
    assert R.owner(255) == (63, 0, 3) and R.owner(256) == (64, 0, 0) and 63 // R.WAVE != 64 // R.WAVE
    assert [R.live_j1_threads(h * w) for h, w in R.FUSED_MAPS] == [0, 0, 0, 0, 1, 646, 703, 704]
    for hw in (4, 256, 2820, 5400, 5632, 5640):
        for lo, hi in R.tie_pairs(hw):
            assert hi == lo + 1 and hi < hw and R.owner(lo)[:2] != R.owner(hi)[:2]
    assert R.tie_pairs(4) == [] and (255, 256) in R.tie_pairs(345) and (2815, 2816) in R.tie_pairs(2820) and (2815, 2816) not in R.tie_pairs(2816)
    assert any(R.owner(lo)[1] == 1 and R.owner(hi)[1] == 1 for lo, hi in R.tie_pairs(5400))


@pytest.mark.parametrize('hwk', [(h, w, 9) for h, w in R.FUSED_MAPS] + list(R.GENERAL_MAPS), ids=lambda s: '%dx%dx%d' % s)
def test_softmax_data_is_what_the_tests_say(hwk):
    H, W, K = hwk
    HW = H * W
    for kind in R.SOFTMAX_KINDS:
        z, want = R.softmax_data(kind, 2, H, W, K)
        assert z.shape == (2, H, W, K) and z.dtype == f32
        flat = z.reshape(2, HW, K)
        assert np.isfinite(flat.max(axis=1)).all()      # no map is all -inf
        if want is not None:      # the planted pixel is the FIRST maximum of its map
            assert np.array_equal(np.argmax(flat, axis=1), want)
        if kind == 'ties' and HW > 1:
            assert ((flat == flat.max(axis=1, keepdims=True)).sum(axis=1) == 2).all()
        if kind == 'neg_inf':
            assert np.array_equal(np.isneginf(flat).any(axis=2), np.arange(HW)[None, :].repeat(2, 0) % 3 == 1)
        if kind == 'integer':
            d = flat - flat.max(axis=1, keepdims=True)
            assert np.array_equal(d, np.round(d)) and d.min() >= -80
        if kind == 'ends' and HW > 2820:
            assert (want == 2819).any() and (want == 0).any() and (want == HW - 1).any()
    ref = O.spatial_softmax(R.softmax_data('neg_inf', 2, H, W, K)[0].astype(f64))
    assert np.isfinite(ref).all() and np.allclose(ref.sum(axis=(1, 2)), 1.0, rtol=1e-12)


def test_window_cases():
    """The hand-written windows pad and crop what they say; with strictly negative data a padded window's zeros are its maximum."""
    for shape in R.WINDOW_SOURCES:
        _, H, W, C = shape
        pos, sgn, neg = (R.window_source(shape, k) for k in R.WINDOW_DATA)
        assert pos.min() > 0 and neg.max() < 0 and sgn.min() < 0 < sgn.max() and max(np.abs(a).max() for a in (pos, sgn, neg)) <= 1
        wins = R.hand_windows(H, W)
        pads = [(max(0, -y0), max(0, y0 + h - H), max(0, -x0), max(0, x0 + w - W)) for y0, x0, h, w in wins]      # top, bottom, left, right
        assert pads[:4] == [(3, 0, 0, 0), (0, 2, 0, 0), (0, 0, 4, 0), (0, 0, 0, 5)] and all(p > 0 for p in pads[4])
        assert wins[5][2:] == (1, 1) and wins[6][2] == 1 and pads[5] == pads[6] == (0, 0, 0, 0)
        for win in wins[7:]:
            assert not MO.take_window(neg[0], win).any()      # wholly outside
        for win in wins[:5]:
            t = MO.take_window(neg[0], win)
            assert t.max() == 0 and t.min() < 0
            ref = MO.resize_skimage(t, *R.ODD_TARGET)
            assert (ref == 0).any() and (ref < 0).any() and ref.max() == 0
        t = MO.take_window(neg[0], wins[6])      # a crop of negative data: 0 lies outside [min, max], the `preserve` branch of the clip
        assert t.max() < 0
