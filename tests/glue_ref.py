"""Shapes, inputs and references of the inference-glue tests (test_gpu_glue.py, test_glue_cpu.py): the three-branch merge kernels of csrc/glue.hip
(upsample_merge3_kernel<float>, upsample_merge3_kernel<__bf16>, upsample_merge3_bf16x8_kernel, upsample_merge3_planar_kernel), the bilinear resize, the
2x2 max pool, spatial softmax / arg-max (softmax_argmax_kernel<9> and the two general kernels) and csrc/multiscale.hip.  No GPU is needed here."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from oracle import jcm_oracle as O

f32, f64 = np.float32, np.float64
U32 = 2.0 ** -24      # unit roundoff of float32

# ------------------------------------------------------------------------------------------------ merge
# (B, H, W, H2, W2, H3, W3) -> what the row is in the table for
MERGE_SHAPES = (
    ((2, 60, 90, 30, 45, 15, 23), "the model's"),
    ((1, 61, 89, 31, 45, 16, 23), 'a 488 x 712 image'),
    ((3, 7, 5, 4, 3, 2, 2), 'tiny'),
    ((1, 12, 20, 1, 1, 1, 1), 'every hi clamps to 0'),
    ((2, 9, 11, 9, 11, 3, 3), 'x2 already full size: the plain-load branch'),
    ((1, 8, 8, 8, 8, 8, 8), 'both branches plain loads'),
    ((1, 5, 7, 10, 14, 20, 28), 'scales > 1'),
)
# kernel -> channel counts.  bf16x4 is what a bf16 call with C % 8 == 4 takes, bf16x8 what C % 8 == 0 takes (upsample_merge3 in glue.hip)
MERGE_CHANNELS = {'f32': (4, 12, 128), 'bf16x4': (4, 12), 'bf16x8': (8, 24, 128), 'planar': (8, 24, 128)}
UNIT_CHANNELS = {'f32': 4, 'bf16x4': 4, 'bf16x8': 8, 'planar': 8}      # channels per thread and loop step
GRID_CAP, BLOCK = 16384, 256      # grid_for() in glue.hip

# bf16x8, C = 8: the unit count chooses the grid, and the grid whether blocks are remapped to XCDs (gridDim % 8 == 0)
BLOCK_CASES = (
    dict(shape=(1, 45, 45, 23, 23, 12, 12), units=2025, blocks=8, remap=True, partial=True),
    dict(shape=(1, 64, 64, 32, 32, 16, 16), units=4096, blocks=16, remap=True, partial=False),
    dict(shape=(1, 40, 44, 20, 22, 10, 11), units=1760, blocks=7, remap=False, partial=True),
)
# past the grid cap: more than 16384 * 256 = 4 194 304 units, so the grid-stride loop makes a second, partial lap.  13 images of the model's geometry with
# 60 units per pixel (61 for bf16x4, which needs C % 8 == 4) are 4 212 000 (4 282 200) units; 12 images are not enough (test_glue_cpu.py checks the counts)
LAP_SHAPE = (13, 60, 90, 30, 45, 15, 23)
LAP_CHANNELS = {'f32': 240, 'bf16x4': 244, 'bf16x8': 480, 'planar': 480}


def units(kernel, shape, C):
    B, H, W = shape[:3]
    return B * H * W * (C // UNIT_CHANNELS[kernel])


def grid_for(total):
    return max(1, min(GRID_CAP, -(-total // BLOCK)))


def nhwc_to_planar(x):
    """[B,H,W,C] -> planar [B,C/8,H,W,8] (the layout of the strip kernels' activations)."""
    B, H, W, C = x.shape
    assert C % 8 == 0
    return np.ascontiguousarray(x.reshape(B, H, W, C // 8, 8).transpose(0, 3, 1, 2, 4))


def planar_to_nhwc(x):
    B, C8, H, W, e = x.shape
    assert e == 8
    return np.ascontiguousarray(x.transpose(0, 2, 3, 1, 4).reshape(B, H, W, C8 * 8))


def bf16_round(x):
    """O.bf16_round; a tensor of the grid-cap cases (tens of millions of entries) is rounded image by image on a few threads."""
    if x.size < (1 << 22) or x.shape[0] == 1:
        return O.bf16_round(x)
    with ThreadPoolExecutor(8) as pool:      # NumPy releases the interpreter lock inside its loops
        return np.concatenate(list(pool.map(lambda b: O.bf16_round(x[b:b + 1]), range(x.shape[0]))))


def merge_inputs(shape, C, bf16, signed=False):
    """x1 [B,H,W,C], x2 [B,H2,W2,C], x3 [B,H3,W3,C] float32: relu(N(0,1)) as the tower's branches are (N(0,1) with signed), bf16 values when bf16."""
    B, H, W, H2, W2, H3, W3 = shape
    rs = np.random.RandomState((1009 * H + 31 * W + 7 * H2 + W3 + 13 * C + B + (500 if signed else 0)) % (2 ** 31))
    xs = []
    for h, w in ((H, W), (H2, W2), (H3, W3)):
        x = rs.standard_normal((B, h, w, C)).astype(f32)
        if not signed:
            x = np.maximum(x, f32(0))
        xs.append(bf16_round(x) if bf16 else x)
    return xs


def input_max(xs):
    return max(float(np.abs(x).max()) for x in xs)


def merge3_ref(x1, x2, x3, dtype):
    """((x1 + up(x2)) + up(x3)) / dtype(3), up = O.resize_bilinear_tf1 to x1's size (the identity for a branch that has it).  dtype float64: the reference
    of the error bound (the taps' coordinates and weights are float32 in either dtype, as TF computes them).  dtype float32: NumPy rounds every operation
    once, in the kernels' expression order -- tl + (tr - tl) * tx, the same for the lower row, top + (bot - top) * ty, (x1 + u2) + u3, and a correctly
    rounded third (div3 of resize_tf1.h) -- and the library is built with -ffp-contract=off, so this is the kernels' result bit for bit."""
    x1, x2, x3 = (np.asarray(t, dtype) for t in (x1, x2, x3))
    H, W = x1.shape[1:3]
    return ((x1 + O.resize_bilinear_tf1(x2, H, W)) + O.resize_bilinear_tf1(x3, H, W)) / dtype(3)


def bf16_ulp(x):
    """The spacing of bfloat16 at |x| (8 significant bits), for normal values."""
    return 2.0 ** (np.floor(np.log2(np.maximum(np.abs(np.asarray(x, f64)), 2.0 ** -126))) - 7)


def one_bf16_ulp_apart(a, b, slack=0.0):
    """Is every |a - b| <= one bf16 ulp (taken at the larger of the two, so that a pair astride a power of two counts as neighbours) + slack?  slack = 0 for
    relu inputs: every term is >= 0, nothing cancels, the float32 and float64 values agree to a relative 1e-5 and round to the same or to neighbouring
    bf16 values.  Signed inputs cancel: a merged value far below M carries the float32 evaluation's ABSOLUTE error, up to 12 * 2^-24 M, which exceeds the
    bf16 ulp of a value below 2^-13 M -- there |bf16(a) - bf16(b)| <= |a - b| + two half ulps is what holds, so slack is that float32 bound."""
    a, b = np.asarray(a), np.asarray(b)
    differ = a != b      # a small share: only these are looked at
    a, b = a[differ].astype(f64), b[differ].astype(f64)
    return bool((np.abs(a - b) <= bf16_ulp(np.maximum(np.abs(a), np.abs(b))) + slack).all())


def bf16_slack(xs, signed):
    return 12 * U32 * input_max(xs) if signed else 0.0


def bf16_refs(xs):
    """(bf16_round of the float32 evaluation, bf16_round of the float64 one, the share of entries where the two differ) on bf16-valued inputs."""
    r32 = bf16_round(merge3_ref(*xs, f32))
    r64 = bf16_round(merge3_ref(*xs, f64)).astype(f32)
    return r32, r64, float((r32 != r64).mean())


# ------------------------------------------------------------------------------------------------ resize, pool
# (B, H, W, C, OH, OW)
RESIZE_SHAPES = (
    ((1, 488, 712, 3, 244, 356), "the tower's sub-sampling resize, c1"),
    ((1, 488, 712, 3, 122, 178), "the tower's sub-sampling resize, c1"),
    ((2, 15, 23, 8, 60, 90), 'up, c4'),
    ((2, 61, 91, 1, 60, 90), 'c1'),
    ((1, 1, 1, 5, 5, 7), 'one source pixel, c1'),
    ((1, 5, 7, 4, 1, 1), 'one target pixel'),
    ((1, 48, 72, 12, 24, 36), 'down, c4'),
    ((2, 9, 9, 4, 9, 9), 'the copy'),
)
POOL_SHAPES = ((2, 1, 1, 4), (1, 1, 9, 4), (1, 9, 1, 8), (3, 7, 5, 12), (1, 31, 46, 32))

# ------------------------------------------------------------------------------------------------ softmax / arg-max
# softmax_argmax_kernel<9>: SA_NT threads, thread tid owns quad tid (register set j = 0) and quad tid + SA_NT (j = 1); a quad is 4 consecutive pixels
SA_NT, SA_QPT, WAVE = 704, 2, 64
SA_MAX_HW = 4 * SA_NT * SA_QPT      # 5632
FUSED_MAPS = ((1, 4), (2, 2), (16, 16), (32, 88), (30, 94), (60, 90), (67, 84), (64, 88))      # K = 9
FUSED_QUADS = (1, 1, 64, 704, 705, 1350, 1407, 1408)
GENERAL_MAPS = ((60, 94, 9), (74, 73, 9), (3, 5, 1), (15, 23, 4), (1, 1, 10), (20, 13, 16))      # (H, W, K)
LAST_OF_J0, FIRST_OF_J1 = 4 * SA_NT - 1, 4 * SA_NT      # pixels 2815 and 2816


def takes_fused(HW, K):
    """softmax_argmax() in glue.hip."""
    return K == 9 and HW % 4 == 0 and HW // 4 <= SA_NT * SA_QPT


def owner(pixel):
    """pixel -> (thread, register set j, position in the quad) of softmax_argmax_kernel<9>."""
    q = pixel // 4
    return q % SA_NT, q // SA_NT, pixel % 4


def live_j1_threads(HW):
    """How many threads have a live quad in register set j = 1."""
    return max(0, HW // 4 - SA_NT)


def tie_pairs(HW):
    """Neighbouring pixel pairs (p, p + 1) owned by different threads, waves or register sets, as far as a map of HW pixels has them: 255/256 (the first
    wave boundary of the fused kernel, and thread 255 / thread 0's second step in the 256-thread general kernels), 2815/2816 (last pixel of j = 0, first of
    j = 1), and 4 tid + 3 / 4 (tid + 1) for threads inside a wave, at a later wave boundary and in set j = 1."""
    cand = [(255, 256), (LAST_OF_J0, FIRST_OF_J1)]
    for tid in (0, 1, 62, 64, 127, 350, 702):
        cand.append((4 * tid + 3, 4 * (tid + 1)))
        cand.append((FIRST_OF_J1 + 4 * tid + 3, FIRST_OF_J1 + 4 * (tid + 1)))
    return [p for p in cand if p[1] < HW]


def softmax_data(kind, B, H, W, K):
    """-> (logits float32 [B,H,W,K], expected arg-max pixels int [B,K] or None).  Kinds: normal = 3 N(0,1); const; integer = integers in [-80, 0], so
    that z - max is exact; neg_inf = -inf at every pixel p % 3 == 1; ties = two equal maxima on a pair of tie_pairs (the map's own first / last pixel
    where it has no such pair), the earlier must win; ends = the maximum at the first pixel, the last pixel and, where the map has it, pixel 2819."""
    HW = H * W
    rs = np.random.RandomState(HW * 31 + K + len(kind))
    z = (3.0 * rs.standard_normal((B, HW, K))).astype(f32)
    want = None
    if kind == 'const':
        z[:] = f32(0.25)
        want = np.zeros((B, K), int)
    elif kind == 'integer':
        z = rs.randint(-80, 1, (B, HW, K)).astype(f32)
    elif kind == 'neg_inf':
        z[:, 1::3] = -np.inf
    elif kind == 'ties':
        pairs = tie_pairs(HW) or [(0, HW - 1)]
        want = np.zeros((B, K), int)
        for b in range(B):
            for k in range(K):
                lo, hi = pairs[(b * K + k) % len(pairs)]
                z[b, lo, k] = z[b, hi, k] = f32(40)
                want[b, k] = lo
    elif kind == 'ends':
        spots = [0, HW - 1] + ([FIRST_OF_J1 + 3] if HW > FIRST_OF_J1 + 3 else [])
        want = np.zeros((B, K), int)
        for b in range(B):
            for k in range(K):
                want[b, k] = spots[(b * K + k) % len(spots)]
                z[b, want[b, k], k] = f32(50)
    else:
        assert kind == 'normal', kind
    return z.reshape(B, H, W, K), want


SOFTMAX_KINDS = ('normal', 'const', 'integer', 'neg_inf', 'ties', 'ends')


def coords_of(pixels, W):
    """[B,K] flat pixels -> [B,2,K] (row, col)."""
    return np.stack([pixels // W, pixels % W], axis=1).astype(np.int32)


# ------------------------------------------------------------------------------------------------ window resize
WINDOW_SOURCES = ((2, 24, 36, 3), (2, 15, 23, 9))      # an image (values in [-1, 1]) and a stack of heat maps
WINDOW_DATA = ('positive', 'signed', 'negative')
ODD_TARGET = (13, 17)


def window_source(shape, kind):
    rs = np.random.RandomState(shape[1] * 10 + len(kind))
    x = rs.random_sample(shape) * 0.8 + 0.1      # [0.1, 0.9)
    if kind == 'signed':
        x = x * 2 - 1      # [-0.8, 0.8)
    elif kind == 'negative':
        x = -x
    return x.astype(f32)


def hand_windows(H, W):
    """(y0, x0, h, w) windows of an H x W source: a pad on each single side, on all sides, a crop to one pixel, to one row, and one wholly outside."""
    return [(-3, 0, H + 3, W), (0, 0, H + 2, W), (0, -4, H, W + 4), (0, 0, H, W + 5), (-2, -3, H + 5, W + 7),
            (H // 2, W // 3, 1, 1), (H - 1, 2, 1, W - 4), (H + 2, W + 1, 4, 6), (-9, -9, 5, 5)]
