"""Plain numpy restatements of the training step's stages between its convolutions, from main.py / TF-1.x semantics (not from the kernels):
batch statistics and the moving-average update, the BatchNorm apply and backward (BN after ReLU: the mask is r > 0), the 2x2/2 SAME max pool
and its backward (first maximum in row-major window order), the adjoint of the TF-1 bilinear resize, the soft-label spatial cross-entropy with
TF's backprop and the softmax backward.

Every function takes `dtype`: np.float64 is the reference; np.float32 evaluates the SAME expressions in float32 with the sums still taken in
float64.  The distance between the two modes is the yardstick of tests/test_gpu_train_stages.py (`bound`): it comes from the reference alone.
"""
import numpy as np

from oracle import jcm_oracle as O

BN_EPS = 1e-3
BN_DECAY = 0.9


def _sum(a, axis):
    return np.sum(a.astype(np.float64), axis=axis)


# --------------------------------------------------------------------------- BatchNorm
def bn_stats(r, mov_mean, mov_var, dtype=np.float64):
    """tf.contrib.layers.batch_norm(is_training=True, decay=0.9) on r [B,H,W,C]: mean and BIASED variance over (B,H,W) -- tf.nn.moments: the mean
    of the squared differences from the mean --, rstd = 1/sqrt(var + eps); the moving mean takes the batch mean, the moving variance the
    Bessel-corrected one (the fused kernel's), without the factor when there is a single sample.  -> dict of [C] arrays in `dtype`."""
    C = r.shape[-1]
    x = np.asarray(r).astype(dtype).reshape(-1, C)
    N = x.shape[0]
    mean = (_sum(x, 0) / N).astype(dtype)
    d = x - mean
    var = (_sum(d * d, 0) / N).astype(dtype)
    rstd = (dtype(1) / np.sqrt(var + dtype(BN_EPS))).astype(dtype)
    unb = var * dtype(N / (N - 1.0)) if N > 1 else var
    decay = dtype(BN_DECAY)
    return dict(mean=mean, var=var, rstd=rstd,
                mov_mean=(np.asarray(mov_mean).astype(dtype) * decay + (dtype(1) - decay) * mean).astype(dtype),
                mov_var=(np.asarray(mov_var).astype(dtype) * decay + (dtype(1) - decay) * unb).astype(dtype))


def bn_apply(r, mean, rstd, gamma, beta, dtype=np.float64):
    """y = gamma * (r - mean) * rstd + beta."""
    t = lambda a: np.asarray(a).astype(dtype)
    return ((t(r) - t(mean)) * t(rstd) * t(gamma) + t(beta)).astype(dtype)


def bn_bwd(dy, r, mean, rstd, gamma, dy_scale=1.0, dtype=np.float64):
    """Backward of y = BN(r), r = relu(z), given dy * dy_scale: with xhat = (r - mean) rstd,
    dbeta = sum dy, dgamma = sum dy xhat, dr = gamma rstd (dy - dbeta / N - xhat dgamma / N), dz = dr where r > 0 and 0 elsewhere, dbias = sum dz.
    -> dict(dz [B,H,W,C], dgamma, dbeta, dbias [C]) in `dtype`."""
    t = lambda a: np.asarray(a).astype(dtype)
    C = r.shape[-1]
    g = t(dy) * dtype(dy_scale)
    rr, m, rs, ga = t(r), t(mean), t(rstd), t(gamma)
    N = rr.size // C
    xhat = (rr - m) * rs
    dbeta = _sum(g.reshape(-1, C), 0).astype(dtype)
    dgamma = _sum((g * xhat).reshape(-1, C), 0).astype(dtype)
    dr = ga * rs * (g - dbeta / dtype(N) - xhat * (dgamma / dtype(N)))
    dz = np.where(rr > 0, dr, dtype(0)).astype(dtype)
    return dict(dz=dz, dgamma=dgamma, dbeta=dbeta, dbias=_sum(dz.reshape(-1, C), 0).astype(dtype))


# --------------------------------------------------------------------------- 2x2/2 SAME max pool
def _slots(y):
    """The four window slots in row-major order: (values [B,Ho,Wo,C] with -inf outside the map, inside mask)."""
    B, H, W, C = y.shape
    Ho, Wo = (H + 1) // 2, (W + 1) // 2
    yp = np.full((B, 2 * Ho, 2 * Wo, C), -np.inf, y.dtype)
    yp[:, :H, :W] = y
    inside = np.zeros((2 * Ho, 2 * Wo), bool)
    inside[:H, :W] = True
    return [(yp[:, dy::2, dx::2], inside[dy::2, dx::2][None, :, :, None]) for dy in (0, 1) for dx in (0, 1)]


def max_pool(y):
    """tf.nn.max_pool(y, 2, 2, 'SAME') (main.py:172-174): odd extents end in half windows; exact in any dtype."""
    s = _slots(y)
    return np.maximum(np.maximum(s[0][0], s[1][0]), np.maximum(s[2][0], s[3][0]))


def max_pool_argmax(y):
    """Slot (0..3, row-major in the window) of each window's FIRST maximum (TF MaxPoolGrad walks the window in that order and keeps a later
    element only when it is strictly greater).  [B,Ho,Wo,C] int."""
    s = _slots(y)
    best, k = s[0][0].copy(), np.zeros(s[0][0].shape, np.int64)
    for i in (1, 2, 3):
        better = s[i][1] & (s[i][0] > best)
        best = np.where(better, s[i][0], best)
        k = np.where(better, i, k)
    return k


def max_pool_bwd(y, dp):
    """dy [B,H,W,C]: dp at the first maximum of each window, 0 elsewhere."""
    B, H, W, C = y.shape
    Ho, Wo = (H + 1) // 2, (W + 1) // 2
    k = max_pool_argmax(y)
    out = np.zeros((B, 2 * Ho, 2 * Wo, C), dp.dtype)
    for i, (dy, dx) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
        out[:, dy::2, dx::2] = np.where(k == i, dp, 0)
    return np.ascontiguousarray(out[:, :H, :W])


# --------------------------------------------------------------------------- adjoint of the TF-1 bilinear resize
def _adjoint_axis(g, axis, n_in, dtype):
    """Transpose of the 1-D operator out[o] = (1 - t[o]) in[lo[o]] + t[o] in[hi[o]] of jcm_oracle.resize_weights_tf1, along `axis` (moved to front)."""
    n_out = g.shape[axis]
    lo, hi, t = O.resize_weights_tf1(n_out, n_in)
    t = t.astype(dtype)
    g = np.moveaxis(g, axis, 0)
    shp = (n_out,) + (1,) * (g.ndim - 1)
    acc = np.zeros((n_in,) + g.shape[1:], np.float64)
    np.add.at(acc, lo, (((dtype(1) - t).reshape(shp)) * g).astype(np.float64))
    np.add.at(acc, hi, (t.reshape(shp) * g).astype(np.float64))
    return np.moveaxis(acc.astype(dtype), 0, axis)


def resize_bwd(dy, h, w, scale=1.0, dtype=np.float64):
    """dx [B,h,w,C] = scale * R^T dy for the operator R of oracle.resize_bilinear_tf1 from h x w to dy's H x W (hi is clamped to the last row /
    column: there both taps of an output land on the same source)."""
    g = np.asarray(dy).astype(dtype)
    return (_adjoint_axis(_adjoint_axis(g, 1, h, dtype), 2, w, dtype) * dtype(scale)).astype(dtype)


# --------------------------------------------------------------------------- losses
def softmax_ce(logits, target, gscale=1.0, dtype=np.float64):
    """main.py:220-240 per (image, joint) map: softmax over the HW pixels; logits [B,HW,K], target [B,HW,Kt] (first K channels).
    loss [B,K] = -sum_px t log_softmax(z); backprop [B,HW,K] = gscale * (softmax - t): TF-1.x's softmax_cross_entropy_with_logits gradient, which
    is the derivative only where the target map sums to one."""
    z = np.asarray(logits).astype(dtype)
    K = z.shape[2]
    t = np.asarray(target)[:, :, :K].astype(dtype)
    zs = z - z.max(axis=1, keepdims=True)
    e = np.exp(zs)
    se = _sum(e, 1).astype(dtype)[:, None, :]
    loss = _sum(t * (np.log(se) - zs), 1).astype(dtype)
    return loss, (dtype(gscale) * (e / se - t)).astype(dtype)


def softmax_bwd(p, g, dtype=np.float64):
    """Gradient through p = softmax over the pixels: p * (g - sum_px p g); p [B,HW,K], g [B,HW,ldg] (first K channels)."""
    pp = np.asarray(p).astype(dtype)
    gg = np.asarray(g)[:, :, :pp.shape[2]].astype(dtype)
    s = _sum(pp * gg, 1).astype(dtype)[:, None, :]
    return (pp * (gg - s)).astype(dtype)


# --------------------------------------------------------------------------- the bound
def bound(ref32, ref64):
    """Per tensor: 4 x the distance of the float32 mode from the float64 one (the project's customary margin over a measured distance) plus
    2^-22 max|ref64| (tensors where the float32 mode happens to be exact)."""
    ref64 = np.asarray(ref64, np.float64)
    return 4.0 * float(np.abs(np.asarray(ref32, np.float64) - ref64).max()) + 2.0 ** -22 * float(np.abs(ref64).max())


def near_zero(r):
    """Entries whose ReLU decision can differ between precisions: 0 < |r| < 2^-20 max|r| (exact zeros are decided alike everywhere)."""
    a = np.abs(np.asarray(r, np.float64))
    return (a > 0) & (a < 2.0 ** -20 * a.max())


def post_relu(rs, shape, shift=0.0):
    """Post-ReLU draws: max(N(shift, 1), 0) in float32 -- about half exact zeros at shift 0, no near-zeros to speak of."""
    return np.maximum(rs.standard_normal(shape) + shift, 0).astype(np.float32)
