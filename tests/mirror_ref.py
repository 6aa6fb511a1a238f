"""The two kernels of the mirrored test-time evaluation restated in numpy (include/jcm.h: jcm_mirror_pairs, jcm_mirror_merge),
with plain indexing and a sequential float64 loop over the copies -- nothing shared with csrc/mirror.hip."""
import numpy as np

HM_FLIP_PERM = [3, 4, 5, 0, 1, 2, 7, 6, 8, 9]      # augmentation.py:20: hm[3:6], hm[0:3], hm[7:8], hm[6:7], hm[8:10]


def mirror_pairs(x):
    """x [B,H,W,C] -> [2B,H,W,C]: out[2b] = x[b], out[2b+1][y][xx][c] = x[b][y][W-1-xx][c]."""
    x = np.asarray(x)
    B, H, W, C = x.shape
    out = np.empty((2 * B, H, W, C), x.dtype)
    for b in range(B):
        out[2 * b] = x[b]
        for xx in range(W):
            out[2 * b + 1, :, xx, :] = x[b, :, W - 1 - xx, :]
    return out


def mirror_merge(hm, group=2, perm=None):
    """hm [n*G,HH,WW,K] float32 -> [n,HH,WW,K] float32: out[i,y,x,k] = float32((v_0 + .. + v_{G-1}) / float64(G)), summed in float64 in the order
    g = 0 .. G-1, v_g = hm[i*G+g,y,x,k] for even g and hm[i*G+g,y,WW-1-x,perm[k]] for odd g."""
    hm = np.asarray(hm)
    assert hm.dtype == np.float32 and hm.ndim == 4 and group >= 2 and group % 2 == 0 and hm.shape[0] % group == 0
    N, HH, WW, K = hm.shape
    perm = HM_FLIP_PERM[:K] if perm is None else [int(p) for p in perm]
    assert sorted(perm) == list(range(K))
    n = N // group
    out = np.empty((n, HH, WW, K), np.float32)
    for i in range(n):
        s = np.zeros((HH, WW, K), np.float64)
        for g in range(group):
            m = hm[i * group + g]
            if g % 2:
                v = np.empty_like(m)
                for x in range(WW):
                    for k in range(K):
                        v[:, x, k] = m[:, WW - 1 - x, perm[k]]
            else:
                v = m
            s = s + v.astype(np.float64)
        with np.errstate(over='ignore'):
            out[i] = (s / np.float64(group)).astype(np.float32)
    return out
