"""Heat-map peaks restated in numpy, pixel by pixel, with np.float32 comparisons: what the GPU tests hold jcm_hm_peaks to
bit for bit.  Shares no code with the library; tests/test_peaks_cpu.py pins it with hand-computed answers.

For one map v [HH,WW] and i = r*WW + c:
  local maximum p: v(p) > threshold, v(p) >= v(q) for every in-bounds 8-neighbour q, v(p) > v(q) for those q with a smaller index;
  order:           value descending, then index ascending; the first min(P, n);
  offset:          +0.25 / -0.25 towards the strictly higher of the two neighbours along an axis when both exist, else 0."""
import numpy as np

NEIGHBOURS = [(-1, -1), (-1, 0), (-1, 1), (0, -1), (0, 1), (1, -1), (1, 0), (1, 1)]


def local_maxima(v, threshold):
    """[(row, col)] of the local maxima of one map, in row-major order."""
    v = np.asarray(v, np.float32)
    thr = np.float32(threshold)
    HH, WW = v.shape
    found = []
    for r in range(HH):
        for c in range(WW):
            x = v[r, c]
            if not x > thr:
                continue
            ok = True
            for dr, dc in NEIGHBOURS:
                rr, cc = r + dr, c + dc
                if rr < 0 or rr >= HH or cc < 0 or cc >= WW:
                    continue
                q = v[rr, cc]
                earlier = rr * WW + cc < r * WW + c
                if (earlier and not x > q) or (not earlier and not x >= q):
                    ok = False
                    break
            if ok:
                found.append((r, c))
    return found


def _offset(lo, hi):
    if hi > lo:
        return np.float32(0.25)
    if hi < lo:
        return np.float32(-0.25)
    return np.float32(0)


def peaks_of_map(v, P, threshold, cand=None):
    """-> cells int32 [P,2], offsets fp32 [P,2], scores fp32 [P], count.  cand: local_maxima(v, threshold) when the caller has it already."""
    v = np.asarray(v, np.float32)
    HH, WW = v.shape
    cand = local_maxima(v, threshold) if cand is None else cand
    # value descending, then index ascending: a stable selection, one winner at a time
    chosen = []
    left = list(cand)
    while left and len(chosen) < P:
        best = 0
        for j in range(1, len(left)):
            if v[left[j]] > v[left[best]]:      # `left` is in index order: the first of equal values stays
                best = j
        chosen.append(left.pop(best))
    cells = np.full((P, 2), -1, np.int32)
    offsets = np.zeros((P, 2), np.float32)
    scores = np.zeros(P, np.float32)
    for s, (r, c) in enumerate(chosen):
        cells[s] = (r, c)
        scores[s] = v[r, c]
        if r - 1 >= 0 and r + 1 < HH:
            offsets[s, 0] = _offset(v[r - 1, c], v[r + 1, c])
        if c - 1 >= 0 and c + 1 < WW:
            offsets[s, 1] = _offset(v[r, c - 1], v[r, c + 1])
    return cells, offsets, scores, len(chosen)


def all_local_maxima(hm, threshold=0.0):
    """{(b, k): local_maxima of map k of image b}: the part of hm_peaks that does not depend on P, for tests that ask several P of one input."""
    hm = np.asarray(hm, np.float32)
    return {(b, k): local_maxima(hm[b, :, :, k], threshold) for b in range(hm.shape[0]) for k in range(hm.shape[3])}


def hm_peaks(hm, P, threshold=0.0, cand=None):
    """hm [B,HH,WW,K] -> {'cells' int32 [B,K,P,2], 'offsets' fp32 [B,K,P,2], 'scores' fp32 [B,K,P], 'count' int32 [B,K]}.
    cand: all_local_maxima(hm, threshold) when the caller has it already."""
    hm = np.asarray(hm, np.float32)
    B, HH, WW, K = hm.shape
    out = {'cells': np.empty((B, K, P, 2), np.int32), 'offsets': np.empty((B, K, P, 2), np.float32), 'scores': np.empty((B, K, P), np.float32),
           'count': np.empty((B, K), np.int32)}
    for b in range(B):
        for k in range(K):
            out['cells'][b, k], out['offsets'][b, k], out['scores'][b, k], out['count'][b, k] = peaks_of_map(hm[b, :, :, k], P, threshold,
                                                                                                                     None if cand is None else cand[b, k])
    return out


def softmax_maps(logits):
    """Spatial softmax of [B,HH,WW,K] logits in float32 (test input only: the kernel under test does no arithmetic)."""
    x = np.asarray(logits, np.float32)
    e = np.exp(x - x.max(axis=(1, 2), keepdims=True), dtype=np.float32)
    return (e / e.sum(axis=(1, 2), keepdims=True, dtype=np.float32)).astype(np.float32)
