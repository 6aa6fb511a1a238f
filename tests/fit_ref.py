"""The letterbox fit restated in float64 numpy (include/jcm.h: jcm_fit_images); nothing here is shared with the library.  It is
the bar for the device: every sum runs tap by tap in ascending order with elementwise array operations over the output pixels -- no np.dot, no
einsum, which reorder or fuse -- so the device's bytes are expected to equal these bit for bit."""
import numpy as np

# (h, w), (OH, OW) -> (y0, x0, ch, cw): the known answers of the geometry (the issue's table)
GEOMETRY_KAT = (
    ((7, 5), (12, 18), (0, 4, 12, 9)),
    ((50, 31), (12, 18), (0, 5, 12, 7)),
    ((13, 40), (12, 18), (3, 0, 6, 18)),
    ((1, 1), (12, 18), (0, 3, 12, 12)),
    ((12, 18), (12, 18), (0, 0, 12, 18)),
    ((37, 53), (24, 36), (0, 1, 24, 34)),
    ((3, 200), (24, 36), (11, 0, 1, 36)),
)


def kat_images():
    """The seven images of the table from one RandomState(0), drawn in the table's order."""
    rs = np.random.RandomState(0)
    return [rs.randint(0, 256, (h, w, 3)).astype(np.uint8) for (h, w), _, _ in GEOMETRY_KAT]


def geometry(h, w, OH, OW):
    """(y0, x0, ch, cw), integers only."""
    h, w, OH, OW = int(h), int(w), int(OH), int(OW)
    if OH * w <= OW * h:
        ch, cw = OH, max(1, (2 * w * OH + h) // (2 * h))
    else:
        cw, ch = OW, max(1, (2 * h * OW + w) // (2 * w))
    return (OH - ch) // 2, (OW - cw) // 2, ch, cw


def axis_taps(n, m):
    """Per output o of m: (lo, weights float64 [hi - lo]) over n source samples."""
    f = np.float64(n) / np.float64(m)
    sup = max(f, np.float64(1.0))
    taps = []
    for o in range(m):
        c = (np.float64(o) + 0.5) * f
        lo = max(0, int(np.floor(c - sup)))
        hi = min(n, int(np.ceil(c + sup)))
        t = [max(np.float64(0.0), np.float64(1.0) - np.abs(((np.float64(i) + 0.5) - c) / sup)) for i in range(lo, hi)]
        T = np.float64(0.0)
        for v in t:
            T = T + v
        taps.append((lo, np.array([v / T for v in t], np.float64)))
    return taps


def _table(taps):
    """Taps of every output padded to the longest: lo int [m], count int [m], weights [m, longest] (zeros behind the count)."""
    longest = max(len(wt) for _, wt in taps)
    lo = np.array([l for l, _ in taps], np.int64)
    cnt = np.array([len(wt) for _, wt in taps], np.int64)
    wgt = np.zeros((len(taps), longest), np.float64)
    for o, (_, wt) in enumerate(taps):
        wgt[o, :len(wt)] = wt
    return lo, cnt, wgt


def resample(img, ch, cw):
    """img uint8 [h,w,C] -> uint8 [ch,cw,C]: the row sums first (ascending source column), then the column sum (ascending source row).  A tap
    beyond an output's count is skipped by np.where, not added with a zero weight: every sum has exactly the operations of the statement."""
    h, w, C = img.shape
    p = img.astype(np.float64)
    lox, nx, wx = _table(axis_taps(w, cw))
    loy, ny, wy = _table(axis_taps(h, ch))
    rows = np.zeros((h, cw, C), np.float64)
    for i in range(wx.shape[1]):
        live = i < nx
        col = np.minimum(lox + i, w - 1)
        rows = np.where(live[None, :, None], rows + wx[None, :, i, None] * p[:, col, :], rows)
    acc = np.zeros((ch, cw, C), np.float64)
    for j in range(wy.shape[1]):
        live = j < ny
        row = np.minimum(loy + j, h - 1)
        acc = np.where(live[:, None, None], acc + wy[:, j, None, None] * rows[row, :, :], acc)
    return np.minimum(255, np.maximum(0, np.floor(acc + 0.5).astype(np.int64))).astype(np.uint8)


def fit(img, OH, OW, pad=0):
    """One image into its frame: (uint8 [OH,OW,C], (y0, x0, ch, cw))."""
    h, w, C = img.shape
    y0, x0, ch, cw = geometry(h, w, OH, OW)
    out = np.full((OH, OW, C), pad, np.uint8)
    out[y0:y0 + ch, x0:x0 + cw] = resample(img, ch, cw)
    return out, (y0, x0, ch, cw)


def fit_batch(images, OH, OW, pad=0):
    outs, geoms = zip(*(fit(im, OH, OW, pad) for im in images))
    return np.stack(outs), np.array(geoms, np.int32)


def as_f32(u8):
    """The float output: byte / float32(255), the one conversion of the byte entries (csrc/u8.h)."""
    return u8.astype(np.float32) / np.float32(255)


def pack(images, lead=1, gap=1):
    """The images back to back in one byte buffer at ODD byte offsets (every image is 3 * h * w bytes; a filler byte keeps the next offset odd):
    (buffer uint8 [n], desc int64 [B,3] = (offset, h, w)).  The filler bytes are 0xEE."""
    parts, desc, off = [np.full(lead, 0xEE, np.uint8)], [], lead
    for im in images:
        if off % 2 == 0:
            parts.append(np.full(gap, 0xEE, np.uint8))
            off += gap
        desc.append((off, im.shape[0], im.shape[1]))
        parts.append(im.reshape(-1))
        off += im.size
    return np.concatenate(parts), np.array(desc, np.int64)
