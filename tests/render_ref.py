"""The pose renderer restated in numpy (include/jcm.h: jcm_render_poses); nothing here is shared with the library.  Both layers
are written in the order the header states -- float64 elementwise array operations from exact integers, then integer arithmetic -- so the
device's bytes are expected to equal these bit for bit."""
import numpy as np

SUB = np.array([-6, -2, 2, 6], np.int64)      # the sub-samples of a pixel, sixteenths around its centre


def coverage(h, w, ay, ax, by, bx, r):
    """int64 [h,w]: how many of the 16 sub-samples of every pixel lie in the capsule."""
    sy = (16 * np.arange(h, dtype=np.int64)[:, None] + SUB[None, :]).reshape(h, 1, 4, 1)
    sx = (16 * np.arange(w, dtype=np.int64)[:, None] + SUB[None, :]).reshape(1, w, 1, 4)
    ey, ex = (sy - ay).astype(np.float64), (sx - ax).astype(np.float64)
    fy, fx = (sy - by).astype(np.float64), (sx - bx).astype(np.float64)
    dy, dx = np.float64(by - ay), np.float64(bx - ax)
    ee = ey * ey + ex * ex
    t = ey * dy + ex * dx
    L2 = dy * dy + dx * dx
    rr = np.float64(r) * np.float64(r)
    at_a = ee <= rr
    at_b = fy * fy + fx * fx <= rr
    along = ee * L2 - t * t <= rr * L2
    inside = np.where((L2 == 0) | (t <= 0), at_a, np.where(t >= L2, at_b, along))
    return inside.sum(axis=(2, 3)).astype(np.int64)


def draw(img, prims):
    """img uint8 [h,w,3], prims int [n,7] = (ay, ax, by, bx, r, rgb, alpha) in painter's order -> uint8 [h,w,3]."""
    h, w, _ = img.shape
    v = img.astype(np.int64)
    for ay, ax, by, bx, r, rgb, alpha in np.asarray(prims, np.int64).reshape(-1, 7):
        ca = coverage(h, w, int(ay), int(ax), int(by), int(bx), int(r))[:, :, None] * int(alpha)
        colour = np.array([(rgb >> 16) & 255, (rgb >> 8) & 255, rgb & 255], np.int64)[None, None, :]
        v = (v * (4080 - ca) + colour * ca + 2040) // 4080
    return v.astype(np.uint8)


def _cells(n, content, origin, stride, cells):
    f = (np.arange(n, dtype=np.float64) + 0.5) * np.float64(content) / np.float64(n) - 0.5 + np.float64(origin)
    c = np.minimum(np.maximum(f / np.float64(stride), 0.0), np.float64(cells - 1))
    i = np.floor(c).astype(np.int64)
    return i, np.minimum(i + 1, cells - 1), c - i.astype(np.float64)


def tint(img, hm, geom, heat_mask, heat_gain, stride):
    """img uint8 [h,w,3], hm float32 [hh,hw,K], geom (y0, x0, ch, cw) -> uint8 [h,w,3]."""
    h, w, _ = img.shape
    hh, hw, K = hm.shape
    y0, x0, ch, cw = (int(g) for g in geom[:4])
    iy, iy1, ty = _cells(h, ch, y0, stride, hh)
    ix, ix1, tx = _cells(w, cw, x0, stride, hw)
    ty, tx = ty[:, None], tx[None, :]
    v = img.astype(np.int64)
    for j in range(K):
        M = hm[:, :, j].max()
        if not M > 0:
            continue
        m = hm[:, :, j].astype(np.float64)
        v00, v01 = m[iy][:, ix], m[iy][:, ix1]
        v10, v11 = m[iy1][:, ix], m[iy1][:, ix1]
        s = (1 - ty) * ((1 - tx) * v00 + tx * v01) + ty * ((1 - tx) * v10 + tx * v11)
        q = np.minimum(255.0, np.maximum(0.0, np.floor(s * 255.0 / np.float64(M) + 0.5))).astype(np.int64)
        add = (q * int(heat_gain) + 127) // 255
        for c in range(3):
            if int(heat_mask[j]) >> c & 1:
                v[:, :, c] = np.minimum(255, v[:, :, c] + add)
    return v.astype(np.uint8)


def render(images, prims, hm=None, geom=None, heat_mask=None, heat_gain=255, stride=8):
    """images: a list of uint8 [h,w,3]; prims int [NP,8] = (image, ay, ax, by, bx, r, rgb, alpha); hm float32 [B,hh,hw,K] -> a list of uint8 [h,w,3]."""
    prims = np.asarray(prims, np.int64).reshape(-1, 8)
    out = []
    for b, im in enumerate(images):
        v = im if hm is None else tint(im, hm[b], geom[b], heat_mask, heat_gain, stride)
        out.append(draw(v, prims[prims[:, 0] == b, 1:]))
    return out


def render_packed(buf, desc, out, prims, **heat):
    """The packed form of the C entry: image b at desc[b] = (offset, h, w) of buf is rendered into the same bytes of a copy of `out`."""
    res = np.array(out, np.uint8, copy=True)
    images = [buf[o:o + 3 * h * w].reshape(h, w, 3) for o, h, w in desc]
    for (o, h, w), r in zip(desc, render(images, prims, **heat)):
        res[o:o + 3 * h * w] = r.reshape(-1)
    return res
