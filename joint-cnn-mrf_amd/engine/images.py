"""Images of any size on their way in and out: the letterbox fits, poses drawn onto the source images, and rendered synthetic people."""
import numpy as np
import torch

from .. import _lib
from ._core import _i32p, _i64p, _u8p


class Images:
    def fit_images(self, images, out_hw=(480, 720), pad=0, dtype=torch.uint8, out=None):
        """Images of any size into the frame the tower reads (include/jcm.h: jcm_fit_images): `images` is a list of uint8 [h,w,3]
        torch tensors or numpy arrays, on the host or on the engine's device, of mixed sizes.  Each is resampled, aspect preserved and
        antialiased, into the centred content rectangle of an out_hw frame; the rest of the frame is the byte `pad`.  One packed device buffer,
        one launch per 64 images.  Returns (x [B,OH,OW,3] of `dtype` -- torch.uint8, or torch.float32 = byte / 255 -- and geom, host int32 [B,6] =
        (y0, x0, ch, cw, h, w): the content rectangle and the source size, what evaluation.fit_to_source takes).  out: a tensor to write into
        instead of a new one.  Sizes, pad and the reduction limit (32 per axis) are checked by the library."""
        ts, desc, off, dtype = self._fit_check(images, dtype)
        return self._fit_run('jcm_fit_images', ts, desc, off, desc, desc[:, 1:], out_hw, pad, dtype, out)

    def _fit_check(self, images, dtype):
        """The input checks fit_images and fit_windows share -> (the images as uint8 torch tensors, desc int64 [B,3] = (byte offset in the packed
        buffer, h, w), the buffer's bytes, dtype)."""
        if not isinstance(images, (list, tuple)) or len(images) == 0:
            raise ValueError('images must be a non-empty list of uint8 [h,w,3] images')
        if dtype not in (torch.uint8, torch.float32):
            raise TypeError('dtype must be torch.uint8 or torch.float32, got %s' % (dtype,))
        C = 3
        ts = []
        for i, im in enumerate(images):
            name = 'images[%d]' % i
            if isinstance(im, np.ndarray):
                if im.dtype != np.uint8:
                    raise TypeError('%s must be uint8, got %s' % (name, im.dtype))
                im = torch.from_numpy(np.ascontiguousarray(im))
            elif not isinstance(im, torch.Tensor):
                raise TypeError('%s must be a torch tensor or a numpy array' % name)
            if im.dtype != torch.uint8:
                raise TypeError('%s must be %s, got %s' % (name, torch.uint8, im.dtype))
            if im.dim() != 3 or im.shape[2] != C or im.shape[0] < 1 or im.shape[1] < 1:
                raise ValueError('%s must be [h,w,3] (HWC), got shape %s' % (name, tuple(im.shape)))
            if im.device.type != 'cpu' and im.device != self.device:
                raise ValueError('%s is on %s, engine is on %s' % (name, im.device, self.device))
            ts.append(im)
        desc = np.empty((len(ts), 3), np.int64)
        off = 0
        for i, im in enumerate(ts):
            desc[i] = (off, im.shape[0], im.shape[1])
            off += im.numel()
        return ts, desc, off, dtype

    def _fit_pack(self, ts, desc, off):
        """The images ts back to back in one new device buffer of `off` bytes, image i at byte desc[i, 0]."""
        src = self._new(off, dtype=torch.uint8)
        if all(im.device.type == 'cpu' for im in ts):      # one packed host buffer, one copy
            src.copy_(torch.cat([im.reshape(-1) for im in ts]))
        else:
            for i, im in enumerate(ts):
                src[int(desc[i, 0]):int(desc[i, 0]) + im.numel()].copy_(im.reshape(-1))
        return src

    def render_poses(self, images, prims, hm=None, geom=None, heat_mask=None, heat_gain=255, stride=8):
        """Poses drawn onto images of any size (include/jcm.h: jcm_render_poses): `images` as for fit_images; `prims` int [NP,8] =
        (image, ay, ax, by, bx, r, rgb = 0xRRGGBB, alpha), capsules in sixteenths of a pixel, sorted by image and applied in listing order (what
        predict.skeleton_primitives makes; NP = 0 draws none).  hm: the heat tint under them -- a device float32 [B,hh,hw,K] tensor, or a list of B
        [hh,hw,K] device tensors, the maps of the frame the images were fitted into; then geom int [B,4 or 6], the fit of every image ((y0, x0, ch,
        cw, ..), what fit_images returns), heat_mask uint8 [K] (bits 0, 1, 2: joint j tints R, G, B), heat_gain 0..255 and stride, frame pixels per
        map cell.  The images are packed as fit_images packs them and drawn on in place there: returns a list of uint8 [h,w,3] device tensors,
        views into that one buffer.  Nothing synchronises; every range is checked by the library."""
        ts, desc, off, _ = self._fit_check(images, torch.uint8)
        B = len(ts)
        pr = np.asarray(prims)
        if pr.size == 0:
            pr = np.zeros((0, 8), np.int32)
        if pr.dtype.kind not in 'iu' or pr.ndim != 2 or pr.shape[1] != 8:
            raise ValueError('prims must be an integer array [NP,8] = (image, ay, ax, by, bx, r, rgb, alpha), got %s %s' % (pr.dtype, pr.shape))
        if pr.shape[0] and (pr.min() < -2 ** 31 or pr.max() >= 2 ** 31):
            raise ValueError('prims holds a value outside int32')
        pr = np.ascontiguousarray(pr, dtype=np.int32)
        hh = hw = K = 0
        g4 = mask = None
        if hm is not None:
            if isinstance(hm, (list, tuple)):
                hm = torch.stack(list(hm))
            self._chk(hm, 4, 'hm')
            hh, hw, K = int(hm.shape[1]), int(hm.shape[2]), int(hm.shape[3])
            if hm.shape[0] != B:
                raise ValueError('hm holds %d images, images %d' % (hm.shape[0], B))
            if geom is None or heat_mask is None:
                raise ValueError('hm needs geom (the fit of every image) and heat_mask (the channels every joint tints)')
            g4 = np.asarray(geom)
            if g4.dtype.kind not in 'iu' or g4.ndim != 2 or g4.shape[0] != B or g4.shape[1] < 4:
                raise ValueError('geom must be an integer array [%d, 4 or 6] = (y0, x0, ch, cw, ..), got %s %s' % (B, g4.dtype, g4.shape))
            g4 = np.ascontiguousarray(g4[:, :4], dtype=np.int32)
            mask = np.ascontiguousarray(np.asarray(heat_mask), dtype=np.uint8).reshape(-1)
            if mask.shape[0] != K:
                raise ValueError('heat_mask has %d entries, hm %d joints' % (mask.shape[0], K))
        buf = self._fit_pack(ts, desc, off)
        self._on_stream(buf, *([hm] if hm is not None else []))
        self._call('jcm_render_poses', self._p(buf), off, _i64p(desc), B, self._p(buf), _i32p(pr) if pr.shape[0] else None, pr.shape[0],
                   self._p(hm), hh, hw, K, int(stride), _i32p(g4) if g4 is not None else None, _u8p(mask) if mask is not None else None, int(heat_gain))
        return [buf[int(d[0]):int(d[0]) + int(d[1] * d[2] * 3)].view(int(d[1]), int(d[2]), 3) for d in desc]

    def synth_people(self, records, prims, H, W, out=None, dtype=torch.uint8):
        """Rendered people (include/jcm.h: jcm_synth_people): `records` int [B,20], one scene record per image, and `prims` int
        [NP,16], the primitives the records name (what synth.people_batch makes; NP = 0: backgrounds only), both host arrays -> [B,H,W,3] on the
        device, torch.uint8 or torch.float32 (= byte / 255).  out: a contiguous device tensor of that shape and dtype to write into instead of
        a new one (a view at any byte offset for uint8).  One launch; nothing synchronises; every range is checked by the library."""
        rec, pr = np.asarray(records), np.asarray(prims)
        if pr.size == 0:
            pr = np.zeros((0, _lib.SYNTH_PRIM_INTS), np.int32)
        for a, n, name in ((rec, _lib.SYNTH_REC_INTS, 'records'), (pr, _lib.SYNTH_PRIM_INTS, 'prims')):
            if a.dtype.kind not in 'iu' or a.ndim != 2 or a.shape[1] != n:
                raise ValueError('%s must be an integer array [.,%d], got %s %s' % (name, n, a.dtype, a.shape))
            if a.size and (a.min() < -2 ** 31 or a.max() >= 2 ** 31):
                raise ValueError('%s holds a value outside int32' % name)
        if rec.shape[0] < 1:
            raise ValueError('records must hold at least one image')
        if dtype not in (torch.uint8, torch.float32):
            raise TypeError('dtype must be torch.uint8 or torch.float32, got %s' % (dtype,))
        rec, pr = np.ascontiguousarray(rec, dtype=np.int32), np.ascontiguousarray(pr, dtype=np.int32)
        B, H, W = rec.shape[0], int(H), int(W)
        if out is None and (H < 1 or W < 1 or B * H * W * 3 >= 2 ** 40):
            raise ValueError('synth_people: H and W >= 1 and an output below 2^40 elements are expected, got %d x %d x %d' % (B, H, W))
        out = self._given_or_new(out, 'out', B, H, W, 3, dtype=dtype)
        if tuple(out.shape) != (B, H, W, 3):
            raise ValueError('out must be [%d,%d,%d,3], got %s' % (B, H, W, tuple(out.shape)))
        self._on_stream(out)
        self._call('jcm_synth_people', _i32p(rec), B, _i32p(pr) if pr.shape[0] else None, pr.shape[0], H, W, int(dtype == torch.float32), self._p(out))
        return out

    def _fit_run(self, entry, ts, desc, off, rows, sizes, out_hw, pad, dtype, out):
        """What fit_images and fit_windows share once the descriptor array is built: the output frame (`out` checked, or a new one), the images
        ts back to back in one device buffer of `off` bytes (desc[:, 0] their offsets), the library's `entry` on the int64 descriptor `rows`
        [n, 3 or 7], and geom [n,6] = the content rectangles it returns + `sizes` [n,2]."""
        OH, OW = int(out_hw[0]), int(out_hw[1])
        n, C = rows.shape[0], 3
        out = self._given_or_new(out, 'out', n, OH, OW, C, dtype=dtype)
        if tuple(out.shape) != (n, OH, OW, C):
            raise ValueError('out must be [%d,%d,%d,%d], got %s' % (n, OH, OW, C, tuple(out.shape)))
        src = self._fit_pack(ts, desc, off)
        geom = np.empty((n, 6), np.int32)
        g4 = np.empty((n, 4), np.int32)
        self._on_stream(src, out)
        self._call(entry, self._p(src), off, _i64p(rows), n, C, OH, OW, int(pad), int(dtype == torch.float32), self._p(out), _i32p(g4))
        geom[:, :4] = g4
        geom[:, 4:] = sizes
        return out, geom

    def fit_windows(self, images, windows, out_hw=(480, 720), pad=0, dtype=torch.uint8, out=None):
        """Rectangles of images of any size into the frame the tower reads (include/jcm.h: jcm_fit_windows): `images` as for
        fit_images; `windows` int [NW,5] = (image index, y0, x0, h, w), the convention of window_resize: rows [y0, y0 + h) and columns
        [x0, x0 + w) of that image, which may reach past any edge (the byte `pad` stands where the image has no sample, and takes part in the
        filter) and may name an image more than once.  Each window is fitted exactly as fit_images would fit the padded crop.  One packed
        device buffer, one launch per 64 windows.  Returns (x [NW,OH,OW,3] of `dtype`, geom host int32 [NW,6] = (y0, x0, ch, cw, h, w) with the
        WINDOW's size: what evaluation.window_to_source takes together with `windows`).  A window that shares no pixel with its image, and the
        size and reduction limits, are refused by the library."""
        ts, desc, off, dtype = self._fit_check(images, dtype)
        wins = np.asarray(windows)
        if wins.dtype.kind not in 'iu' or wins.ndim != 2 or wins.shape[1] != 5 or wins.shape[0] < 1:
            raise ValueError('windows must be an integer array [NW,5] = (image index, y0, x0, h, w), got %s %s' % (wins.dtype, wins.shape))
        wins = wins.astype(np.int64)
        if wins[:, 0].min() < 0 or wins[:, 0].max() >= len(ts):
            raise ValueError('windows name images %d..%d; there are %d' % (wins[:, 0].min(), wins[:, 0].max(), len(ts)))
        d7 = np.ascontiguousarray(np.concatenate([desc[wins[:, 0]], wins[:, 1:]], axis=1))
        return self._fit_run('jcm_fit_windows', ts, desc, off, d7, wins[:, 3:], out_hw, pad, dtype, out)
