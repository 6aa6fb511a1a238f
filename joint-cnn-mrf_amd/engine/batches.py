"""Training batches: the augmentations, and batches read through an index from a device-resident data set."""
import torch

from ._core import _f32p, _f64p, _host_index, _i32p


class Batches:
    def augment_train(self, x, y, params, x_out=None, y_out=None):
        """Training-time augmentation (augmentation.py:58-78): x [B,H,W,3], y [B,h,w,K+1] = y_in, params [B,6] device fp32
        (augmentation.draw_params / check_params) -> (x_out, y_out), new tensors unless given.  Enqueued on the engine's stream."""
        self._chk(x, 4, 'x')
        self._chk(y, 4, 'y')
        self._chk(params, 2, 'params')
        B, H, W, C = x.shape
        _, hh, hw, Ky = y.shape
        if C != 3 or y.shape[0] != B or Ky != self.n_joints + 1 or tuple(params.shape) != (B, 6):
            raise ValueError('augment_train expects x [B,H,W,3], y [B,h,w,%d], params [B,6]; got %s, %s, %s'
                             % (self.n_joints + 1, tuple(x.shape), tuple(y.shape), tuple(params.shape)))
        x_out, y_out = self._given_or_new(x_out, 'x_out', *x.shape), self._given_or_new(y_out, 'y_out', *y.shape)
        if x_out.shape != x.shape or y_out.shape != y.shape:
            raise ValueError('x_out / y_out must have the shapes of x / y')
        self._on_stream(x, y, params, x_out, y_out)      # tensors made on torch's current stream: the engine's stream waits for them, and keeps them alive
        self._call('jcm_augment_train', self._p(x), self._p(y), self._p(params), B, H, W, hh, hw, self._p(x_out), self._p(y_out))
        return x_out, y_out

    # ------------------------------------------------------------------ batches from a device-resident data set (dataset.py)
    def _chk_indexed(self, who, x_all, y_all, idx, params, x_out, y_out):
        """Shared checks of gather_batch / augment_train_indexed -> (host int32 indices, x_out, y_out).  The index RANGE is checked by the
        entry point itself (on the host, before any launch).  x_all: float32, or uint8 (a byte data set; the outputs are float32 either way)."""
        self._chk_img(x_all, 'x_all')
        self._chk(y_all, 4, 'y_all')
        N, H, W, C = x_all.shape
        if C != 3 or y_all.shape[0] != N or y_all.shape[3] != self.n_joints + 1 or N < 1:
            raise ValueError('%s expects x_all [N,H,W,3] and y_all [N,h,w,%d]; got %s, %s' % (who, self.n_joints + 1, tuple(x_all.shape), tuple(y_all.shape)))
        idx = _host_index(who, idx)
        B = idx.shape[0]
        if params is not None:
            self._chk(params, 2, 'params')
            if tuple(params.shape) != (B, 6):
                raise ValueError('%s expects params [%d,6] for %d indices; got %s' % (who, B, B, tuple(params.shape)))
        x_out, y_out = self._given_or_new(x_out, 'x_out', B, H, W, 3), self._given_or_new(y_out, 'y_out', B, *y_all.shape[1:])
        if tuple(x_out.shape) != (B, H, W, 3) or tuple(y_out.shape) != (B,) + tuple(y_all.shape[1:]):
            raise ValueError('x_out / y_out must be [%d,...] with the image / map shapes of the data set; got %s, %s' % (B, tuple(x_out.shape), tuple(y_out.shape)))
        self._on_stream(*[t for t in (x_all, y_all, params, x_out, y_out) if t is not None])
        return idx, x_out, y_out

    def gather_batch(self, x_all, y_all, idx, x_out=None, y_out=None):
        """x_out[b] = x_all[idx[b]], y_out[b] = y_all[idx[b]] (bit for bit): x_all [N,H,W,3], y_all [N,h,w,K+1] device fp32, idx HOST integers
        [B] in [0, N) (repeats allowed) -> (x_out, y_out), new tensors unless given.  Enqueued on the engine's stream; the host does not wait.
        x_all may be uint8: x_out[b] = float32(x_all[idx[b]]) / float32(255), correctly rounded (fp32, as always)."""
        idx, x_out, y_out = self._chk_indexed('gather_batch', x_all, y_all, idx, None, x_out, y_out)
        N, H, W, _ = x_all.shape
        self._call('jcm_gather_batch' + ('_u8' if x_all.dtype == torch.uint8 else ''), self._p(x_all), self._p(y_all), N, _i32p(idx), idx.shape[0],
                   H, W, y_all.shape[1], y_all.shape[2], self._p(x_out), self._p(y_out))
        return x_out, y_out

    def augment_train_indexed(self, x_all, y_all, idx, params, x_out=None, y_out=None):
        """augment_train of the images idx[b] of the data set (x_all, y_all) with params[b], read through the index: the same bits as
        gather_batch followed by augment_train, without the gathered copy.  x_all may be uint8 (a byte data set): the same bits as from the
        float data set float32(x_all) / float32(255)."""
        idx, x_out, y_out = self._chk_indexed('augment_train_indexed', x_all, y_all, idx, params, x_out, y_out)
        N, H, W, _ = x_all.shape
        self._call('jcm_augment_train_indexed' + ('_u8' if x_all.dtype == torch.uint8 else ''), self._p(x_all), self._p(y_all), N, _i32p(idx),
                   self._p(params), idx.shape[0], H, W, y_all.shape[1], y_all.shape[2], self._p(x_out), self._p(y_out))
        return x_out, y_out

    # ------------------------------------------------------------------ the affine augmentation (augmentation.py)
    def _affine_call(self, who, x, cells, idx, colour, geom, pad, x_out, y_out, width=None):
        """The checks and the call the two affine entries share; idx None: image b of x / cells itself; width None: the plain entries, else the
        antialiased ones (jcm_augment_affine_aa*) with that [B] array of filter half-widths."""
        from ..augmentation import check_affine, check_width
        u8 = self._chk_img(x, 'x_all' if idx is not None else 'x')
        self._chk(cells, 3, 'cells', torch.int32)
        N, H, W, C = x.shape
        if u8 and idx is None:
            raise TypeError('%s: x must be float32 (byte images are read through an index: augment_affine_indexed)' % who)
        if C != 3 or tuple(cells.shape) != (N, 10, 2) or N < 1 or self.n_joints != 9:
            raise ValueError('%s expects x [N,H,W,3] and cells [N,10,2] on an engine with n_joints == 9; got %s, %s, n_joints = %d'
                             % (who, tuple(x.shape), tuple(cells.shape), self.n_joints))
        if H % 8 or W % 8:
            raise ValueError('%s: images of %d x %d; a heat-map cell is 8 x 8 pixels, H and W must be multiples of 8' % (who, H, W))
        if idx is not None:
            idx = _host_index(who, idx)
        B = N if idx is None else idx.shape[0]
        colour, geom = check_affine(colour, geom)
        if colour.shape[0] != B:
            raise ValueError('%s: %d parameter rows for a batch of %d' % (who, colour.shape[0], B))
        aa, wp = ('_aa', (_f64p(check_width(width, B)),)) if width is not None else ('', ())
        hh, hw = H // 8, W // 8
        x_out, y_out = self._given_or_new(x_out, 'x_out', B, H, W, 3), self._given_or_new(y_out, 'y_out', B, hh, hw, 10)
        if tuple(x_out.shape) != (B, H, W, 3) or tuple(y_out.shape) != (B, hh, hw, 10):
            raise ValueError('x_out / y_out must be [%d,%d,%d,3] and [%d,%d,%d,10]; got %s, %s' % (B, H, W, B, hh, hw, tuple(x_out.shape), tuple(y_out.shape)))
        self._on_stream(x, cells, x_out, y_out)
        indexed = () if idx is None else (N, _i32p(idx))
        self._call('jcm_augment_affine' + aa + ('' if idx is None else '_indexed_u8' if u8 else '_indexed'), self._p(x), self._p(cells), *indexed,
                   _f32p(colour), _f64p(geom), *wp, B, H, W, hh, hw, float(pad), self._p(x_out), self._p(y_out))
        return x_out, y_out

    def augment_affine(self, x, cells, colour, geom, pad=0.0, x_out=None, y_out=None, width=None):
        """The affine augmentation: x [B,H,W,3] device fp32, cells [B,10,2] device int32 = the (row, col) heat-map cell of every channel's
        joint, colour [B,3] / geom [B,12] HOST arrays (augmentation.affine_geometry), pad the value outside the source -> (x_out [B,H,W,3], y_out
        [B,H/8,W/8,10]), new tensors unless given: one bilinear sample of the image through the inverse map, the targets redrawn as 3x3 blobs at the cells
        the forward map sends the joints to.  Enqueued on the engine's stream; the host does not wait.
        width: None, or a HOST float64 [B] array of filter half-widths in [1, 4] (augmentation.affine_footprint(geom)): the antialiased sample
         -- image b through a triangle filter of half-width width[b] source pixels, the plain sample's bits where that is exactly 1."""
        return self._affine_call('augment_affine', x, cells, None, colour, geom, pad, x_out, y_out, width)

    def augment_affine_indexed(self, x_all, cells_all, idx, colour, geom, pad=0.0, x_out=None, y_out=None, width=None):
        """augment_affine of the images idx[b] of the data set (x_all [N,H,W,3], cells_all [N,10,2]) read through the index: the same bits as gather_batch
        followed by augment_affine, without the gathered copy.  x_all may be uint8 (a byte data set): the same bits as from the float data set
        float32(x_all) / float32(255).  width: as in augment_affine."""
        return self._affine_call('augment_affine_indexed', x_all, cells_all, idx, colour, geom, pad, x_out, y_out, width)

    def joint_cells(self, y):
        """y [B,h,w,K+1] target maps -> int32 [B,K+1,2], the (row, col) of every channel's arg-max cell (the first maximum, as jcm_argmax_coords picks it): the
        cells the affine augmentation transforms when the data set did not keep them.  A blob cut by the border loses its true centre this way."""
        self._chk(y, 4, 'y')
        self._on_stream(y)
        with torch.cuda.stream(self._stream):      # the coordinates are written on the engine's stream
            return self.argmax_coords(y).permute(0, 2, 1).contiguous()
