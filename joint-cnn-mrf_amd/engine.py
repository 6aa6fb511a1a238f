"""Handle object over the C ABI: one Engine per (device, stream) holds the packed weights,
spatial-model tables and workspace that the reference keeps as module globals + a
tf.Session (SURVEY.md 8b 'Implicit state').  torch is used only to own device buffers."""
import ctypes

import numpy as np
import torch

from . import _lib, motion
from .motion import SEQ_EXCLUDE      # noqa: F401  (the default of seq_tracks; engine.SEQ_EXCLUDE stays importable)


def _hm_size(n):
    """Three SAME stride-2 stages (conv1 + two max-pools): ceil(ceil(ceil(n/2)/2)/2)."""
    for _ in range(3):
        n = (n + 1) // 2
    return n


def _precision(name):
    return {'fp32': _lib.JCM_PRECISION_F32, 'f32': _lib.JCM_PRECISION_F32, 'bf16': _lib.JCM_PRECISION_BF16}[name]


def _f32_conv(name):      # 'exact' = the default; 'split16' = the direct kernels on two fp16 parts per operand (fp16x3)
    if name not in ('exact', 'split16'):
        raise ValueError("f32_conv must be 'exact' or 'split16' (the bf16x6 arm 'split' was retired in round 5)")
    return {'exact': 0, 'split16': 2}[name]


def _flag(v):
    return int(bool(v))


# keyword of Engine.__init__ = key of jcm_set_option, and what turns the keyword's value into the option's
_INIT_OPTIONS = (('precision', _precision), ('n_joints', int), ('f32_conv', _f32_conv), ('micro_batch', int), ('conv9_fft', _flag), ('fft_single', _flag),
                 ('fft_t16', _flag), ('fft_fuse', int), ('fft_tiles', _flag), ('fft_logits_rows', _flag), ('call_order', _flag), ('split_min_wgs', int))


class Engine:
    """Owns a jcm_handle.  All tensor arguments are torch CUDA float32 NHWC, contiguous."""

    def __init__(self, device=0, precision='fp32', n_joints=9, stream=None, f32_conv=None, split_min_wgs=None, micro_batch=None, conv9_fft=None, call_order=None, fft_single=None, fft_t16=None, fft_fuse=None, fft_tiles=None, fft_logits_rows=None):
        if not torch.cuda.is_available():
            raise RuntimeError('joint-cnn-mrf_amd needs an MI355X (gfx950) GPU; torch.cuda.is_available() is False '
                               'and there is no CPU path')
        self._lib = _lib.load()
        self.device = torch.device('cuda', device if isinstance(device, int) else torch.device(device).index or 0)
        self.n_joints = int(n_joints)
        self.precision = precision
        self._stream = stream if stream is not None else torch.cuda.current_stream(self.device)
        h = ctypes.c_void_p()
        _lib.check(self._lib.jcm_create(self.device.index, ctypes.c_void_p(self._stream.cuda_stream), ctypes.byref(h)),
                   'jcm_create')
        self._h = h
        self._finalized = False
        self._shapes = {}      # name -> shape of the parameters given so far (act_summary: does a layer have BatchNorm?)
        given = dict(precision=precision, n_joints=self.n_joints, f32_conv=f32_conv, micro_batch=micro_batch, conv9_fft=conv9_fft, fft_single=fft_single, fft_t16=fft_t16,
                     fft_fuse=fft_fuse, fft_tiles=fft_tiles, fft_logits_rows=fft_logits_rows, call_order=call_order, split_min_wgs=split_min_wgs)
        for key, convert in _INIT_OPTIONS:      # the option of the same name (include/jcm.h); None leaves the library's default
            if given[key] is not None:
                self.set_option(key, convert(given[key]))

    # ------------------------------------------------------------------ lifecycle
    def close(self):
        if getattr(self, '_h', None) is not None and self._h.value:
            self._lib.jcm_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ------------------------------------------------------------------ parameters
    def set_tensor(self, name, value):
        """`name` is the reference's TF variable name; `value` numpy or torch (host or device)."""
        if isinstance(value, torch.Tensor):
            t = value.detach().to(torch.float32).contiguous()
            ptr, shape, keep = t.data_ptr(), tuple(t.shape), t
        else:
            a = np.ascontiguousarray(value, dtype=np.float32)
            ptr, shape, keep = a.ctypes.data, a.shape, a
        if len(shape) == 0:
            raise ValueError('scalar parameter %r' % name)
        arr = (ctypes.c_int64 * len(shape))(*shape)
        _lib.check(self._lib.jcm_set_tensor(self._h, name.encode(), ctypes.c_void_p(ptr), arr, len(shape)),
                   'jcm_set_tensor(%s)' % name)
        self._shapes[name] = tuple(int(d) for d in shape)
        del keep

    def load_params(self, params, finalize=True):
        for name, value in params.items():
            self.set_tensor(name, value)
        if finalize:
            self.finalize()
        return self

    def update_tensor(self, name, value, refresh=True):
        """Overwrite a stored parameter after finalize (Saver.restore on a live session, main.py:612); refresh rebuilds
        the derived tables (pass False on all but the last tensor of a batch of updates)."""
        a = np.ascontiguousarray(value, dtype=np.float32)
        _lib.check(self._lib.jcm_update_tensor(self._h, name.encode(), ctypes.c_void_p(a.ctypes.data), a.size, int(bool(refresh))),
                   'jcm_update_tensor(%s)' % name)

    def finalize(self):
        _lib.check(self._lib.jcm_finalize(self._h), 'jcm_finalize')
        self._finalized = True

    # ------------------------------------------------------------------ helpers
    def _chk(self, t, ndim, name, dtype=torch.float32):
        if not isinstance(t, torch.Tensor):
            raise TypeError('%s must be a torch tensor' % name)
        if t.device != self.device:
            raise ValueError('%s is on %s, engine is on %s' % (name, t.device, self.device))
        if t.dtype != dtype:
            raise TypeError('%s must be %s, got %s' % (name, dtype, t.dtype))
        if t.dim() != ndim:
            raise ValueError('%s must have %d dims (NHWC), got shape %s' % (name, ndim, tuple(t.shape)))
        if not t.is_contiguous():
            raise ValueError('%s must be contiguous (NHWC)' % name)
        return t

    def _chk_img(self, t, name):
        """An image tensor [.,H,W,3]: float32, or uint8 (byte k is float32(k) / float32(255)) -> True for bytes.  Every other
        dtype is refused as _chk refuses it."""
        u8 = isinstance(t, torch.Tensor) and t.dtype == torch.uint8
        self._chk(t, 4, name, torch.uint8 if u8 else torch.float32)
        return u8

    def _new(self, *shape, dtype=torch.float32):
        return torch.empty(shape, dtype=dtype, device=self.device)

    @staticmethod
    def _p(t):
        return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)

    # ------------------------------------------------------------------ ops (main.py names)
    def conv_layer(self, x, name, stride, last_layer=False, n_out=None):
        """main.py:156-169."""
        self._chk(x, 4, 'x')
        B, H, W, _ = x.shape
        if n_out is None:
            raise ValueError('n_out is required to size the output')
        out = self._new(B, -(-H // stride), -(-W // stride), n_out)
        _lib.check(self._lib.jcm_conv_layer(self._h, name.encode(), stride, int(bool(last_layer)), self._p(x), B, H, W,
                                            self._p(out)), 'jcm_conv_layer(%s)' % name)
        return out

    def conv_layer_pre(self, x, name, stride, n_out):
        """pre_activ of main.py:160: conv_SAME(x, w) + b of ANY stored layer, BatchNorm or not (fp32 engines only) -> [B,ceil(H/s),ceil(W/s),n_out]."""
        self._chk(x, 4, 'x')
        B, H, W, _ = x.shape
        if stride not in (1, 2):
            raise ValueError('stride must be 1 or 2, got %r' % (stride,))
        out = self._new(B, -(-H // stride), -(-W // stride), int(n_out))
        self._on_stream(x, out)
        _lib.check(self._lib.jcm_conv_layer_pre(self._h, name.encode(), stride, self._p(x), B, H, W, self._p(out)), 'jcm_conv_layer_pre(%s)' % name)
        return out

    def conv_layer_merged(self, x1, x2, x3, name, n_out):
        """conv_layer(((x1 + up(x2)) + up(x3)) / 3) (main.py:58,67,69-71), the merge formed as the tower forms it (inside the layer's forward row
        pass on the frequency-domain route)."""
        for t, nm in ((x1, 'x1'), (x2, 'x2'), (x3, 'x3')):
            self._chk(t, 4, nm)
        B, H, W, C = x1.shape
        if x2.shape[0] != B or x3.shape[0] != B or x2.shape[3] != C or x3.shape[3] != C:
            raise ValueError('x1, x2, x3 must share batch and channel counts')
        out = self._new(B, H, W, n_out)
        _lib.check(self._lib.jcm_conv_layer_merged(self._h, name.encode(), self._p(x1), self._p(x2), x2.shape[1], x2.shape[2], self._p(x3), x3.shape[1], x3.shape[2],
                                                   B, H, W, self._p(out)), 'jcm_conv_layer_merged(%s)' % name)
        return out

    def upsample_merge3(self, x1, x2, x3, planar=False):
        """((x1 + up(x2)) + up(x3)) / 3 (main.py:58,67,69-70) by the merge kernel alone, as the tower launches it where conv5 does not form the merge
        itself.  float32 or bfloat16 tensors, all three of one dtype (the engine's precision plays no part): NHWC x1 [B,H,W,C], x2 [B,H2,W2,C],
        x3 [B,H3,W3,C] with C % 4 == 0, or with planar=True bfloat16 [B,C/8,H,W,8].  Returns x1's dtype, shape and layout."""
        ts = (x1, x2, x3)
        if not all(isinstance(t, torch.Tensor) for t in ts):
            raise TypeError('x1, x2, x3 must be torch tensors')
        if x1.dtype not in (torch.float32, torch.bfloat16) or x2.dtype != x1.dtype or x3.dtype != x1.dtype:
            raise TypeError('x1, x2, x3 must share one dtype, torch.float32 or torch.bfloat16; got %s, %s, %s' % (x1.dtype, x2.dtype, x3.dtype))
        if planar and x1.dtype != torch.bfloat16:
            raise TypeError('planar tensors are torch.bfloat16, got %s' % x1.dtype)
        for t, nm in zip(ts, ('x1', 'x2', 'x3')):
            self._chk(t, 5 if planar else 4, nm, x1.dtype)
        if planar:
            (B, C8, H, W, e), C = x1.shape, x1.shape[1] * 8
            same = e == 8 and all(t.shape[0] == B and t.shape[1] == C8 and t.shape[4] == 8 for t in ts)
            sizes = [(t.shape[2], t.shape[3]) for t in (x2, x3)]
        else:
            B, H, W, C = x1.shape
            same = C % 4 == 0 and all(t.shape[0] == B and t.shape[3] == C for t in ts)
            sizes = [(t.shape[1], t.shape[2]) for t in (x2, x3)]
        if not same or min(x1.shape) < 1 or min(min(s) for s in sizes) < 1:
            raise ValueError('x1, x2, x3 must be non-empty and share batch and channel counts (%s); got %s, %s, %s'
                             % ('[B,C/8,H,W,8]' if planar else '[B,H,W,C], C % 4 == 0', tuple(x1.shape), tuple(x2.shape), tuple(x3.shape)))
        out = torch.empty_like(x1)
        self._on_stream(x1, x2, x3, out)
        _lib.check(self._lib.jcm_upsample_merge3(self._h, self._p(x1), self._p(x2), sizes[0][0], sizes[0][1], self._p(x3), sizes[1][0], sizes[1][1],
                                                 B, H, W, C, int(x1.dtype == torch.bfloat16), int(bool(planar)), self._p(out)), 'jcm_upsample_merge3')
        return out

    def max_pool(self, x):
        """main.py:172-174."""
        self._chk(x, 4, 'x')
        B, H, W, C = x.shape
        out = self._new(B, (H + 1) // 2, (W + 1) // 2, C)
        _lib.check(self._lib.jcm_max_pool(self._h, self._p(x), B, H, W, C, self._p(out)), 'jcm_max_pool')
        return out

    def resize_bilinear(self, x, oh, ow):
        """tf.image.resize_images, TF-1.x legacy bilinear (main.py:51,58,60,67,89)."""
        self._chk(x, 4, 'x')
        B, H, W, C = x.shape
        out = self._new(B, oh, ow, C)
        _lib.check(self._lib.jcm_resize_bilinear(self._h, self._p(x), B, H, W, C, oh, ow, self._p(out)), 'jcm_resize_bilinear')
        return out

    def conv1_pool(self, x, scope, sub=1):
        """pool1(conv1_<res>(x[:, ::sub, ::sub])) (main.py:44-45,52-53,61-62) by the dispatch the tower uses: x [B,H,W,3] float32 or uint8, sub in
        {1, 2, 4} dividing H and W -> the pooled map, float32 (bfloat16 on a bf16 engine)."""
        u8 = self._chk_img(x, 'x')
        B, H, W, C = x.shape
        if C != 3:
            raise ValueError('x must be [B,H,W,3], got %s' % (tuple(x.shape),))
        if sub not in (1, 2, 4) or H % sub or W % sub:
            raise ValueError('sub must be 1, 2 or 4 and divide H and W, got sub = %r for %d x %d' % (sub, H, W))
        n_out = self._shapes[scope + '/weights'][3]
        out = self._new(B, (H // sub + 3) // 4, (W // sub + 3) // 4, n_out, dtype=torch.bfloat16 if self.precision == 'bf16' else torch.float32)      # ceil(ceil(n/2)/2) = ceil(n/4)
        self._on_stream(x, out)
        _lib.check(self._lib.jcm_conv1_pool(self._h, scope.encode(), self._p(x), int(u8), B, H, W, int(sub), self._p(out)), 'jcm_conv1_pool(%s)' % scope)
        return out

    def conv2_pool(self, p1, scope):
        """pool2(conv2_<res>(p1)) (main.py:46-47,54-55,63-64) of a bf16 engine as the tower runs it: p1 [B,H,W,Cin] bfloat16 -> [B,ceil(H/2),ceil(W/2),Cout]
        bfloat16.  An fp32 engine raises RuntimeError: its tower never materialises the pooled map."""
        self._chk(p1, 4, 'p1', torch.bfloat16)
        B, H, W, _ = p1.shape
        n_out = self._shapes[scope + '/weights'][3]
        out = self._new(B, (H + 1) // 2, (W + 1) // 2, n_out, dtype=torch.bfloat16)
        self._on_stream(p1, out)
        _lib.check(self._lib.jcm_conv2_pool(self._h, scope.encode(), self._p(p1), B, H, W, self._p(out)), 'jcm_conv2_pool(%s)' % scope)
        return out

    def model(self, x):
        """main.py:29-74: [B,H,W,3] (float32 or uint8) -> logits [B,H/8,W/8,K]."""
        u8 = self._chk_img(x, 'x')
        B, H, W, C = x.shape
        if C != 3:
            raise ValueError('x must be [B,H,W,3], got %s' % (tuple(x.shape),))
        out = self._new(B, _hm_size(H), _hm_size(W), self.n_joints)
        if u8:
            _lib.check(self._lib.jcm_pd_forward_u8(self._h, self._p(x), B, H, W, self._p(out)), 'jcm_pd_forward_u8')
        else:
            _lib.check(self._lib.jcm_pd_forward(self._h, self._p(x), B, H, W, self._p(out)), 'jcm_pd_forward')
        return out

    def spatial_softmax(self, hm):
        """main.py:212-217."""
        self._chk(hm, 4, 'hm')
        B, H, W, K = hm.shape
        out = torch.empty_like(hm)
        _lib.check(self._lib.jcm_spatial_softmax(self._h, self._p(hm), B, H * W, K, self._p(out)), 'jcm_spatial_softmax')
        return out

    def conv_mrf(self, A, Bm):
        """main.py:77-91: A [1,120,180,1], B [b,60,90,1] -> [b,60,90,1]."""
        self._chk(A, 4, 'A')
        self._chk(Bm, 4, 'B')
        if tuple(A.shape) != (1, 120, 180, 1) or tuple(Bm.shape[1:]) != (60, 90, 1):
            raise ValueError('conv_mrf expects A [1,120,180,1] and B [b,60,90,1]; got %s, %s' % (tuple(A.shape), tuple(Bm.shape)))
        out = torch.empty_like(Bm)
        _lib.check(self._lib.jcm_conv_mrf(self._h, self._p(A), self._p(Bm), Bm.shape[0], self._p(out)), 'jcm_conv_mrf')
        return out

    def spatial_model(self, heat_map):
        """main.py:94-125: [B,60,90,K+1] -> [B,60,90,K]."""
        self._chk(heat_map, 4, 'heat_map')
        B = heat_map.shape[0]
        if tuple(heat_map.shape[1:]) != (60, 90, self.n_joints + 1):
            raise ValueError('spatial_model expects [B,60,90,%d], got %s' % (self.n_joints + 1, tuple(heat_map.shape)))
        out = self._new(B, 60, 90, self.n_joints)
        _lib.check(self._lib.jcm_sm_forward(self._h, self._p(heat_map), B, self._p(out)), 'jcm_sm_forward')
        return out

    def argmax_coords(self, hm):
        """evaluation.py:15-24: [B,H,W,K] -> int32 [B,2,K] (row, col)."""
        self._chk(hm, 4, 'hm')
        B, H, W, K = hm.shape
        out = self._new(B, 2, K, dtype=torch.int32)
        _lib.check(self._lib.jcm_argmax_coords(self._h, self._p(hm), B, H, W, K, self._p(out)), 'jcm_argmax_coords')
        return out

    def det_curve(self, pred_coords, y, radii, hits=None, want_dist=False, want_true=False):
        """evaluation.py:15-36 for every joint and every radius in one launch and one pass over the targets.
        pred_coords int32 [B,2,K] (row, col); y [B,H,W,C] with C >= K: the targets y_in, channels >= K ignored; radii: up to 32 numbers
        (host).  hits: int32 [K,R] device tensor that is ADDED to (zeros when not given): hits[k,r] += #images whose joint k lies within
        radii[r] % of the torso length.  Returns {'hits'} plus 'norm_dist' fp32 [B,K] (want_dist) and 'true_coords' int32 [B,2,K]
        (want_true).  Nothing is read back.  K, C and the number of radii are checked by the library."""
        self._chk(pred_coords, 3, 'pred_coords', torch.int32)
        self._chk(y, 4, 'y')
        B, H, W, C = y.shape
        K = pred_coords.shape[2]
        if tuple(pred_coords.shape) != (B, 2, K):
            raise ValueError('pred_coords must be [B,2,K] with the batch size of y; got %s, y %s' % (tuple(pred_coords.shape), tuple(y.shape)))
        rad = np.ascontiguousarray(np.asarray(radii if isinstance(radii, np.ndarray) else list(radii), dtype=np.float32).reshape(-1))
        R = int(rad.size)
        if hits is not None:
            self._chk(hits, 2, 'hits', torch.int32)
            if tuple(hits.shape) != (K, R):
                raise ValueError('hits must be [K,R] = [%d,%d], got %s' % (K, R, tuple(hits.shape)))
        out = {'hits': hits if hits is not None else torch.zeros((K, R), dtype=torch.int32, device=self.device)}
        if want_dist:
            out['norm_dist'] = self._new(B, K)
        if want_true:
            out['true_coords'] = self._new(B, 2, K, dtype=torch.int32)
        self._on_stream(pred_coords, y, *out.values())      # the zeros and the caller's tensors were made on torch's current stream
        _lib.check(self._lib.jcm_det_curve(self._h, self._p(pred_coords), self._p(y), B, H, W, K, C, rad.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), R,
                                           self._p(out.get('true_coords')), self._p(out.get('norm_dist')), self._p(out['hits'])), 'jcm_det_curve')
        return out

    def hm_peaks(self, hm, max_peaks=4, threshold=0.0):
        """The top max_peaks local maxima of every map of hm [B,H,W,K] (probabilities or logits) in one launch: a pixel above
        `threshold` that no 8-neighbour exceeds (the first pixel of a plateau), ranked by value, then by index.  Returns {'cells' int32
        [B,K,P,2] (row, col), 'offsets' fp32 [B,K,P,2] (+-0.25 of a cell towards the higher neighbour, 0 on the border and between equal
        neighbours), 'scores' fp32 [B,K,P] (the map's value), 'count' int32 [B,K]}, device tensors; slots from count on hold -1 / 0 / 0.
        Peak 0 is argmax_coords wherever count > 0.  Nothing is read back.  max_peaks (1..8) and the map size (H * W <= 21600) are checked by
        the library."""
        self._chk(hm, 4, 'hm')
        B, H, W, K = hm.shape
        P = int(max_peaks)
        n = max(P, 0)
        out = {'cells': self._new(B, K, n, 2, dtype=torch.int32), 'offsets': self._new(B, K, n, 2), 'scores': self._new(B, K, n),
               'count': self._new(B, K, dtype=torch.int32)}
        self._on_stream(hm, *out.values())
        _lib.check(self._lib.jcm_hm_peaks(self._h, self._p(hm), B, H, W, K, P, float(threshold), self._p(out['cells']), self._p(out['offsets']),
                                          self._p(out['scores']), self._p(out['count'])), 'jcm_hm_peaks')
        return out

    def _add_peaks_pose(self, r, scratch, peaks, decode, torso):
        """The tail of the forward family.  peaks = P: hm_peaks of the call's probabilities, which are in r (want_prob) or in scratch; decode:
        pose_decode of the call's pd_peaks on its part-detector probabilities and torso map.  Returns r."""
        for key in ('pd', 'sm') if peaks else ():
            prob = r.get(key + '_prob', scratch.get(key + '_prob'))
            if prob is not None:
                r[key + '_peaks'] = self.hm_peaks(prob, max_peaks=peaks)
        if decode:
            with torch.cuda.stream(self._stream):      # the probabilities were written on the engine's stream
                hm10 = torch.cat([r.get('pd_prob', scratch.get('pd_prob')), torso], dim=3)
            r['pose'] = self.pose_decode(hm10, r['pd_peaks'])
        return r

    def pose_decode(self, hm10, peaks, want_tables=False):
        """Of the candidate cells per joint in `peaks` (the dict of hm_peaks on nine joint maps, P <= 4: 'cells' int32 [B,9,P,2], 'count' int32
        [B,9]) the ONE combination with the highest spatial-model energy on hm10 [B,60,90,10] (what spatial_model takes: nine part-detector
        probabilities and the torso map) -- a joint MAP over P^9 poses (include/jcm.h: jcm_pose_decode).  Returns {'index' int32
        [B,9] (the chosen peak per joint), 'coords' int32 [B,2,9] (its cell, the layout of argmax_coords), 'score' fp32 [B], 'score0' fp32 [B]
        (the all-peak-0 pose: the independent arg-maxes)} plus, with want_tables, 'V' fp32 [B,9,P] and 'M' fp32 [B,36,P,P].  An image with an
        empty candidate list has no pose: -1 / -1 / -inf / -inf.  Device tensors; nothing is read back.  P is checked by the library."""
        self._chk(hm10, 4, 'hm10')
        cells, count = peaks['cells'], peaks['count']
        self._chk(cells, 4, "peaks['cells']", torch.int32)
        self._chk(count, 2, "peaks['count']", torch.int32)
        B, P = hm10.shape[0], cells.shape[2]
        if tuple(hm10.shape[1:]) != (60, 90, 10) or tuple(cells.shape) != (B, 9, P, 2) or tuple(count.shape) != (B, 9):
            raise ValueError("pose_decode expects hm10 [B,60,90,10], peaks['cells'] [B,9,P,2] and peaks['count'] [B,9]; got %s, %s, %s"
                             % (tuple(hm10.shape), tuple(cells.shape), tuple(count.shape)))
        out = {'index': self._new(B, 9, dtype=torch.int32), 'coords': self._new(B, 2, 9, dtype=torch.int32), 'score': self._new(B), 'score0': self._new(B)}
        if want_tables:
            out['V'] = self._new(B, 9, P)
            out['M'] = self._new(B, 36, P, P)
        self._on_stream(hm10, cells, count, *out.values())
        _lib.check(self._lib.jcm_pose_decode(self._h, self._p(hm10), B, self._p(cells), self._p(count), P, self._p(out['index']), self._p(out['coords']),
                                             self._p(out['score']), self._p(out['score0']), self._p(out.get('V')), self._p(out.get('M'))), 'jcm_pose_decode')
        return out

    def seq_pose_viterbi(self, V, M, count, cells, tau):
        """The clip decode (include/jcm.h: jcm_seq_pose_viterbi): the most probable sequence of POSES through a clip -- per frame the
        P^9 poses of pose_decode with their scores, linked in time by tau, one P x P table of log-scores per joint and frame.  V fp32 [T,9,P] or
        [S,T,9,P] and M fp32 [.,36,P,P] as pose_decode(want_tables=True) returns them for the clip's frames, count int32 [.,9] and cells int32
        [.,9,P,2] as hm_peaks does, tau float64 [.,9,P,P] (motion.seq_pose_tau; host or device): tau[t,j,a,b] scores joint j going from
        candidate a of frame t-1 to candidate b of frame t.  Returns {'index' int32 [S,T,9], 'coords' int32 [S,T,2,9], 'frame_score' fp32 [S,T],
        'maxes' float64 [S,T], 'breaks' int32 [S,T]}, device tensors without the S axis for tables without one; nothing is read back.  Shapes
        and dtypes that do not fit raise ValueError before any launch; the plane and the back-pointers (3 P^9 bytes per frame) live in the
        engine's workspace, and a clip they do not fit in is a RuntimeError that names the bytes.  There is no online form."""
        if not isinstance(V, torch.Tensor) or V.dim() not in (3, 4):
            raise ValueError('V must be a device tensor [T,9,P] or [S,T,9,P]')
        single = V.dim() == 3
        if not isinstance(tau, torch.Tensor):
            tau = torch.from_numpy(np.ascontiguousarray(np.asarray(tau, np.float64))).to(self.device)
        lift = lambda t: t.unsqueeze(0) if single and isinstance(t, torch.Tensor) else t
        try:
            V, M, count, cells, tau = (self._chk(lift(t), n, name, dt) for t, n, name, dt in (
                (V, 4, 'V', torch.float32), (M, 5, 'M', torch.float32), (count, 3, 'count', torch.int32), (cells, 5, 'cells', torch.int32),
                (tau, 5, 'tau', torch.float64)))
        except TypeError as e:
            raise ValueError(str(e))
        S, T, K, P = V.shape
        if (K != 9 or not 1 <= P <= 4 or S < 1 or T < 1 or tuple(M.shape) != (S, T, 36, P, P) or tuple(count.shape) != (S, T, 9)
                or tuple(cells.shape) != (S, T, 9, P, 2) or tuple(tau.shape) != (S, T, 9, P, P)):
            raise ValueError('seq_pose_viterbi expects V [S,T,9,P] with 1 <= P <= 4, M [S,T,36,P,P], count [S,T,9], cells [S,T,9,P,2] and tau [S,T,9,P,P]; '
                             'got %s, %s, %s, %s, %s' % tuple(tuple(t.shape) for t in (V, M, count, cells, tau)))
        out = {'index': self._new(S, T, 9, dtype=torch.int32), 'coords': self._new(S, T, 2, 9, dtype=torch.int32), 'frame_score': self._new(S, T),
               'maxes': self._new(S, T, dtype=torch.float64), 'breaks': self._new(S, T, dtype=torch.int32)}
        self._on_stream(V, M, count, cells, tau, *out.values())
        _lib.check(self._lib.jcm_seq_pose_viterbi(self._h, self._p(V), self._p(M), self._p(count), self._p(cells), self._p(tau), S, T, P, self._p(out['index']),
                                                  self._p(out['coords']), self._p(out['frame_score']), self._p(out['maxes']), self._p(out['breaks'])),
                   'jcm_seq_pose_viterbi')
        return {k: v[0] for k, v in out.items()} if single else out

    def _seq_args(self, hm, sigma, radius):
        """hm [T,HH,WW,K] or [S,T,HH,WW,K] -> (hm as [S,T,HH,WW,K], whether a sequence axis was added, host taps [K,2R+1], R)."""
        if not isinstance(hm, torch.Tensor) or hm.dim() not in (4, 5):
            raise ValueError('hm must be a device tensor [T,HH,WW,K] or [S,T,HH,WW,K]')
        single = hm.dim() == 4
        hm5 = self._chk(hm.unsqueeze(0) if single else hm, 5, 'hm')
        R, taps = motion.seq_kernel(sigma, radius, hm5.shape[4])
        return hm5, single, taps, R

    def _seq_shift(self, shift, S, T, single):
        """shift: int32 [T,2] (a 4-d hm) or [S,T,2] = (sy, sx), host or device -> a contiguous device int32 [S,T,2]."""
        if not isinstance(shift, torch.Tensor):
            a = np.asarray(shift)
            if a.dtype.kind not in 'iu' or a.size and (a.min() < -2 ** 31 or a.max() >= 2 ** 31):
                raise ValueError('shift must hold int32 values, got %s' % (a.dtype,))
            shift = torch.from_numpy(np.ascontiguousarray(a.astype(np.int32)))
        if shift.dtype != torch.int32:
            raise ValueError('shift must be int32, got %s' % (shift.dtype,))
        if single and shift.dim() == 2:
            shift = shift.unsqueeze(0)
        if tuple(shift.shape) != (S, T, 2):
            raise ValueError('shift must be [S,T,2] = %s (or [T,2] with a 4-d hm), got %s' % ((S, T, 2), tuple(shift.shape)))
        return shift.to(self.device).contiguous()

    def _seq_centre(self, centre, shift, S, T, HH, WW, single):
        """centre: int32 [T,HH,WW,2] (a 4-d hm) or [S,T,HH,WW,2] = (sy, sx) per cell, host or device -> a contiguous device int32 [S,T,HH,WW,2]."""
        if shift is not None:
            raise ValueError('centre and shift are two forms of one thing: a shift per cell or one per frame; give one of them')
        if not isinstance(centre, torch.Tensor):
            a = np.asarray(centre)
            if a.dtype.kind not in 'iu' or a.size and (a.min() < -2 ** 31 or a.max() >= 2 ** 31):
                raise ValueError('centre must hold int32 values, got %s' % (a.dtype,))
            centre = torch.from_numpy(np.ascontiguousarray(a.astype(np.int32)))
        if centre.dtype != torch.int32:
            raise ValueError('centre must be int32, got %s' % (centre.dtype,))
        if single and centre.dim() == 4:
            centre = centre.unsqueeze(0)
        if tuple(centre.shape) != (S, T, HH, WW, 2):
            raise ValueError('centre must be [S,T,HH,WW,2] = %s (or [T,HH,WW,2] with a 4-d hm), got %s' % ((S, T, HH, WW, 2), tuple(centre.shape)))
        return centre.to(self.device).contiguous()

    def seq_filter(self, hm, sigma, rho, radius=None, state=None, shift=None, centre=None):
        """The causal forward filter of a clip's heat maps (include/jcm.h: jcm_seq_filter): hm [T,HH,WW,K] or [S,T,HH,WW,K],
        frame after frame of what forward returns as pd_prob / sm_prob; sigma: a scalar or K values, the motion per frame in heat-map cells
        (motion.seq_taps builds the taps); rho in [0,1]: the mass of the uniform "anywhere" term; radius: default min(16, ceil(3 max sigma));
        state: float64 [S,K,HH,WW] ([K,HH,WW] for a 4-d hm), the 'state' of the call that ended just before frame 0, or None at a clip's start.
        Returns {'filtered' fp32 like hm, 'coords' int32 [S,T,2,K] (row, col), 'norm' float64 [S,T,K], 'reset' int32 [S,T,K], 'state' float64
        [S,K,HH,WW]}, device tensors without the S axis for a 4-d hm; nothing is read back.  HH * WW <= 8192 and K <= 16 are checked by the
        library.
        shift: None, or int32 [T,2] / [S,T,2] = (sy, sx) on the host or the device, for maps whose lattice moves (include/jcm.h:
        jcm_seq_filter_moving): cell (y, x) of frame t is cell (y + sy, x + sx) of frame t-1; shift[0] applies to the transition from `state`
        and is ignored without one.  'coords' are in every frame's own lattice, 'state' in the last frame's.
        centre: None, or int32 [T,HH,WW,2] / [S,T,HH,WW,2] = (sy, sx) on the host or the device: the same shift per DESTINATION cell (DESIGN.md 4.29,
        include/jcm.h: jcm_seq_filter_centred) -- cell (y, x) of frame t was cell (y + sy, x + sx) of frame t-1, one table for all joints
        (motion.flow_cell_shifts makes one of Engine.frame_flow's output); centre[0] applies to the transition from `state` and is ignored without
        one.  A table that is uniform over every frame gives the bits of shift=, an all-zero table those of a call without either.  centre with shift is a ValueError."""
        hm5, single, taps, R = self._seq_args(hm, sigma, radius)
        S, T, HH, WW, K = hm5.shape
        if centre is not None:
            centre = self._seq_centre(centre, shift, S, T, HH, WW, single)
        elif shift is not None:
            shift = self._seq_shift(shift, S, T, single)
        if state is not None:
            state = self._chk(state.unsqueeze(0) if single and isinstance(state, torch.Tensor) and state.dim() == 3 else state, 4, 'state', torch.float64)
            if tuple(state.shape) != (S, K, HH, WW):
                raise ValueError('state must be [S,K,HH,WW] = %s, got %s' % ((S, K, HH, WW), tuple(state.shape)))
        out = {'filtered': self._new(S, T, HH, WW, K), 'coords': self._new(S, T, 2, K, dtype=torch.int32), 'norm': self._new(S, T, K, dtype=torch.float64),
               'reset': self._new(S, T, K, dtype=torch.int32), 'state': self._new(S, K, HH, WW, dtype=torch.float64)}
        self._on_stream(hm5, *(t for t in (state, shift, centre) if t is not None), *out.values())
        tp = taps.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
        tail = (self._p(state), self._p(out['filtered']), self._p(out['coords']), self._p(out['norm']), self._p(out['reset']), self._p(out['state']))
        if centre is not None:
            _lib.check(self._lib.jcm_seq_filter_centred(self._h, self._p(hm5), S, T, HH, WW, K, tp, R, float(rho), self._p(centre), *tail), 'jcm_seq_filter_centred')
        elif shift is not None:
            _lib.check(self._lib.jcm_seq_filter_moving(self._h, self._p(hm5), S, T, HH, WW, K, tp, R, float(rho), self._p(shift), *tail), 'jcm_seq_filter_moving')
        else:
            _lib.check(self._lib.jcm_seq_filter(self._h, self._p(hm5), S, T, HH, WW, K, tp, R, float(rho), *tail), 'jcm_seq_filter')
        return {k: v[0] for k, v in out.items()} if single else out

    def seq_viterbi(self, hm, sigma, rho, radius=None, shift=None, centre=None):
        """The most probable track through a clip's heat maps (include/jcm.h: jcm_seq_viterbi); hm, sigma, rho and radius as for
        seq_filter.  Returns {'path' int32 [S,T,2,K] (row, col), 'maxes' float64 [S,T,K], 'breaks' int32 [S,T,K]}, device tensors without the S
        axis for a 4-d hm; nothing is read back.  The back-pointers (2 bytes per cell, frame, joint and sequence) live in the engine's
        workspace; a clip they do not fit in is a RuntimeError that names the bytes.
        shift: as for seq_filter (include/jcm.h: jcm_seq_viterbi_moving); 'path' is in every frame's own lattice, shift[0] is ignored.
        centre: as for seq_filter (include/jcm.h: jcm_seq_viterbi_centred); centre[0] is never read.  centre with shift is a ValueError."""
        hm5, single, taps, R = self._seq_args(hm, sigma, radius)
        S, T, HH, WW, K = hm5.shape
        if centre is not None:
            centre = self._seq_centre(centre, shift, S, T, HH, WW, single)
        elif shift is not None:
            shift = self._seq_shift(shift, S, T, single)
        out = {'path': self._new(S, T, 2, K, dtype=torch.int32), 'maxes': self._new(S, T, K, dtype=torch.float64), 'breaks': self._new(S, T, K, dtype=torch.int32)}
        self._on_stream(hm5, *(t for t in (shift, centre) if t is not None), *out.values())
        tp = taps.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
        tail = (self._p(out['path']), self._p(out['maxes']), self._p(out['breaks']))
        if centre is not None:
            _lib.check(self._lib.jcm_seq_viterbi_centred(self._h, self._p(hm5), S, T, HH, WW, K, tp, R, float(rho), self._p(centre), *tail), 'jcm_seq_viterbi_centred')
        elif shift is not None:
            _lib.check(self._lib.jcm_seq_viterbi_moving(self._h, self._p(hm5), S, T, HH, WW, K, tp, R, float(rho), self._p(shift), *tail), 'jcm_seq_viterbi_moving')
        else:
            _lib.check(self._lib.jcm_seq_viterbi(self._h, self._p(hm5), S, T, HH, WW, K, tp, R, float(rho), *tail), 'jcm_seq_viterbi')
        return {k: v[0] for k, v in out.items()} if single else out

    def frame_shift(self, x, rect, search=motion.SEQ_CAMERA_SEARCH, prev=None):
        """The camera's whole-pixel translation between consecutive fitted frames (include/jcm.h: jcm_frame_shift): x uint8
        [T,H,W,3] on the device, the letterboxed frames of a clip; rect = (y0, x0, ch, cw), the content rectangle of their fit (the first four of
        fit_images' geom) -- nothing outside it is read; search: the coarse radius D in 1..16, reaching +-(4 D + 3) pixels a frame; prev: uint8
        [H,W,3], the frame before frame 0, or None at a clip's start.  Returns {'disp' int32 [T,2] = (dy, dx): the content at pixel (y, x) of
        frame t is at (y + dy, x + dx) of frame t-1, 'sad' int64 [T,2] = (the sum of absolute luma differences at disp, the same at (0, 0))},
        device tensors; row 0 is zero without prev.  Integer arithmetic throughout; nothing is read back.  motion.camera_shifts turns 'disp' into
        the shift of seq_filter / seq_viterbi.  Sizes, the rectangle and search are checked by the library."""
        self._chk(x, 4, 'x', torch.uint8)
        T, H, W, C = x.shape
        if C != 3:
            raise ValueError('x must be [T,H,W,3], got shape %s' % (tuple(x.shape),))
        if prev is not None:
            self._chk(prev, 3, 'prev', torch.uint8)
            if tuple(prev.shape) != (H, W, 3):
                raise ValueError('prev must be [H,W,3] = %s, got %s' % ((H, W, 3), tuple(prev.shape)))
        y0, x0, ch, cw = (int(v) for v in rect)
        out = {'disp': self._new(T, 2, dtype=torch.int32), 'sad': self._new(T, 2, dtype=torch.int64)}
        self._on_stream(x, *([prev] if prev is not None else []), *out.values())
        _lib.check(self._lib.jcm_frame_shift(self._h, self._p(x), T, H, W, y0, x0, ch, cw, int(search), self._p(prev), self._p(out['disp']),
                                             self._p(out['sad'])), 'jcm_frame_shift')
        return out

    def frame_flow(self, x, rect, ref, search=motion.SEQ_FLOW_SEARCH):
        """One whole-pixel displacement per heat-map cell between every frame and its reference frames (include/jcm.h:
        jcm_frame_flow): x uint8 [T,H,W,3] on the device, the letterboxed frames of a clip, H and W multiples of 8; rect = (y0, x0, ch, cw), the
        content rectangle of their fit -- nothing outside it is read; ref: int [T,R] on the host or the device, R in 1..8: slot r of frame t is
        matched against frame ref[t,r], a negative entry (or one >= T) is "no such frame" (motion.flow_refs builds the layout hm_flow_pool
        takes); search: the radius D in 1..16 pixels.  Returns {'flow' int32 [T,R,H/8,W/8,2] = (dy, dx): the content at pixel (y, x) of frame t is
        at (y + dy, x + dx) of the reference frame, 'sad' int32 [T,R,H/8,W/8,2] = (the sum of absolute luma differences over the cell's block
        at flow, the same at (0, 0))}, device tensors, zero where there is no frame or no pixel.  Integer arithmetic throughout; nothing is
        read back.  Sizes, the rectangle and search are checked by the library."""
        self._chk(x, 4, 'x', torch.uint8)
        T, H, W, C = x.shape
        if C != 3:
            raise ValueError('x must be [T,H,W,3], got shape %s' % (tuple(x.shape),))
        if not isinstance(ref, torch.Tensor):
            a = np.asarray(ref)
            if a.dtype.kind not in 'iu' or a.size and (a.min() < -2 ** 31 or a.max() >= 2 ** 31):
                raise ValueError('ref must hold int32 values, got %s' % (a.dtype,))
            ref = torch.from_numpy(np.ascontiguousarray(a.astype(np.int32)))
        if ref.dtype != torch.int32:
            raise ValueError('ref must be int32, got %s' % (ref.dtype,))
        if ref.dim() != 2 or ref.shape[0] != T:
            raise ValueError('ref must be [T,R] = [%d,R], got %s' % (T, tuple(ref.shape)))
        ref = ref.to(self.device).contiguous()
        R = int(ref.shape[1])
        y0, x0, ch, cw = (int(v) for v in rect)
        out = {'flow': self._new(T, R, H // 8, W // 8, 2, dtype=torch.int32), 'sad': self._new(T, R, H // 8, W // 8, 2, dtype=torch.int32)}
        self._on_stream(x, ref, *out.values())
        _lib.check(self._lib.jcm_frame_flow(self._h, self._p(x), T, H, W, y0, x0, ch, cw, int(search), self._p(ref), R, self._p(out['flow']),
                                            self._p(out['sad'])), 'jcm_frame_flow')
        return out

    def hm_flow_pool(self, hm, flow, weights):
        """The neighbouring frames' heat maps warped onto every frame by its cells' own displacement and pooled with the frame's map (DESIGN.md
        4.28, include/jcm.h: jcm_hm_flow_pool): hm fp32 [T,HH,WW,K]; flow int32 [T,2N,HH,WW,2], what frame_flow returns for motion.flow_refs(T, N);
        weights: N + 1 host values, w[0] > 0 for the frame itself and w[n] >= 0 for the frames n before and after (motion.flow_weights).  Returns
        fp32 like hm: the weighted mean, in float64 and one fixed order, of the frame's value and the bilinear samples of the neighbours that
        exist.  A device tensor; nothing is read back.  N in 1..4, K <= 16 and HH * WW <= 8192 are checked by the library."""
        self._chk(hm, 4, 'hm')
        self._chk(flow, 5, 'flow', torch.int32)
        T, HH, WW, K = hm.shape
        w = np.ascontiguousarray(np.asarray(weights, np.float64).reshape(-1))
        N = int(w.size) - 1
        if tuple(flow.shape) != (T, 2 * N, HH, WW, 2):
            raise ValueError('flow must be [T,2N,HH,WW,2] = %s for %d weights, got %s' % ((T, 2 * N, HH, WW, 2), w.size, tuple(flow.shape)))
        out = self._new(T, HH, WW, K)
        self._on_stream(hm, flow, out)
        _lib.check(self._lib.jcm_hm_flow_pool(self._h, self._p(hm), T, HH, WW, K, self._p(flow), N, w.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
                                              self._p(out)), 'jcm_hm_flow_pool')
        return out

    def seq_smooth(self, hm, sigma, rho, radius=None, want_smoothed=True):
        """The smoothed marginals P(x_t | all frames) of a clip's heat maps and the expected transition statistics of the backward pass (DESIGN.md
        4.23, include/jcm.h: jcm_seq_smooth); hm, sigma, rho and radius as for seq_filter, offline (no state).  Returns {'smoothed' fp32 like hm
        (left out with want_smoothed=False), 'coords' int32 [S,T,2,K] (row, col), 'conf' fp32 [S,T,K] (the marginal at that cell), 'norm' float64
        [S,T,K] and 'reset' int32 [S,T,K] (the filter's), 'mass' float64 [S,T,K], 'cut' int32 [S,T,K], 'trans' float64 [S,T,K,3] (moved, jumped,
        squared displacement; row 0 is zero)}, device tensors without the S axis for a 4-d hm; nothing is read back.  HH * WW <= 6144 here; the
        float64 beliefs of all frames live in the engine's workspace, and a clip they do not fit in is a RuntimeError that names the bytes."""
        hm5, single, taps, R = self._seq_args(hm, sigma, radius)
        S, T, HH, WW, K = hm5.shape
        out = {'coords': self._new(S, T, 2, K, dtype=torch.int32), 'conf': self._new(S, T, K), 'norm': self._new(S, T, K, dtype=torch.float64),
               'reset': self._new(S, T, K, dtype=torch.int32), 'mass': self._new(S, T, K, dtype=torch.float64), 'cut': self._new(S, T, K, dtype=torch.int32),
               'trans': self._new(S, T, K, 3, dtype=torch.float64)}
        if want_smoothed:
            out['smoothed'] = self._new(S, T, HH, WW, K)
        self._on_stream(hm5, *out.values())
        _lib.check(self._lib.jcm_seq_smooth(self._h, self._p(hm5), S, T, HH, WW, K, taps.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), R, float(rho),
                                            self._p(out.get('smoothed')), self._p(out['coords']), self._p(out['conf']), self._p(out['norm']),
                                            self._p(out['reset']), self._p(out['mass']), self._p(out['cut']), self._p(out['trans'])), 'jcm_seq_smooth')
        return {k: v[0] for k, v in out.items()} if single else out

    def seq_smooth_lag(self, hm, sigma, rho, lag, radius=None, state=None, flush=False, want_smoothed=False):
        """The fixed-lag smoother (include/jcm.h: jcm_seq_smooth_lag): frame s of a live clip as P(x_s | frames 0 .. s+lag),
        lag >= 1 frames late -- what seq_smooth writes for frame s given frames 0 .. s+lag, bit for bit, for any split of the clip into calls.
        hm [T,HH,WW,K] or [S,T,HH,WW,K]: the NEW frames only (T may be 0 with a state, to flush a clip); sigma, rho and radius as for seq_filter;
        state: the 'state' of the call that ended just before frame 0, or None at a clip's start; flush=True ends the clip: every pending frame
        is emitted with the future it has.  Returns the E emitted frames' {'coords' int32 [S,E,2,K], 'conf' fp32 [S,E,K], 'norm' float64
        [S,E,K], 'reset' int32 [S,E,K], 'mass' float64 [S,E,K], 'cut' int32 [S,E,K], 'smoothed' fp32 [S,E,HH,WW,K] with want_smoothed}, without
        the S axis for a 4-d hm, 'lag' int32 [E], the lag each emitted frame actually got (below `lag` only at a flushed clip's end), and
        'state': a dict of device tensors -- the pending frames' maps, float64 beliefs, norm and reset -- with the shape, lag and taps the next
        call checks; None after a flush.  E may be 0.  The window is assembled and cut with device copies; nothing is read back."""
        hm5, single, taps, R = self._seq_args(hm, sigma, radius)
        S, T, HH, WW, K = hm5.shape
        L, flush = int(lag), bool(flush)
        if L < 1:
            raise ValueError('lag must be >= 1, got %r (lag 0 is the causal filter: seq_filter)' % (lag,))
        sig = {'shape': (S, HH, WW, K), 'lag': L, 'taps': (R, float(rho), taps.tobytes())}
        P = 0
        if state is not None:
            if not isinstance(state, dict) or any(state.get(k) != v for k, v in sig.items()):
                raise ValueError("state is not the 'state' of a seq_smooth_lag call with these maps' shape %s, this lag and these taps" % (sig['shape'],))
            P = int(state['hm'].shape[1])
        W = P + T
        if W < 1:
            raise ValueError('seq_smooth_lag needs a frame: hm has none and there is no pending frame')
        E = W if flush else max(0, W - L)
        self._on_stream(hm5, *([state[k] for k in ('hm', 'belief', 'norm', 'reset')] if state is not None else []))
        with torch.cuda.stream(self._stream):
            win = {'hm': self._new(S, W, HH, WW, K), 'belief': self._new(S * K, W, HH * WW, dtype=torch.float64),
                   'norm': self._new(S, W, K, dtype=torch.float64), 'reset': self._new(S, W, K, dtype=torch.int32)}
            win['hm'][:, P:] = hm5
            for k in (win if state is not None else ()):
                win[k][:, :P] = state[k]
            out = {'coords': self._new(S, E, 2, K, dtype=torch.int32), 'conf': self._new(S, E, K), 'mass': self._new(S, E, K, dtype=torch.float64),
                   'cut': self._new(S, E, K, dtype=torch.int32)}
            if want_smoothed:
                out['smoothed'] = self._new(S, E, HH, WW, K)
            _lib.check(self._lib.jcm_seq_smooth_lag(self._h, self._p(win['hm']), S, W, P, HH, WW, K, taps.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), R,
                                                    float(rho), L, int(flush), self._p(win['belief']), self._p(win['norm']), self._p(win['reset']),
                                                    self._p(out.get('smoothed')), self._p(out['coords']), self._p(out['conf']), self._p(out['mass']),
                                                    self._p(out['cut'])), 'jcm_seq_smooth_lag')
            out['norm'], out['reset'] = win['norm'][:, :E].contiguous(), win['reset'][:, :E].contiguous()
            if single:
                out = {k: v[0] for k, v in out.items()}
            out['lag'] = torch.clamp(torch.arange(W - 1, W - 1 - E, -1, dtype=torch.int32, device=self.device), max=L)
            out['state'] = None if flush else dict(sig, **{k: v[:, E:].contiguous() for k, v in win.items()})
        return out

    def seq_fit(self, hm, sigma=None, rho=None, iters=10, radius=16, fit_rho=True):
        """motion.seq_fit on this engine: sigma per joint and rho re-estimated on the clip's own maps (EM, one seq_smooth per iteration)."""
        return motion.seq_fit(self, hm, motion.SEQ_SIGMA if sigma is None else sigma, motion.SEQ_RHO if rho is None else rho, iters=iters, radius=radius,
                              fit_rho=fit_rho)

    def seq_tracks(self, hm, people, sigma, rho, radius=None, exclude=SEQ_EXCLUDE, mode='viterbi', state=None, want_filtered=False):
        """Several consistent tracks through single-channel maps -- one torso per person of a clip (include/jcm.h:
        jcm_seq_tracks_viterbi / jcm_seq_tracks_filter).  hm [T,HH,WW] or [S,T,HH,WW], non-negative (spatial_softmax of the torso energy);
        people = M in 1..4; sigma (a scalar), rho and radius as for seq_filter (motion.seq_taps builds the one tap row); exclude = D in 0..64:
        pass n sees the map with the cells within D (Chebyshev) of every earlier track's cell zeroed, frame by frame, where that track has a
        positive value -- SEQ_EXCLUDE is an untuned placeholder.  Track 0 is seq_viterbi / seq_filter on the map, bit for bit.
        mode 'viterbi' returns {'path' int32 [S,M,T,2] (row, col), 'maxes' float64 [S,M,T], 'breaks' int32 [S,M,T], 'value' fp32 [S,M,T]};
        mode 'filter' takes state (float64 [S,M,HH*WW] or None at a clip's start) and returns {'coords', 'norm', 'reset', 'value' in the same
        shapes, 'state' float64 [S,M,HH*WW]} and, with want_filtered, 'filtered' fp32 [S,M,T,HH,WW], the beliefs.  Device tensors, without the S axis for a 3-d hm; nothing is read back.  M, D and the map size
        (HH * WW <= 8192) are checked by the library."""
        if mode not in ('filter', 'viterbi'):
            raise ValueError("mode must be 'filter' or 'viterbi', got %r" % (mode,))
        if state is not None and mode != 'filter':
            raise ValueError("state belongs to mode='filter'")
        if not isinstance(hm, torch.Tensor) or hm.dim() not in (3, 4):
            raise ValueError('hm must be a device tensor [T,HH,WW] or [S,T,HH,WW]')
        single = hm.dim() == 3
        hm4 = self._chk(hm.unsqueeze(0) if single else hm, 4, 'hm')
        S, T, HH, WW = hm4.shape
        M, D = int(people), int(exclude)
        R, tap_row = motion.seq_kernel(sigma, radius, 1)
        taps = tap_row.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
        n = max(M, 0)
        cells, v, f = motion.SEQ_KEYS[mode]
        out = {cells: self._new(S, n, T, 2, dtype=torch.int32), v: self._new(S, n, T, dtype=torch.float64), f: self._new(S, n, T, dtype=torch.int32),
               'value': self._new(S, n, T)}
        if mode == 'filter':
            if state is not None:
                state = self._chk(state.unsqueeze(0) if single and isinstance(state, torch.Tensor) and state.dim() == 2 else state, 3, 'state', torch.float64)
                if tuple(state.shape) != (S, n, HH * WW):
                    raise ValueError('state must be [S,M,HH*WW] = %s, got %s' % ((S, n, HH * WW), tuple(state.shape)))
            out['state'] = self._new(S, n, HH * WW, dtype=torch.float64)
            if want_filtered:
                out['filtered'] = self._new(S, n, T, HH, WW)
            self._on_stream(hm4, *([state] if state is not None else []), *out.values())
            _lib.check(self._lib.jcm_seq_tracks_filter(self._h, self._p(hm4), S, T, HH, WW, M, taps, R, float(rho), D, self._p(state), self._p(out.get('filtered')),
                                                       self._p(out['coords']), self._p(out['norm']), self._p(out['reset']), self._p(out['state']),
                                                       self._p(out['value'])), 'jcm_seq_tracks_filter')
        else:
            self._on_stream(hm4, *out.values())
            _lib.check(self._lib.jcm_seq_tracks_viterbi(self._h, self._p(hm4), S, T, HH, WW, M, taps, R, float(rho), D, self._p(out['path']),
                                                        self._p(out['maxes']), self._p(out['breaks']), self._p(out['value'])), 'jcm_seq_tracks_viterbi')
        return {k: t[0] for k, t in out.items()} if single else out

    @staticmethod
    def _chk_decode(decode, use_sm, peaks):
        if decode and not (use_sm and 1 <= peaks <= 4):
            raise ValueError('decode=True needs use_sm=True and 1 <= peaks <= 4 (the candidates are pd_peaks); got use_sm=%s, peaks=%s' % (bool(use_sm), peaks))

    def _dead_slots(self, count, vs, float_fill):
        """The tensors vs, each [B,M,...], with the slots at or beyond count [B] emptied: int32 entries become -1, float entries float_fill --
        -inf through torch.where, 0 by multiplying with the live mask.  A list, made inside the caller's `with torch.cuda.stream(self._stream)`."""
        B, M = vs[0].shape[:2]
        live = torch.arange(M, device=self.device).view(1, M) < count.view(B, 1)          # [B,M]
        lives = [live.view(B, M, *([1] * (v.dim() - 2))) for v in vs]
        return [v * lv.to(v.dtype) if v.dtype != torch.int32 and float_fill == 0
                else torch.where(lv, v, torch.full_like(v, -1 if v.dtype == torch.int32 else float_fill)) for v, lv in zip(vs, lives)]

    def torso_infer(self, prob, want_energy=False, cells=None):
        """The torso map from the part detector (include/jcm.h: jcm_torso_infer): prob [B,60,90,9], the part-detector
        probabilities -> {'cell' int32 [B,2] (row, col): the cell whose nine correlations of joint map and learned prior e_{j|torso} have the
        highest log-sum E, 'torso' fp32 [B,60,90,1]: the 3x3 blob of data.target_heat_maps at it -- the tenth channel spatial_model takes} plus,
        with want_energy, 'energy' fp32 [B,60,90] = E.  cells (int32 [N,2], device): no energy is formed and prob is not read (it may be None);
        'torso' [N,60,90,1] holds the blobs at the given cells, clamped into the map, and 'cell' the clamped cells.  Device tensors; nothing is
        read back.  The geometry is checked by the library."""
        if cells is not None:
            self._chk(cells, 2, 'cells', torch.int32)
            if cells.shape[1] != 2:
                raise ValueError('cells must be [N,2], got %s' % (tuple(cells.shape),))
            N = cells.shape[0]
            out = {'torso': self._new(N, 60, 90, 1)}
            self._on_stream(cells, out['torso'])
            _lib.check(self._lib.jcm_torso_infer(self._h, self._p(None), N, 60, 90, 9, self._p(cells), self._p(None), self._p(None), self._p(out['torso'])),
                       'jcm_torso_infer')
            with torch.cuda.stream(self._stream):
                out['cell'] = torch.stack([cells[:, 0].clamp(0, 59), cells[:, 1].clamp(0, 89)], dim=1)
            return out
        self._chk(prob, 4, 'prob')
        B, H, W, K = prob.shape
        out = {'cell': self._new(B, 2, dtype=torch.int32), 'torso': self._new(B, H, W, 1)}
        if want_energy:
            out['energy'] = self._new(B, H, W)
        self._on_stream(prob, *out.values())
        _lib.check(self._lib.jcm_torso_infer(self._h, self._p(prob), B, H, W, K, self._p(None), self._p(out.get('energy')), self._p(out['cell']),
                                             self._p(out['torso'])), 'jcm_torso_infer')
        return out

    def torso_sm(self, prob, want_prob=True, people=1, people_threshold=0.0, want_torso_prob=False):
        """The spatial model on part-detector probabilities prob [B,60,90,9] that come without a torso map: torso_infer,
        spatial_model on [prob, torso], softmax_argmax -- what forward(torso='infer') runs behind the part detector.  Returns {'sm_coords',
        'torso_cell' int32 [B,2], 'torso' [B,60,90,1], 'hm10' (the spatial model's input, [B * people,60,90,10])} plus 'sm_prob' (want_prob) and,
        for people = M > 1, 'people' (see forward): the torso candidates are the top-M local maxima of spatial_softmax(E) (hm_peaks, K = 1),
        torso_infer(cells=) writes the B * M blobs and the spatial model runs once on B * M images, image b's probabilities repeated for its M
        slots; the top-level entries are slot 0.  want_torso_prob: also 'torso_prob' [B,60,90] = spatial_softmax(E), the map the people's candidates
        are the maxima of and Engine.seq_tracks tracks; every other entry is what the call without it returns."""
        self._chk(prob, 4, 'prob')
        B, K, M = prob.shape[0], 9, int(people)
        if tuple(prob.shape[1:]) != (60, 90, K) or self.n_joints != K:
            raise ValueError('torso_sm expects prob [B,60,90,9] on an engine with 9 joints; got %s, n_joints = %d' % (tuple(prob.shape), self.n_joints))
        if not 1 <= M <= 4:
            raise ValueError('people must be in 1..4, got %r' % (people,))
        t = self.torso_infer(prob, want_energy=M > 1 or bool(want_torso_prob))
        r = {}
        if want_torso_prob:
            r['torso_prob'] = self.spatial_softmax(t['energy'].view(B, 60, 90, 1)).view(B, 60, 90)
        if M == 1:
            with torch.cuda.stream(self._stream):
                hm10 = torch.cat([prob, t['torso']], dim=3)
            sm_prob, r['sm_coords'] = self.softmax_argmax(self.spatial_model(hm10), want_prob=want_prob)
            r['torso_cell'], r['torso'] = t['cell'], t['torso']
        else:
            pk = self.hm_peaks(self.spatial_softmax(t['energy'].view(B, 60, 90, 1)), max_peaks=M, threshold=people_threshold)
            cells = pk['cells'].view(B, M, 2)
            blobs = self.torso_infer(None, cells=cells.view(B * M, 2))['torso']
            with torch.cuda.stream(self._stream):
                hm10 = torch.cat([prob.repeat_interleave(M, dim=0), blobs], dim=3)
            pm, cm = self.softmax_argmax(self.spatial_model(hm10), want_prob=want_prob)
            with torch.cuda.stream(self._stream):
                count = pk['count'].view(B)
                cm, *pm = self._dead_slots(count, [cm.view(B, M, 2, K)] + ([pm.view(B, M, 60, 90, K)] if pm is not None else []), 0)
                pm = pm[0] if pm else None
                r['people'] = {'count': count, 'torso_cell': cells, 'torso_score': pk['scores'].view(B, M), 'sm_coords': cm}
                if pm is not None:
                    r['people']['sm_prob'] = pm
                r['torso_cell'], r['torso'] = cells[:, 0].contiguous(), blobs.view(B, M, 60, 90, 1)[:, 0].contiguous()
                r['sm_coords'] = cm[:, 0].contiguous()
                sm_prob = pm[:, 0].contiguous() if pm is not None else None
        if sm_prob is not None:
            r['sm_prob'] = sm_prob
        r['hm10'] = hm10
        return r

    def _forward_infer(self, x, want_prob, peaks, decode, people, people_threshold, want_torso_prob=False):
        """forward(torso='infer'): the part detector (the forward without spatial model: the same pd_* bits), then torso_sm on its probabilities."""
        B, M = x.shape[0], people
        if (_hm_size(x.shape[1]), _hm_size(x.shape[2]), self.n_joints) != (60, 90, 9):
            raise ValueError("torso='infer' is defined for 60x90 heat maps (480x720 images) and 9 joints; got x %s, n_joints = %d" % (tuple(x.shape), self.n_joints))
        r = self.forward(x, None, use_sm=False, want_prob=True)
        s = self.torso_sm(r['pd_prob'], want_prob=bool(want_prob or peaks), people=M, people_threshold=people_threshold, want_torso_prob=want_torso_prob)
        hm10 = s.pop('hm10')
        scratch = {}
        if not want_prob:
            scratch = {'pd_prob': r.pop('pd_prob'), 'sm_prob': s.pop('sm_prob', None)}
            if M > 1:
                s['people'].pop('sm_prob', None)
        r.update(s)
        self._add_peaks_pose(r, scratch, peaks, decode and M == 1, r['torso'])
        if decode and M > 1:      # per slot: image b's candidates against each of its M torso maps
            rep = {k: r['pd_peaks'][k].repeat_interleave(M, dim=0).contiguous() for k in ('cells', 'count')}
            pose = self.pose_decode(hm10, rep)
            with torch.cuda.stream(self._stream):      # slots at or beyond count have no pose: -1 / -inf, as pose_decode writes an image without one
                r['pose'] = dict(zip(pose, self._dead_slots(r['people']['count'], [v.view(B, M, *v.shape[1:]) for v in pose.values()], float('-inf'))))
        return r

    def softmax_argmax(self, logits, want_prob=True):
        """spatial_softmax + arg-max of the probabilities in one kernel (the tail of forward()):
        [B,H,W,K] logits -> (prob [B,H,W,K] or None, coords int32 [B,2,K])."""
        self._chk(logits, 4, 'logits')
        B, H, W, K = logits.shape
        prob = torch.empty_like(logits) if want_prob else None
        coords = self._new(B, 2, K, dtype=torch.int32)
        _lib.check(self._lib.jcm_softmax_argmax(self._h, self._p(logits), B, H, W, K, self._p(prob), self._p(coords)), 'jcm_softmax_argmax')
        return prob, coords

    def forward(self, x, torso=None, use_sm=True, want_prob=True, peaks=0, decode=False, flip_test=False, people=1, people_threshold=0.0,
                want_torso_prob=False):
        """The tower of main.py:522-531 in one C call.  Returns a dict with 'pd_coords',
        'sm_coords' (int32 [B,2,K]) and, if want_prob, 'pd_prob' / 'sm_prob' [B,60,90,K].  x: float32, or uint8 (byte k standing for
        float32(k) / float32(255): the same bits out as for that float image, a quarter of the bytes in).  peaks = P > 0: also 'pd_peaks'
        and, with use_sm, 'sm_peaks', the dict of hm_peaks(prob, P) of this call's probabilities (kept in a scratch tensor when
        want_prob is False); every other entry is what the call without peaks returns.  decode=True (needs use_sm and 1 <= peaks <= 4): also
        'pose', the dict of pose_decode with pd_peaks as candidates on this call's part-detector probabilities and torso map; every other
        entry is what the call without it returns.  flip_test=True: mirrored test-time evaluation -- ONE forward on
        mirror_pairs(x) (2B images; with use_sm on mirror_pairs(torso)), 'pd_prob' / 'sm_prob' the mirror_merge of its probabilities, [B,...],
        the coords argmax_coords of the merged maps; peaks and decode work on the merged maps (kept in scratch when want_prob is False) and the
        unmirrored torso map.  False changes nothing.  torso='infer' (needs use_sm): no torso map is given -- it is inferred from
        this call's part-detector probabilities (torso_infer) and the spatial model runs on it; the dict gains 'torso_cell' int32 [B,2] and 'torso'
        [B,60,90,1], 'pd_*' are the bits of forward(use_sm=False) and 'sm_*' those of forward(x, torso=r['torso']); peaks and decode as before.
        people = M in 1..4 (with torso='infer'; 1 changes nothing): one spatial-model result per torso candidate, the top-M local maxima of
        spatial_softmax(E) above people_threshold (hm_peaks; slot 0 is the arg-max): the dict gains 'people' = {'count' int32 [B], 'torso_cell'
        int32 [B,M,2], 'torso_score' fp32 [B,M], 'sm_coords' int32 [B,M,2,K], and with want_prob 'sm_prob' [B,M,60,90,K]}, slots at or beyond
        count holding -1 in the coordinates and 0 in the maps; the top-level 'sm_*', 'torso_cell' and 'torso' are slot 0, and with decode 'pose'
        is decoded per slot, [B,M,...].  flip_test=True with torso='infer' is a ValueError.  want_torso_prob (with torso='infer'; False changes
        nothing): the dict gains 'torso_prob' [B,60,90] = spatial_softmax of the torso energy E."""
        self._chk_decode(decode, use_sm, peaks)
        self._chk_img(x, 'x')
        B, H, W, C = x.shape
        if C != 3:
            raise ValueError('x must be [B,H,W,3]')
        infer = isinstance(torso, str)
        if infer and torso != 'infer':
            raise ValueError("torso must be a tensor, None or 'infer', got %r" % (torso,))
        if not isinstance(people, int) or not 1 <= people <= 4 or (people > 1 and not infer):
            raise ValueError("people must be an integer in 1..4 and needs torso='infer' above 1; got people=%r, torso=%s" % (people, 'infer' if infer else 'given'))
        if want_torso_prob and not infer:
            raise ValueError("want_torso_prob needs torso='infer': a given torso map has no energy")
        if infer:
            if not use_sm or flip_test:
                raise ValueError("torso='infer' needs use_sm=True and does not combine with flip_test=True (the torso under mirrored evaluation is not defined); "
                                 'got use_sm=%s, flip_test=%s' % (bool(use_sm), bool(flip_test)))
            return self._forward_infer(x, want_prob, peaks, decode, people, float(people_threshold), bool(want_torso_prob))
        if use_sm:
            if torso is None:
                raise ValueError('use_sm=True needs the torso heat map y_in[..., 9:] (main.py:528)')
            self._chk(torso, 4, 'torso')
            if tuple(torso.shape) != (B, 60, 90, 1):
                raise ValueError('torso must be [B,60,90,1], got %s' % (tuple(torso.shape),))
        if flip_test:
            return self._forward_flip(x, torso, use_sm, want_prob, peaks, decode)
        return self._tower_call('jcm_forward', x, torso if use_sm else None, use_sm, want_prob, peaks, decode, torso)

    def _tower_call(self, entry, x, maps, use_sm, want_prob, peaks, decode, torso, losses=False):
        """The library call forward and eval_forward share: `entry` (its _u8 twin for byte images) on x and `maps` (forward's torso map, eval_forward's
        y) into a new result dict -- 'pd_coords', with use_sm 'sm_coords', with want_prob the '*_prob' maps (with peaks and without want_prob they go
        to a scratch dict instead), with `losses` 'losses' fp32 [2], the entry's last argument -- then the peaks and pose tail."""
        B, H, W, _ = x.shape
        hh, ww, K = _hm_size(H), _hm_size(W), self.n_joints
        r, scratch = {}, {}
        for key in ('pd', 'sm') if use_sm else ('pd',):
            r[key + '_coords'] = self._new(B, 2, K, dtype=torch.int32)
            if want_prob or peaks:
                (r if want_prob else scratch)[key + '_prob'] = self._new(B, hh, ww, K)
        if losses:
            r['losses'] = self._new(2)
        what = entry + ('_u8' if x.dtype == torch.uint8 else '')
        _lib.check(getattr(self._lib, what)(self._h, self._p(x), self._p(maps), B, H, W, int(bool(use_sm)),
                                            self._p(r.get('pd_prob', scratch.get('pd_prob'))), self._p(r.get('sm_prob', scratch.get('sm_prob'))),
                                            self._p(r['pd_coords']), self._p(r.get('sm_coords')), *([self._p(r['losses'])] if losses else [])), what)
        return self._add_peaks_pose(r, scratch, peaks, decode, torso)

    def _forward_flip(self, x, torso, use_sm, want_prob, peaks, decode):
        """forward(flip_test=True): the existing forward on the 2B interleaved images, its maps merged pair by pair."""
        r2 = self.forward(self.mirror_pairs(x), self.mirror_pairs(torso) if use_sm else None, use_sm=use_sm, want_prob=True)
        r, scratch = {}, {}
        for key in (('pd', 'sm') if use_sm else ('pd',)):
            self._on_stream(r2[key + '_prob'])
            prob = self.mirror_merge(r2[key + '_prob'])
            r[key + '_coords'] = self.argmax_coords(prob)
            (r if want_prob else scratch)[key + '_prob'] = prob
        return self._add_peaks_pose(r, scratch, peaks, decode, torso)

    def eval_forward(self, x, y, use_sm=True, want_prob=True, peaks=0, decode=False):
        """The tower in inference mode plus the two cross-entropy losses of the graph (main.py:538-539), as eval_error
        runs it per batch (main.py:275-283).  y = y_in [B,60,90,K+1]: targets + torso channel.  Returns the dict of
        forward() plus 'losses' (device fp32 [2]: loss_pd, loss_sm).  x: float32 or uint8, as for forward(); peaks and decode as for forward()
        (the torso map is channel K of y)."""
        self._chk_decode(decode, use_sm, peaks)
        self._chk_img(x, 'x')
        self._chk(y, 4, 'y')
        B, H, W, C = x.shape
        hh, ww, K = _hm_size(H), _hm_size(W), self.n_joints
        if C != 3 or tuple(y.shape) != (B, hh, ww, K + 1):
            raise ValueError('x must be [B,H,W,3] and y [B,%d,%d,%d]; got %s, %s' % (hh, ww, K + 1, tuple(x.shape), tuple(y.shape)))
        return self._tower_call('jcm_eval_forward', x, y, use_sm, want_prob, peaks, decode, y[..., K:], losses=True)

    def window_resize(self, src, windows, oh, ow):
        """Pad-or-crop `windows` [(src_index, y0, x0, h, w), ...] of src [N,H,W,C], each resized to
        (oh, ow) with skimage.transform.resize's 0.13.x defaults (main.py:326-379)."""
        self._chk(src, 4, 'src')
        N, H, W, C = src.shape
        wins = np.ascontiguousarray(np.asarray(windows, dtype=np.int32).reshape(-1, 5))
        out = self._new(wins.shape[0], int(oh), int(ow), C)
        _lib.check(self._lib.jcm_window_resize(self._h, self._p(src), N, H, W, C,
                                               wins.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), wins.shape[0],
                                               int(oh), int(ow), self._p(out)), 'jcm_window_resize')
        return out

    def group_mean(self, x, group):
        """np.average over consecutive groups of `group` leading entries (main.py:413-414)."""
        if x.shape[0] % group:
            raise ValueError('leading dimension %d is not a multiple of %d' % (x.shape[0], group))
        n = x.shape[0] // group
        out = self._new(n, *x.shape[1:])
        m = 1
        for d in x.shape[1:]:
            m *= int(d)
        _lib.check(self._lib.jcm_group_mean(self._h, self._p(x.contiguous()), n, group, m, self._p(out)), 'jcm_group_mean')
        return out

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
        _lib.check(self._lib.jcm_render_poses(
            self._h, self._p(buf), off, desc.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), B, self._p(buf),
            pr.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)) if pr.shape[0] else None, pr.shape[0], self._p(hm), hh, hw, K, int(stride),
            g4.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)) if g4 is not None else None,
            mask.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)) if mask is not None else None, int(heat_gain)), 'jcm_render_poses')
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
        if out is None:
            if H < 1 or W < 1 or B * H * W * 3 >= 2 ** 40:
                raise ValueError('synth_people: H and W >= 1 and an output below 2^40 elements are expected, got %d x %d x %d' % (B, H, W))
            out = self._new(B, H, W, 3, dtype=dtype)
        else:
            self._chk(out, 4, 'out', dtype)
            if tuple(out.shape) != (B, H, W, 3):
                raise ValueError('out must be [%d,%d,%d,3], got %s' % (B, H, W, tuple(out.shape)))
        self._on_stream(out)
        _lib.check(self._lib.jcm_synth_people(
            self._h, rec.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), B, pr.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)) if pr.shape[0] else None,
            pr.shape[0], H, W, int(dtype == torch.float32), self._p(out)), 'jcm_synth_people')
        return out

    def _fit_run(self, entry, ts, desc, off, rows, sizes, out_hw, pad, dtype, out):
        """What fit_images and fit_windows share once the descriptor array is built: the output frame (`out` checked, or a new one), the images
        ts back to back in one device buffer of `off` bytes (desc[:, 0] their offsets), the library's `entry` on the int64 descriptor `rows`
        [n, 3 or 7], and geom [n,6] = the content rectangles it returns + `sizes` [n,2]."""
        OH, OW = int(out_hw[0]), int(out_hw[1])
        n, C = rows.shape[0], 3
        if out is None:
            out = self._new(n, OH, OW, C, dtype=dtype)
        else:
            self._chk(out, 4, 'out', dtype)
            if tuple(out.shape) != (n, OH, OW, C):
                raise ValueError('out must be [%d,%d,%d,%d], got %s' % (n, OH, OW, C, tuple(out.shape)))
        src = self._fit_pack(ts, desc, off)
        geom = np.empty((n, 6), np.int32)
        g4 = np.empty((n, 4), np.int32)
        self._on_stream(src, out)
        _lib.check(getattr(self._lib, entry)(self._h, self._p(src), off, rows.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), n, C, OH, OW, int(pad),
                                             int(dtype == torch.float32), self._p(out), g4.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))), entry)
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

    def mirror_pairs(self, x):
        """x [B,H,W,C] float32 or uint8 -> [2B,H,W,C] of the same type: out[2b] = x[b], out[2b+1] = x[b] mirrored left/right (out[2b+1,y,xx,c] =
        x[b,y,W-1-xx,c]); bit copies, one launch (include/jcm.h: jcm_mirror_pairs)."""
        if not isinstance(x, torch.Tensor) or x.dtype not in (torch.float32, torch.uint8):
            raise ValueError('mirror_pairs: x must be a float32 or uint8 torch tensor, got %s' % (getattr(x, 'dtype', type(x)),))
        if x.dim() != 4:
            raise ValueError('mirror_pairs: x must have 4 dims (NHWC), got shape %s' % (tuple(x.shape),))
        self._chk(x, 4, 'x', x.dtype)
        B, H, W, C = x.shape
        if min(B, H, W, C) < 1:
            raise ValueError('mirror_pairs: x must not be empty, got shape %s' % (tuple(x.shape),))
        out = self._new(2 * B, H, W, C, dtype=x.dtype)
        self._on_stream(x, out)
        _lib.check(self._lib.jcm_mirror_pairs(self._h, self._p(x), int(x.dtype == torch.uint8), B, H, W, C, self._p(out)), 'jcm_mirror_pairs')
        return out

    def mirror_merge(self, hm, group=2, perm=None):
        """hm [n*group,HH,WW,K] float32, copy g of group i at i*group+g, the odd g maps of mirrored inputs -> [n,HH,WW,K]: the mean over the group
        (float64, g in order, as group_mean) with the odd copies read mirrored back, out[i,y,x,k] from hm[i*group+g,y,WW-1-x,perm[k]].  perm: K host
        integers, a permutation of 0..K-1; None = the FLIC left/right table [3,4,5,0,1,2,7,6,8,9] cut to K (include/jcm.h: jcm_mirror_merge)."""
        if not isinstance(hm, torch.Tensor) or hm.dtype != torch.float32:
            raise ValueError('mirror_merge: hm must be a float32 torch tensor, got %s' % (getattr(hm, 'dtype', type(hm)),))
        if hm.dim() != 4:
            raise ValueError('mirror_merge: hm must have 4 dims [n*group,HH,WW,K], got shape %s' % (tuple(hm.shape),))
        self._chk(hm, 4, 'hm')
        group = int(group)
        N, HH, WW, K = hm.shape
        if group < 2 or group % 2:
            raise ValueError('mirror_merge: group = %d; the copies come in (plain, mirrored) pairs, so it is even and >= 2' % group)
        if N < group or N % group or min(HH, WW, K) < 1:
            raise ValueError('mirror_merge: hm %s is not a whole number of groups of %d non-empty maps' % (tuple(hm.shape), group))
        table = None
        if perm is not None:
            table = np.asarray(perm).reshape(-1)
            if table.dtype.kind not in 'iu' or table.shape[0] != K or sorted(table.tolist()) != list(range(K)):
                raise ValueError('mirror_merge: perm must be a permutation of 0..%d, got %s' % (K - 1, list(np.asarray(perm).reshape(-1).tolist())))
            table = np.ascontiguousarray(table, dtype=np.int32)
        elif K > 10 or sorted(_lib.HM_FLIP_PERM[:K]) != list(range(K)):
            raise ValueError('mirror_merge: the FLIC left/right table cut to K = %d channels is not a permutation; give perm' % K)
        out = self._new(N // group, HH, WW, K)
        self._on_stream(hm, out)
        _lib.check(self._lib.jcm_mirror_merge(self._h, self._p(hm), N // group, group, HH, WW, K,
                                              table.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)) if table is not None else None, self._p(out)), 'jcm_mirror_merge')
        return out

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
        x_out = self._new(*x.shape) if x_out is None else self._chk(x_out, 4, 'x_out')
        y_out = self._new(*y.shape) if y_out is None else self._chk(y_out, 4, 'y_out')
        if x_out.shape != x.shape or y_out.shape != y.shape:
            raise ValueError('x_out / y_out must have the shapes of x / y')
        self._on_stream(x, y, params, x_out, y_out)      # tensors made on torch's current stream: the engine's stream waits for them, and keeps them alive
        _lib.check(self._lib.jcm_augment_train(self._h, self._p(x), self._p(y), self._p(params), B, H, W, hh, hw,
                                               self._p(x_out), self._p(y_out)), 'jcm_augment_train')
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
        if isinstance(idx, torch.Tensor):
            if idx.device.type != 'cpu':
                raise ValueError('%s: idx is a host array (it is checked on the host and travels in the kernel arguments), got a tensor on %s' % (who, idx.device))
            idx = idx.numpy()
        idx = np.asarray(idx)
        if idx.ndim != 1 or idx.size < 1 or idx.dtype.kind not in 'iu':
            raise ValueError('%s: idx must be a non-empty 1-D integer array, got shape %s dtype %s' % (who, idx.shape, idx.dtype))
        if idx.dtype != np.int32:
            if int(idx.min()) < -2 ** 31 or int(idx.max()) >= 2 ** 31:
                raise ValueError('%s: idx does not fit int32' % who)
            idx = idx.astype(np.int32)
        idx = np.ascontiguousarray(idx)
        B = idx.shape[0]
        if params is not None:
            self._chk(params, 2, 'params')
            if tuple(params.shape) != (B, 6):
                raise ValueError('%s expects params [%d,6] for %d indices; got %s' % (who, B, B, tuple(params.shape)))
        x_out = self._new(B, H, W, 3) if x_out is None else self._chk(x_out, 4, 'x_out')
        y_out = self._new(B, *y_all.shape[1:]) if y_out is None else self._chk(y_out, 4, 'y_out')
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
        fn, what = (self._lib.jcm_gather_batch_u8, 'jcm_gather_batch_u8') if x_all.dtype == torch.uint8 else (self._lib.jcm_gather_batch, 'jcm_gather_batch')
        _lib.check(fn(self._h, self._p(x_all), self._p(y_all), N, idx.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), idx.shape[0],
                      H, W, y_all.shape[1], y_all.shape[2], self._p(x_out), self._p(y_out)), what)
        return x_out, y_out

    def augment_train_indexed(self, x_all, y_all, idx, params, x_out=None, y_out=None):
        """augment_train of the images idx[b] of the data set (x_all, y_all) with params[b], read through the index: the same bits as
        gather_batch followed by augment_train, without the gathered copy.  x_all may be uint8 (a byte data set): the same bits as from the
        float data set float32(x_all) / float32(255)."""
        idx, x_out, y_out = self._chk_indexed('augment_train_indexed', x_all, y_all, idx, params, x_out, y_out)
        N, H, W, _ = x_all.shape
        fn, what = ((self._lib.jcm_augment_train_indexed_u8, 'jcm_augment_train_indexed_u8') if x_all.dtype == torch.uint8
                    else (self._lib.jcm_augment_train_indexed, 'jcm_augment_train_indexed'))
        _lib.check(fn(self._h, self._p(x_all), self._p(y_all), N, idx.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                      self._p(params), idx.shape[0], H, W, y_all.shape[1], y_all.shape[2], self._p(x_out), self._p(y_out)), what)
        return x_out, y_out

    # ------------------------------------------------------------------ the affine augmentation (augmentation.py)
    def _affine_call(self, who, x, cells, idx, colour, geom, pad, x_out, y_out, width=None):
        """The checks and the call the two affine entries share; idx None: image b of x / cells itself; width None: the plain entries, else the
        antialiased ones (jcm_augment_affine_aa*) with that [B] array of filter half-widths."""
        from .augmentation import check_affine, check_width
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
            if isinstance(idx, torch.Tensor):
                if idx.device.type != 'cpu':
                    raise ValueError('%s: idx is a host array (it is checked on the host and travels in the kernel arguments), got a tensor on %s' % (who, idx.device))
                idx = idx.numpy()
            idx = np.asarray(idx)
            if idx.ndim != 1 or idx.size < 1 or idx.dtype.kind not in 'iu':
                raise ValueError('%s: idx must be a non-empty 1-D integer array, got shape %s dtype %s' % (who, idx.shape, idx.dtype))
            if idx.dtype != np.int32:
                if int(idx.min()) < -2 ** 31 or int(idx.max()) >= 2 ** 31:
                    raise ValueError('%s: idx does not fit int32' % who)
                idx = idx.astype(np.int32)
            idx = np.ascontiguousarray(idx)
        B = N if idx is None else idx.shape[0]
        colour, geom = check_affine(colour, geom)
        if colour.shape[0] != B:
            raise ValueError('%s: %d parameter rows for a batch of %d' % (who, colour.shape[0], B))
        aa, wp = ('_aa', (check_width(width, B).ctypes.data_as(ctypes.POINTER(ctypes.c_double)),)) if width is not None else ('', ())
        hh, hw = H // 8, W // 8
        x_out = self._new(B, H, W, 3) if x_out is None else self._chk(x_out, 4, 'x_out')
        y_out = self._new(B, hh, hw, 10) if y_out is None else self._chk(y_out, 4, 'y_out')
        if tuple(x_out.shape) != (B, H, W, 3) or tuple(y_out.shape) != (B, hh, hw, 10):
            raise ValueError('x_out / y_out must be [%d,%d,%d,3] and [%d,%d,%d,10]; got %s, %s' % (B, H, W, B, hh, hw, tuple(x_out.shape), tuple(y_out.shape)))
        self._on_stream(x, cells, x_out, y_out)
        cp, gp = colour.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), geom.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
        if idx is None:
            what = 'jcm_augment_affine' + aa
            status = getattr(self._lib, what)(self._h, self._p(x), self._p(cells), cp, gp, *wp, B, H, W, hh, hw, float(pad), self._p(x_out), self._p(y_out))
        else:
            what = 'jcm_augment_affine' + aa + ('_indexed_u8' if u8 else '_indexed')
            status = getattr(self._lib, what)(self._h, self._p(x), self._p(cells), N, idx.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), cp, gp, *wp, B, H, W,
                                              hh, hw, float(pad), self._p(x_out), self._p(y_out))
        _lib.check(status, what)
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

    # ------------------------------------------------------------------ TensorBoard summaries (summary.py)
    def _on_stream(self, *ts):
        cur = torch.cuda.current_stream(self.device)
        if cur != self._stream:
            self._stream.wait_stream(cur)
            for t in ts:
                t.record_stream(self._stream)

    def tensor_stats(self, data, segments, scale=1.0, clip_norm=0.0):
        """Histogram statistics per segment (offset, count) of the flat device tensor `data`, or of the stored trainable
        parameters (jcm_train_param_info layout) when `data` is None.  Returns host (stats float64 [n,4] = min, max, sum,
        sum_squares; counts int64 [n, 3 + JCM_HIST_BUCKETS] = num, n_pos, n_nonfinite, buckets).  clip_norm > 0: the values are
        scaled by the clip factor of the last optimizer update (see jcm_tensor_stats)."""
        seg = np.ascontiguousarray(np.asarray(segments, np.int64).reshape(-1, 2))
        n = seg.shape[0]
        if data is not None:
            self._chk(data, 1, 'data')
            if n and int((seg[:, 0] + seg[:, 1]).max()) > data.numel():
                raise ValueError('tensor_stats: a segment reaches past the end of data (%d elements)' % data.numel())
        stats = self._new(n, 4, dtype=torch.float64)
        counts = self._new(n, 3 + _lib.JCM_HIST_BUCKETS, dtype=torch.int64)
        if data is not None:
            self._on_stream(data)
        _lib.check(self._lib.jcm_tensor_stats(self._h, self._p(data), seg.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), n, float(scale),
                                              float(clip_norm), self._p(stats), self._p(counts)), 'jcm_tensor_stats')
        return stats.cpu().numpy(), counts.cpu().numpy()

    def image_u8(self, x, out=None):
        """NormalizeFloatImage (TF-1.x summary_image_op.cc) per image: x [N,H,W,C] fp32, C in {1, 3} -> uint8 [N,H,W,C] device."""
        self._chk(x, 4, 'x')
        N, H, W, C = x.shape
        out = self._new(N, H, W, C, dtype=torch.uint8) if out is None else self._chk(out, 4, 'out', torch.uint8)
        self._on_stream(x, out)
        _lib.check(self._lib.jcm_image_u8(self._h, self._p(x), N, H, W, C, self._p(out)), 'jcm_image_u8')
        return out

    def act_summary(self, z, name, n_groups=1, pic_channel=7, n_pics=3):
        """main.py:167-168 in one pass over z = conv_layer_pre(., name) [B,H,W,C]: per group of B // n_groups consecutive images (a tower's slice;
        the B % n_groups trailing images are left out) the statistics of tensor_stats, the activation BN(relu(z)) of layer `name`, and channel
        pic_channel of the first n_pics activations of every group.  Returns {'activ' [B,H,W,C] (z itself for a layer without BatchNorm; the
        left-out images are not written), 'stats' float64 [n_groups,4], 'counts' int64 [n_groups, 3 + JCM_HIST_BUCKETS] (host, as tensor_stats),
        'pics' fp32 [n_groups,n_pics,H,W] (device)}.  The arguments are checked by the library."""
        self._chk(z, 4, 'z')
        B, H, W, C = z.shape
        n_groups, n_pics = int(n_groups), int(n_pics)
        has_bn = name + '/BatchNorm/gamma' in self._shapes
        activ = torch.empty_like(z) if has_bn else None
        stats = self._new(max(n_groups, 1), 4, dtype=torch.float64)
        counts = self._new(max(n_groups, 1), 3 + _lib.JCM_HIST_BUCKETS, dtype=torch.int64)
        pics = self._new(max(n_groups, 1), max(n_pics, 0), H, W)
        self._on_stream(*[t for t in (z, activ, stats, counts, pics) if t is not None])
        _lib.check(self._lib.jcm_act_summary(self._h, name.encode(), self._p(z), B, H, W, C, n_groups, int(pic_channel), n_pics, self._p(activ),
                                             self._p(stats), self._p(counts), self._p(pics if n_pics > 0 else None)), 'jcm_act_summary(%s)' % name)
        torch.cuda.current_stream(self.device).wait_stream(self._stream)
        return {'activ': activ if has_bn else z, 'stats': stats.cpu().numpy(), 'counts': counts.cpu().numpy(), 'pics': pics}

    def bn_folded(self, name, n):
        """The folded inference-mode BatchNorm stored for conv layer `name` -> host (scale, shift), float32 [n]."""
        sc, sh = np.empty(int(n), np.float32), np.empty(int(n), np.float32)
        _lib.check(self._lib.jcm_bn_folded(self._h, name.encode(), ctypes.c_void_p(sc.ctypes.data), ctypes.c_void_p(sh.ctypes.data), int(n)), 'jcm_bn_folded(%s)' % name)
        return sc, sh

    def hm_overlay(self, x, hm, n=None):
        """show_img_plus_hm (tensorboard.py:60-71) of the first n images: x [B,H,W,3], hm [B,h,w,9] -> uint8 [n,10,H,W,3] device
        (pictures 0-8: one joint each, 9: all joints)."""
        self._chk(x, 4, 'x')
        self._chk(hm, 4, 'hm')
        B, H, W, C = x.shape
        n = B if n is None else int(n)
        if C != 3 or hm.shape[0] != B or not 1 <= n <= B:
            raise ValueError('hm_overlay expects x [B,H,W,3], hm [B,h,w,K], 1 <= n <= B; got %s, %s, n=%d' % (tuple(x.shape), tuple(hm.shape), n))
        K = hm.shape[3]
        out = self._new(n, K + 1, H, W, 3, dtype=torch.uint8)
        self._on_stream(x, hm, out)
        _lib.check(self._lib.jcm_hm_overlay(self._h, self._p(x), self._p(hm), n, H, W, hm.shape[1], hm.shape[2], K, self._p(out)), 'jcm_hm_overlay')
        return out

    def set_option(self, key, value):
        """jcm_set_option(key, value) -- include/jcm.h lists the keys."""
        _lib.check(self._lib.jcm_set_option(self._h, key.encode(), int(value)), 'jcm_set_option(%s)' % key)

    def get_option(self, key):
        """jcm_get_option(key): the value the handle holds."""
        v = ctypes.c_int64(0)
        _lib.check(self._lib.jcm_get_option(self._h, key.encode(), ctypes.byref(v)), 'jcm_get_option(%s)' % key)
        return v.value

    def set_sm_algo(self, algo):
        """Pairwise-convolution algorithm of the spatial model: 'fft_fused' (default; every transform in LDS, sm_fused.hip / sm_lds.hip;
        'fft' is an alias) or 'direct' (LDS sliding-window VALU kernel, the independent cross-check).  Both are hand-written HIP paths; the
        rocFFT routes of rounds 1-4 ('fft', 'fft_split') were removed in round 5."""
        self.set_option('sm_algo', {'fft': 3, 'fft_fused': 3, 'direct': 1}[algo])

    def set_conv9_fft(self, on):
        """fp32 engines: run the wide 9x9 layers in the frequency domain (in-LDS FFTs + one complex channel GEMM per frequency;
        default) or on the fp32 MFMA accumulation chain.  Both pass the same parity tests."""
        self.set_option('conv9_fft', _flag(on))

    def set_micro_batch(self, n):
        """Images per internal slice of forward(): bounds the workspace when a rank holds a large share of a
        global batch (BASELINE configs[3]: 2048 images over the ranks).  0 = default (256 bf16 / 64 fp32)."""
        self.set_option('micro_batch', int(n))

    def set_profile(self, on):
        self.set_option('profile', _flag(on))

    def profile_read(self, scope):
        """(total_ms, launches) of the HIP-event-bracketed launches of conv layer `scope`."""
        ms, n = ctypes.c_double(0), ctypes.c_int(0)
        _lib.check(self._lib.jcm_profile_read(self._h, scope.encode(), ctypes.byref(ms), ctypes.byref(n)), 'jcm_profile_read')
        return ms.value, n.value

    def conv_kernel_name(self, scope, B, H, W):
        """The HIP kernel a [B,H,W,Cin] launch of conv layer `scope` takes on this engine."""
        buf = ctypes.create_string_buffer(128)
        _lib.check(self._lib.jcm_conv_kernel_name(self._h, scope.encode(), int(B), int(H), int(W), buf, 128), 'jcm_conv_kernel_name')
        return buf.value.decode()

    def workspace_bytes(self):
        return int(self._lib.jcm_workspace_bytes(self._h))
