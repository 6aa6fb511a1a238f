"""The ops that carry main.py's names, layer by layer, and the small glue entries beside them."""
import numpy as np
import torch

from ._core import _hm_size, _i32p


class Layers:
    # ------------------------------------------------------------------ ops (main.py names)
    def conv_layer(self, x, name, stride, last_layer=False, n_out=None):
        """main.py:156-169."""
        self._chk(x, 4, 'x')
        B, H, W, _ = x.shape
        if n_out is None:
            raise ValueError('n_out is required to size the output')
        out = self._new(B, -(-H // stride), -(-W // stride), n_out)
        self._call('jcm_conv_layer', name.encode(), stride, int(bool(last_layer)), self._p(x), B, H, W, self._p(out), what='jcm_conv_layer(%s)' % name)
        return out

    def conv_layer_pre(self, x, name, stride, n_out):
        """pre_activ of main.py:160: conv_SAME(x, w) + b of ANY stored layer, BatchNorm or not (fp32 engines only) -> [B,ceil(H/s),ceil(W/s),n_out]."""
        self._chk(x, 4, 'x')
        B, H, W, _ = x.shape
        if stride not in (1, 2):
            raise ValueError('stride must be 1 or 2, got %r' % (stride,))
        out = self._new(B, -(-H // stride), -(-W // stride), int(n_out))
        self._on_stream(x, out)
        self._call('jcm_conv_layer_pre', name.encode(), stride, self._p(x), B, H, W, self._p(out), what='jcm_conv_layer_pre(%s)' % name)
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
        self._call('jcm_conv_layer_merged', name.encode(), self._p(x1), self._p(x2), x2.shape[1], x2.shape[2], self._p(x3), x3.shape[1], x3.shape[2],
                   B, H, W, self._p(out), what='jcm_conv_layer_merged(%s)' % name)
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
        self._call('jcm_upsample_merge3', self._p(x1), self._p(x2), sizes[0][0], sizes[0][1], self._p(x3), sizes[1][0], sizes[1][1],
                   B, H, W, C, int(x1.dtype == torch.bfloat16), int(bool(planar)), self._p(out))
        return out

    def max_pool(self, x):
        """main.py:172-174."""
        self._chk(x, 4, 'x')
        B, H, W, C = x.shape
        out = self._new(B, (H + 1) // 2, (W + 1) // 2, C)
        self._call('jcm_max_pool', self._p(x), B, H, W, C, self._p(out))
        return out

    def resize_bilinear(self, x, oh, ow):
        """tf.image.resize_images, TF-1.x legacy bilinear (main.py:51,58,60,67,89)."""
        self._chk(x, 4, 'x')
        B, H, W, C = x.shape
        out = self._new(B, oh, ow, C)
        self._call('jcm_resize_bilinear', self._p(x), B, H, W, C, oh, ow, self._p(out))
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
        self._call('jcm_conv1_pool', scope.encode(), self._p(x), int(u8), B, H, W, int(sub), self._p(out), what='jcm_conv1_pool(%s)' % scope)
        return out

    def conv2_pool(self, p1, scope):
        """pool2(conv2_<res>(p1)) (main.py:46-47,54-55,63-64) of a bf16 engine as the tower runs it: p1 [B,H,W,Cin] bfloat16 -> [B,ceil(H/2),ceil(W/2),Cout]
        bfloat16.  An fp32 engine raises RuntimeError: its tower never materialises the pooled map."""
        self._chk(p1, 4, 'p1', torch.bfloat16)
        B, H, W, _ = p1.shape
        n_out = self._shapes[scope + '/weights'][3]
        out = self._new(B, (H + 1) // 2, (W + 1) // 2, n_out, dtype=torch.bfloat16)
        self._on_stream(p1, out)
        self._call('jcm_conv2_pool', scope.encode(), self._p(p1), B, H, W, self._p(out), what='jcm_conv2_pool(%s)' % scope)
        return out

    def model(self, x):
        """main.py:29-74: [B,H,W,3] (float32 or uint8) -> logits [B,H/8,W/8,K]."""
        u8 = self._chk_img(x, 'x')
        B, H, W, C = x.shape
        if C != 3:
            raise ValueError('x must be [B,H,W,3], got %s' % (tuple(x.shape),))
        out = self._new(B, _hm_size(H), _hm_size(W), self.n_joints)
        self._call('jcm_pd_forward' + ('_u8' if u8 else ''), self._p(x), B, H, W, self._p(out))
        return out

    def spatial_softmax(self, hm):
        """main.py:212-217."""
        self._chk(hm, 4, 'hm')
        B, H, W, K = hm.shape
        out = torch.empty_like(hm)
        self._call('jcm_spatial_softmax', self._p(hm), B, H * W, K, self._p(out))
        return out

    def conv_mrf(self, A, Bm):
        """main.py:77-91: A [1,120,180,1], B [b,60,90,1] -> [b,60,90,1]."""
        self._chk(A, 4, 'A')
        self._chk(Bm, 4, 'B')
        if tuple(A.shape) != (1, 120, 180, 1) or tuple(Bm.shape[1:]) != (60, 90, 1):
            raise ValueError('conv_mrf expects A [1,120,180,1] and B [b,60,90,1]; got %s, %s' % (tuple(A.shape), tuple(Bm.shape)))
        out = torch.empty_like(Bm)
        self._call('jcm_conv_mrf', self._p(A), self._p(Bm), Bm.shape[0], self._p(out))
        return out

    def spatial_model(self, heat_map):
        """main.py:94-125: [B,60,90,K+1] -> [B,60,90,K]."""
        self._chk(heat_map, 4, 'heat_map')
        B = heat_map.shape[0]
        if tuple(heat_map.shape[1:]) != (60, 90, self.n_joints + 1):
            raise ValueError('spatial_model expects [B,60,90,%d], got %s' % (self.n_joints + 1, tuple(heat_map.shape)))
        out = self._new(B, 60, 90, self.n_joints)
        self._call('jcm_sm_forward', self._p(heat_map), B, self._p(out))
        return out

    def argmax_coords(self, hm):
        """evaluation.py:15-24: [B,H,W,K] -> int32 [B,2,K] (row, col)."""
        self._chk(hm, 4, 'hm')
        B, H, W, K = hm.shape
        out = self._new(B, 2, K, dtype=torch.int32)
        self._call('jcm_argmax_coords', self._p(hm), B, H, W, K, self._p(out))
        return out

    def softmax_argmax(self, logits, want_prob=True):
        """spatial_softmax + arg-max of the probabilities in one kernel (the tail of forward()):
        [B,H,W,K] logits -> (prob [B,H,W,K] or None, coords int32 [B,2,K])."""
        self._chk(logits, 4, 'logits')
        B, H, W, K = logits.shape
        prob = torch.empty_like(logits) if want_prob else None
        coords = self._new(B, 2, K, dtype=torch.int32)
        self._call('jcm_softmax_argmax', self._p(logits), B, H, W, K, self._p(prob), self._p(coords))
        return prob, coords

    def window_resize(self, src, windows, oh, ow):
        """Pad-or-crop `windows` [(src_index, y0, x0, h, w), ...] of src [N,H,W,C], each resized to
        (oh, ow) with skimage.transform.resize's 0.13.x defaults (main.py:326-379)."""
        self._chk(src, 4, 'src')
        N, H, W, C = src.shape
        wins = np.ascontiguousarray(np.asarray(windows, dtype=np.int32).reshape(-1, 5))
        out = self._new(wins.shape[0], int(oh), int(ow), C)
        self._call('jcm_window_resize', self._p(src), N, H, W, C, _i32p(wins), wins.shape[0], int(oh), int(ow), self._p(out))
        return out

    def group_mean(self, x, group):
        """np.average over consecutive groups of `group` leading entries (main.py:413-414)."""
        if x.shape[0] % group:
            raise ValueError('leading dimension %d is not a multiple of %d' % (x.shape[0], group))
        n = x.shape[0] // group
        out = self._new(n, *x.shape[1:])
        self._call('jcm_group_mean', self._p(x.contiguous()), n, group, int(np.prod(x.shape[1:])), self._p(out))
        return out
