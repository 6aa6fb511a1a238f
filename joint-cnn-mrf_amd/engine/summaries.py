"""What the TensorBoard summaries read from the device."""
import ctypes

import numpy as np
import torch

from .. import _lib
from ._core import _i64p


class Summaries:
    # ------------------------------------------------------------------ TensorBoard summaries (summary.py)
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
        self._call('jcm_tensor_stats', self._p(data), _i64p(seg), n, float(scale), float(clip_norm), self._p(stats), self._p(counts))
        return stats.cpu().numpy(), counts.cpu().numpy()

    def image_u8(self, x, out=None):
        """NormalizeFloatImage (TF-1.x summary_image_op.cc) per image: x [N,H,W,C] fp32, C in {1, 3} -> uint8 [N,H,W,C] device."""
        self._chk(x, 4, 'x')
        N, H, W, C = x.shape
        out = self._given_or_new(out, 'out', N, H, W, C, dtype=torch.uint8)
        self._on_stream(x, out)
        self._call('jcm_image_u8', self._p(x), N, H, W, C, self._p(out))
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
        self._call('jcm_act_summary', name.encode(), self._p(z), B, H, W, C, n_groups, int(pic_channel), n_pics, self._p(activ),
                   self._p(stats), self._p(counts), self._p(pics if n_pics > 0 else None), what='jcm_act_summary(%s)' % name)
        torch.cuda.current_stream(self.device).wait_stream(self._stream)
        return {'activ': activ if has_bn else z, 'stats': stats.cpu().numpy(), 'counts': counts.cpu().numpy(), 'pics': pics}

    def bn_folded(self, name, n):
        """The folded inference-mode BatchNorm stored for conv layer `name` -> host (scale, shift), float32 [n]."""
        sc, sh = np.empty(int(n), np.float32), np.empty(int(n), np.float32)
        self._call('jcm_bn_folded', name.encode(), ctypes.c_void_p(sc.ctypes.data), ctypes.c_void_p(sh.ctypes.data), int(n), what='jcm_bn_folded(%s)' % name)
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
        self._call('jcm_hm_overlay', self._p(x), self._p(hm), n, H, W, hm.shape[1], hm.shape[2], K, self._p(out))
        return out
