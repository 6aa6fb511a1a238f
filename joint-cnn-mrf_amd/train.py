"""Host side of the joint training step (reference: main.py:464-470,491-506,511-577,644).

`Trainer` wraps an fp32 `Engine`: `loss_and_grads` is one tower's forward (training-mode BatchNorm)
+ `opt.compute_gradients`; `train_step` adds the tower average (an RCCL all-reduce of the flat
gradient buffer when `torch.distributed` is initialised -- average_gradients, main.py:243-267),
`grad_renorm(., 4.0)` and `opt.apply_gradients`.  The arithmetic is libjcm's HIP kernels; torch
only owns the buffers and runs the collective.
"""
import ctypes

import numpy as np
import torch

from . import _lib
from .augmentation import AffineDraw

CLIP_NORM = 4.0      # main.py:576


def piecewise_lr(n_iters, n_updates_total, lr):
    """lr_tf of main.py:467-469,492: tf.train.piecewise_constant(n_iters, round([.7,.8,.9]*total),
    [lr, lr/2, lr/5, lr/10]) -- the value used by update number n_iters+1."""
    bounds = [round(0.7 * n_updates_total), round(0.8 * n_updates_total), round(0.9 * n_updates_total)]
    vals = [lr, lr / 2, lr / 5, lr / 10]
    for b, v in zip(bounds, vals):
        if n_iters <= b:
            return v
    return vals[-1]


class Trainer:
    def __init__(self, engine, optimizer='adam', lr=0.001, lmbd=0.001, use_sm=True, n_updates_total=None, overlap_allreduce=False):
        # fp32 handle: fp32 tensors (frequency domain by default; the fp32 MFMA chain with conv9_fft=False; fp16x3 direct kernels with f32_conv='split16'); bf16 handle: mixed precision
        # (bf16 activations / gradients and bf16 MFMA, fp32 master weights, statistics, losses, spatial model, optimizer)
        if optimizer not in ('adam', 'momentum'):
            raise Exception('wrong optimizer')                      # main.py:506
        self.eng = engine
        self.optimizer, self.lr, self.lmbd, self.use_sm = optimizer, float(lr), float(lmbd), bool(use_sm)
        self.n_updates_total = n_updates_total
        # start each layer's gradient all-reduce (RCCL) as soon as the backward pass has produced it; opt-in.  The boxes
        # of this build have one GPU: the path runs end to end on a one-rank RCCL group (tests/test_gpu_dist.py)
        self.overlap_allreduce = bool(overlap_allreduce)
        self._cb_error = None
        self._lib = engine._lib
        _lib.check(self._lib.jcm_train_begin(engine._h), 'jcm_train_begin')
        nt, ne = ctypes.c_int64(), ctypes.c_int64()
        _lib.check(self._lib.jcm_train_param_count(engine._h, ctypes.byref(nt), ctypes.byref(ne)), 'jcm_train_param_count')
        self.n_elements = ne.value
        self.layout = []                                            # (name, offset, count)
        buf = ctypes.create_string_buffer(256)
        for i in range(nt.value):
            off, cnt = ctypes.c_int64(), ctypes.c_int64()
            _lib.check(self._lib.jcm_train_param_info(engine._h, i, buf, 256, ctypes.byref(off), ctypes.byref(cnt)),
                       'jcm_train_param_info')
            self.layout.append((buf.value.decode(), off.value, cnt.value))
        self.grads = torch.zeros(self.n_elements, dtype=torch.float32, device=engine.device)
        self._moving = None                                         # [(name, offset, count)] of the BN moving statistics
        self._ready_hook = None                                     # user hook(offset, count) for the gradient-ready notifications
        self._pending, self._covered, self._side = [], [], None
        self._cb = _lib.GRAD_READY_FN(self._on_grads_ready)         # keep the ctypes thunk alive as long as the trainer
        _lib.check(self._lib.jcm_train_set_grad_callback(engine._h, ctypes.cast(self._cb, ctypes.c_void_p), None),
                   'jcm_train_set_grad_callback')
        self.losses = torch.zeros(4, dtype=torch.float32, device=engine.device)
        self._aug = None                                            # (x, y, params) buffers of the augmented batch (loss_and_grads(augment=))
        self._aff = None                                            # (x, y) buffers of the affinely augmented batch (augment=AffineDraw)
        self._gat = None                                            # (x, y) buffers of the gathered batch (loss_and_grads_indexed)
        self.last_batch = None                                      # the device batch (x, y) the last step trained on

    @property
    def n_iters(self):
        n = ctypes.c_int64()
        _lib.check(self._lib.jcm_train_steps(self.eng._h, ctypes.byref(n)), 'jcm_train_steps')
        return n.value

    @staticmethod
    def heat_map_size(H, W):
        """The heat-map size (hh, ww) of an H x W image: three SAME stride-2 stages (conv1 and the two pools), ceil(ceil(ceil(n/2)/2)/2)."""
        c = lambda n: -(-n // 2)
        return c(c(c(H))), c(c(c(W)))

    def loss_and_grads(self, x, y, augment=None):
        """x [B,H,W,3], y [B,hh,ww,K+1] (hh x ww = heat_map_size(H, W): 60x90 for 480x720) -> (losses[4] device tensor, flat grads device tensor).
        losses = (loss_tower, loss_pd, loss_sm, weight_decay).  `augment`: None, or a host [B,6] array of augmentation
        parameters (augmentation.draw_params): the step trains on the augmented copy of (x, y) (main.py:494-497); or an
        augmentation.AffineDraw: the step trains on the affine sample of x and on targets redrawn at the transformed arg-max cells of y
        (DESIGN.md 4.20)."""
        e = self.eng
        e._chk(x, 4, 'x')
        e._chk(y, 4, 'y')
        B, H, W, C = x.shape
        hh, ww = self.heat_map_size(H, W)
        if C != 3 or tuple(y.shape) != (B, hh, ww, e.n_joints + 1):      # the kernels read y as [B,hh,ww,K+1]: another size would be read past its end
            raise ValueError('x must be [B,H,W,3] and y [B,%d,%d,%d] (the heat-map size of the image); got %s, %s'
                             % (hh, ww, e.n_joints + 1, tuple(x.shape), tuple(y.shape)))
        if isinstance(augment, AffineDraw):
            xa, ya = self._aff_buffers(x.shape, y.shape, augment)
            x, y = e.augment_affine(x, e.joint_cells(y), augment.colour, augment.geom, augment.pad, xa, ya, width=augment.width)
        elif augment is not None:
            x, y = self._augmented(x, y, augment)
        return self._loss_and_grads(x, y)

    def _loss_and_grads(self, x, y):
        """jcm_train_loss_grads on the checked device batch (x, y) -- what loss_and_grads and loss_and_grads_indexed hand to the step."""
        e = self.eng
        B, H, W, _ = x.shape
        self.last_batch = (x, y)
        self._cb_error = None
        status = self._lib.jcm_train_loss_grads(e._h, e._p(x), e._p(y), B, H, W, int(self.use_sm), self.lmbd,
                                                e._p(self.grads), e._p(self.losses))
        if self._cb_error is not None:      # ctypes swallows exceptions raised inside a callback: re-raise them here
            err, self._cb_error = self._cb_error, None
            self._pending, self._covered = [], []
            raise err
        _lib.check(status, 'jcm_train_loss_grads')
        return self.losses, self.grads

    def _aug_buffers(self, shape_x, shape_y, augment):
        """(x, y, params) buffers of the augmented batch, kept across steps of the same shapes, the parameters uploaded."""
        from .augmentation import check_params
        e = self.eng
        p = check_params(augment)
        if p.shape[0] != shape_x[0]:
            raise ValueError('augment has %d parameter rows for a batch of %d' % (p.shape[0], shape_x[0]))
        if self._aug is None or tuple(self._aug[0].shape) != tuple(shape_x) or tuple(self._aug[1].shape) != tuple(shape_y):
            self._aug = (torch.empty(tuple(shape_x), dtype=torch.float32, device=e.device), torch.empty(tuple(shape_y), dtype=torch.float32, device=e.device),
                         torch.empty(p.shape, dtype=torch.float32, device=e.device))
        xa, ya, pd = self._aug
        with torch.cuda.stream(e._stream):       # behind the previous step's reads of the parameter buffer; the host does not wait
            pd.copy_(torch.from_numpy(p).pin_memory(), non_blocking=True)
        return xa, ya, pd

    def _aff_buffers(self, shape_x, shape_y, draw):
        """(x, y) buffers of the affinely augmented batch, kept across steps of the same shapes (the draw itself travels in the kernel arguments)."""
        if len(draw) != shape_x[0]:
            raise ValueError('augment has %d parameter rows for a batch of %d' % (len(draw), shape_x[0]))
        if self._aff is None or tuple(self._aff[0].shape) != tuple(shape_x) or tuple(self._aff[1].shape) != tuple(shape_y):
            dev = self.eng.device
            self._aff = (torch.empty(tuple(shape_x), dtype=torch.float32, device=dev), torch.empty(tuple(shape_y), dtype=torch.float32, device=dev))
        return self._aff

    def _augmented(self, x, y, augment):
        """The augmented copy of (x, y) in buffers the trainer owns (kept across steps of the same shapes)."""
        xa, ya, pd = self._aug_buffers(x.shape, y.shape, augment)
        return self.eng.augment_train(x, y, pd, xa, ya)

    def loss_and_grads_indexed(self, dataset, idx, augment=None):
        """loss_and_grads on the batch (dataset.x[idx], dataset.y[idx]) of a DeviceDataset on this engine's device: gathered on the device
        (Engine.gather_batch), or with `augment` read by the augmentation through the index (Engine.augment_train_indexed), into buffers
        the trainer owns.  idx: host integers.  Nothing here makes the host wait."""
        e = self.eng
        idx = np.asarray(idx).reshape(-1)
        B, (H, W) = idx.shape[0], dataset.x.shape[1:3]
        hh, ww = self.heat_map_size(H, W)
        if dataset.x.shape[3] != 3 or tuple(dataset.y.shape[1:]) != (hh, ww, e.n_joints + 1):
            raise ValueError('the data set must hold x [N,H,W,3] and y [N,%d,%d,%d] (the heat-map size of the image); got %s, %s'
                             % (hh, ww, e.n_joints + 1, tuple(dataset.x.shape), tuple(dataset.y.shape)))
        shape_x, shape_y = (B, H, W, 3), (B, hh, ww, e.n_joints + 1)
        if isinstance(augment, AffineDraw):
            if getattr(dataset, 'cells', None) is None:
                raise ValueError('the affine augmentation reads the joint cells of the data set: it must have .cells [N,10,2] (dataset.DeviceDataset)')
            xa, ya = self._aff_buffers(shape_x, shape_y, augment)
            x, y = e.augment_affine_indexed(dataset.x, dataset.cells, idx, augment.colour, augment.geom, augment.pad, xa, ya, width=augment.width)
        elif augment is not None:
            xa, ya, pd = self._aug_buffers(shape_x, shape_y, augment)
            x, y = e.augment_train_indexed(dataset.x, dataset.y, idx, pd, xa, ya)
        else:
            if self._gat is None or tuple(self._gat[0].shape) != shape_x:
                self._gat = (torch.empty(shape_x, dtype=torch.float32, device=e.device), torch.empty(shape_y, dtype=torch.float32, device=e.device))
            x, y = e.gather_batch(dataset.x, dataset.y, idx, *self._gat)
        return self._loss_and_grads(x, y)

    def layer_grads(self, scope, x, dz, want_dx=True):
        """The weight gradient (+ lmbd * w) and the data gradient of ONE stride-1 conv layer on given tensors, through the kernels the training
        step uses on this engine: x [B,H,W,Cin], dz [B,H,W,Cout] -> (dw flat numpy [k*k*Cin*Cout] in HWIO order, dx [B,H,W,Cin] device or None).
        fp32 engines take fp32 x and dz; bf16 engines bf16 x and dz (the mixed-precision step's tensors) and return a bf16 dx."""
        e = self.eng
        dt = torch.bfloat16 if e.precision == 'bf16' else torch.float32
        e._chk(x, 4, 'x', dt)
        e._chk(dz, 4, 'dz', dt)
        B, H, W, _ = x.shape
        if tuple(dz.shape[:3]) != (B, H, W):
            raise ValueError('dz must be [%d,%d,%d,Cout]; got %s' % (B, H, W, tuple(dz.shape)))
        dx = torch.empty_like(x) if want_dx else None
        _lib.check(self._lib.jcm_train_layer_grads(e._h, scope.encode(), e._p(x), e._p(dz), B, H, W, self.lmbd, e._p(self.grads), e._p(dx)),
                   'jcm_train_layer_grads(%s)' % scope)
        off, cnt = next((o, c) for n, o, c in self.layout if n == scope + '/weights')
        return self.grads[off:off + cnt].cpu().numpy(), dx

    # ------------------------------------------------------------------ the stages between the convolutions, one at a time (include/jcm.h)
    def _act_dtype(self):
        return torch.bfloat16 if self.eng.precision == 'bf16' else torch.float32

    def _slice(self, name):
        off, cnt = next((o, c) for n, o, c in self.layout if n == name)
        return self.grads[off:off + cnt]

    def bn_forward(self, scope, r, pool=False):
        """Training-mode BatchNorm of layer `scope` on r [B,H,W,C] (jcm_train_bn_fwd): -> (y, pooled y or None, mean [C], rstd [C]); the handle's
        moving statistics advance.  Tensors of the engine's activation type (bf16 engines: bfloat16); the statistics are float32."""
        e = self.eng
        e._chk(r, 4, 'r', self._act_dtype())
        B, H, W, C = r.shape
        y = torch.empty_like(r)
        p = torch.empty((B, (H + 1) // 2, (W + 1) // 2, C), dtype=r.dtype, device=e.device) if pool else None
        mean, rstd = e._new(C), e._new(C)
        _lib.check(self._lib.jcm_train_bn_fwd(e._h, scope.encode(), e._p(r), B, H, W, e._p(y), e._p(p), e._p(mean), e._p(rstd)), 'jcm_train_bn_fwd(%s)' % scope)
        return y, p, mean, rstd

    def bn_backward(self, scope, dy, r, y=None, mean=None, rstd=None, dy_scale=1.0, pooled=False):
        """Backward of BN(relu(.)) of layer `scope` (jcm_train_bn_bwd): dy [B,H,W,C], or with pooled=True the gradient of the 2x2-pooled map (y required)
        -> (dz [B,H,W,C], dgamma, dbeta, dbias: views of self.grads).  mean / rstd: the forward pass's (None: what the handle kept)."""
        e = self.eng
        dt = self._act_dtype()
        e._chk(r, 4, 'r', dt)
        e._chk(dy, 4, 'dy', dt)
        B, H, W, C = r.shape
        if tuple(dy.shape) != ((B, (H + 1) // 2, (W + 1) // 2, C) if pooled else (B, H, W, C)):
            raise ValueError('dy has shape %s for r %s (pooled=%s)' % (tuple(dy.shape), tuple(r.shape), bool(pooled)))
        if y is not None and (e._chk(y, 4, 'y', dt).shape != r.shape):
            raise ValueError('y must have the shape of r')
        for t, n in ((mean, 'mean'), (rstd, 'rstd')):
            if t is not None and (e._chk(t, 1, n).shape[0] != C):
                raise ValueError('%s must be [%d]' % (n, C))
        dz = torch.empty_like(r)
        _lib.check(self._lib.jcm_train_bn_bwd(e._h, scope.encode(), e._p(dy), float(dy_scale), int(bool(pooled)), e._p(r), e._p(y), e._p(mean), e._p(rstd),
                                              B, H, W, e._p(self.grads), e._p(dz)), 'jcm_train_bn_bwd(%s)' % scope)
        return dz, self._slice(scope + '/BatchNorm/gamma'), self._slice(scope + '/BatchNorm/beta'), self._slice(scope + '/biases')

    def resize_backward(self, dy, h, w, scale=1.0):
        """The adjoint of Engine.resize_bilinear from [B,h,w,C], times scale (jcm_train_resize_bwd): dy [B,H,W,C] -> dx [B,h,w,C]."""
        e = self.eng
        e._chk(dy, 4, 'dy', self._act_dtype())
        B, H, W, C = dy.shape
        dx = torch.empty((B, h, w, C), dtype=dy.dtype, device=e.device)
        _lib.check(self._lib.jcm_train_resize_bwd(e._h, e._p(dy), B, h, w, H, W, C, float(scale), e._p(dx)), 'jcm_train_resize_bwd')
        return dx

    def softmax_ce(self, logits, target, gscale=1.0, dz=None, accumulate=False):
        """main.py:220-240 per map (jcm_train_softmax_ce): logits [B,HW,K], target [B,HW,Kt >= K] -> loss [B,K]; dz [B,HW,ldz >= K] (optional, written
        in place): columns < K (+)= gscale * (softmax - target)."""
        e = self.eng
        e._chk(logits, 3, 'logits')
        e._chk(target, 3, 'target')
        B, HW, K = logits.shape
        if tuple(target.shape[:2]) != (B, HW) or target.shape[2] < K:
            raise ValueError('target must be [%d,%d,>=%d]; got %s' % (B, HW, K, tuple(target.shape)))
        if dz is not None and (tuple(e._chk(dz, 3, 'dz').shape[:2]) != (B, HW) or dz.shape[2] < K):
            raise ValueError('dz must be [%d,%d,>=%d]; got %s' % (B, HW, K, tuple(dz.shape)))
        loss = e._new(B, K)
        _lib.check(self._lib.jcm_train_softmax_ce(e._h, e._p(logits), e._p(target), B, HW, K, target.shape[2], float(gscale), e._p(loss), e._p(dz),
                                                  dz.shape[2] if dz is not None else 0, int(bool(accumulate))), 'jcm_train_softmax_ce')
        return loss

    def softmax_backward(self, p, g, dz):
        """dz [B,HW,ldz] += p * (g - sum_px p g) per map (jcm_train_softmax_bwd): p [B,HW,K], g [B,HW,ldg >= K]; dz in place."""
        e = self.eng
        e._chk(p, 3, 'p')
        e._chk(g, 3, 'g')
        e._chk(dz, 3, 'dz')
        B, HW, K = p.shape
        if tuple(g.shape[:2]) != (B, HW) or tuple(dz.shape[:2]) != (B, HW) or g.shape[2] < K or dz.shape[2] < K:
            raise ValueError('g and dz must be [%d,%d,>=%d]; got %s, %s' % (B, HW, K, tuple(g.shape), tuple(dz.shape)))
        _lib.check(self._lib.jcm_train_softmax_bwd(e._h, e._p(p), e._p(g), B, HW, K, g.shape[2], e._p(dz), dz.shape[2]), 'jcm_train_softmax_bwd')
        return dz

    def sm_grads(self, pd_prob, y, gscale=None, dlog=None):
        """The spatial model's training stage by itself (jcm_train_sm_grads): pd_prob [B,5400,K] probabilities, y [B,5400,K+1] targets ->
        (ce [B,K] unscaled, dlog [B,5400,16]); the energy_* / bias_* / bn_sm slices of self.grads take the gradients of gscale * sum(ce) (default
        gscale: 1 / (B K), the step's mean), dlog's channels < K gain the gradient w.r.t. the part detector's logits (dlog=None: added to zeros),
        bn_sm's moving statistics advance.  Nothing else of self.grads is written."""
        e = self.eng
        e._chk(pd_prob, 3, 'pd_prob')
        e._chk(y, 3, 'y')
        B, HW, K = pd_prob.shape
        if (HW, K) != (5400, e.n_joints) or tuple(y.shape) != (B, HW, K + 1):
            raise ValueError('pd_prob must be [B,5400,%d] and y [B,5400,%d]; got %s, %s' % (e.n_joints, e.n_joints + 1, tuple(pd_prob.shape), tuple(y.shape)))
        if dlog is None:
            dlog = torch.zeros((B, HW, 16), dtype=torch.float32, device=e.device)
        elif tuple(e._chk(dlog, 3, 'dlog').shape) != (B, HW, 16):
            raise ValueError('dlog must be [%d,%d,16]; got %s' % (B, HW, tuple(dlog.shape)))
        ce = e._new(B, K)
        _lib.check(self._lib.jcm_train_sm_grads(e._h, e._p(pd_prob), e._p(y), B, float(1.0 / (B * K) if gscale is None else gscale), e._p(ce), e._p(dlog),
                                                e._p(self.grads)), 'jcm_train_sm_grads')
        return ce, dlog

    def grads_dict(self):
        """The flat gradient buffer as {TF variable name: numpy array} (reference shapes unknown here: flat)."""
        g = self.grads.cpu().numpy()
        return {n: g[o:o + c].copy() for n, o, c in self.layout}

    # ------------------------------------------------------------------ tower average overlapped with the backward pass
    def set_ready_hook(self, fn):
        """fn(offset, count) is called from inside loss_and_grads as each layer's gradients become final."""
        self._ready_hook = fn

    def _overlap_active(self):
        import torch.distributed as dist
        return self.overlap_allreduce and dist.is_available() and dist.is_initialized() and dist.get_backend() == 'nccl'

    def _on_grads_ready(self, _user, offset, count):
        """jcm_grad_ready_fn: the kernels writing grads[offset:offset+count] are enqueued on the engine's stream.  With RCCL
        the range's all-reduce starts now, on a side stream behind an event, while the backward pass keeps the compute
        stream busy (xGMI links and MFMA pipes are independent resources); other back ends reduce after the pass."""
        if self._cb_error is not None:
            return                                          # a previous notification failed: stop enqueueing, re-raise after the pass
        try:
            if self._ready_hook is not None:
                self._ready_hook(int(offset), int(count))
            if not self._overlap_active():
                return
            import torch.distributed as dist
            if self._side is None:
                self._side = torch.cuda.Stream(device=self.eng.device)
            ev = torch.cuda.Event()
            ev.record(self.eng._stream)
            self._side.wait_event(ev)
            with torch.cuda.stream(self._side):
                self._pending.append(dist.all_reduce(self.grads[offset:offset + count], async_op=True))
            self._covered.append((int(offset), int(count)))
        except BaseException as exc:                        # noqa: BLE001 -- must not propagate into the C caller
            self._cb_error = exc

    def average_gradients(self):
        """main.py:243-267 across ranks: mean of the per-tower gradients.  Ranges already in flight (see _on_grads_ready)
        are waited for; whatever was not reported during the pass is reduced now."""
        from . import dist as jdist
        if not self._pending:
            jdist.average_gradients(self.grads, stream=self.eng._stream)
            return
        import torch.distributed as dist
        with torch.cuda.stream(self.eng._stream):
            for w in self._pending:
                w.wait()                                    # the compute stream waits for the collective
            pos = 0
            for off, cnt in sorted(self._covered) + [(self.n_elements, 0)]:
                if off > pos:
                    dist.all_reduce(self.grads[pos:off])    # e.g. the spatial-model blocks when use_sm is off (zeros)
                pos = max(pos, off + cnt)
            if dist.get_world_size() > 1:
                self.grads.div_(dist.get_world_size())
        self._pending, self._covered = [], []

    def apply(self, lr=None, want_norm=False):
        """grad_renorm + apply_gradients (main.py:576-577) on self.grads."""
        if lr is None:
            lr = self.lr if self.n_updates_total is None else piecewise_lr(self.n_iters, self.n_updates_total, self.lr)
        norm = ctypes.c_float()
        opt = _lib.JCM_OPT_ADAM if self.optimizer == 'adam' else _lib.JCM_OPT_MOMENTUM
        _lib.check(self._lib.jcm_train_apply(self.eng._h, self.eng._p(self.grads), opt, float(lr), CLIP_NORM,
                                             ctypes.byref(norm) if want_norm else None), 'jcm_train_apply')
        return norm.value if want_norm else None

    def sync_moving_statistics(self, names_and_counts):
        """Keep the replicas identical under data parallelism: every rank advanced moving_mean /
        moving_variance with its own tower's batch statistics (main.py:557 runs the towers' update ops on
        the shared variables one after the other); here the replicas take the mean of the per-rank results,
        i.e. one update with the tower-averaged statistics.  `names_and_counts`: [(name, count)]."""
        import torch.distributed as dist
        if not (dist.is_available() and dist.is_initialized()):
            return
        from . import dist as jdist
        if self._moving is None:
            off, lay = 0, []
            for n, c in names_and_counts:
                lay.append((n, off, c))
                off += c
            self._moving = lay
            self._moving_buf = torch.zeros(off, dtype=torch.float32, device=self.eng.device)
        buf = self._moving_buf
        for n, o, c in self._moving:
            _lib.check(self._lib.jcm_get_tensor(self.eng._h, n.encode(), ctypes.c_void_p(buf.data_ptr() + 4 * o), c), 'jcm_get_tensor(%s)' % n)
        jdist.average_gradients(buf, stream=self.eng._stream)
        for i, (n, o, c) in enumerate(self._moving):
            _lib.check(self._lib.jcm_update_tensor(self.eng._h, n.encode(), ctypes.c_void_p(buf.data_ptr() + 4 * o), c,
                                                   int(i == len(self._moving) - 1)), 'jcm_update_tensor(%s)' % n)

    def train_step(self, x, y, want_norm=False, moving=None, augment=None):
        """One sess.run(train_step) (main.py:644).  Returns (losses tensor, grad norm or None).
        `moving`: [(name, count)] of the BN moving statistics to keep in sync across ranks (N > 1).
        `augment`: host [B,6] augmentation parameters, an augmentation.AffineDraw or None (loss_and_grads)."""
        self.loss_and_grads(x, y, augment=augment)
        self.average_gradients()
        norm = self.apply(want_norm=want_norm)
        if moving:
            self.sync_moving_statistics(moving)
        return self.losses, norm

    def train_step_indexed(self, dataset, idx, want_norm=False, moving=None, augment=None):
        """train_step on the batch idx of a DeviceDataset (loss_and_grads_indexed)."""
        self.loss_and_grads_indexed(dataset, idx, augment=augment)
        self.average_gradients()
        norm = self.apply(want_norm=want_norm)
        if moving:
            self.sync_moving_statistics(moving)
        return self.losses, norm

    @staticmethod
    def moving_statistics_of(params):
        return [(k, int(np.asarray(v).size)) for k, v in sorted(params.items())
                if k.endswith('moving_mean') or k.endswith('moving_variance')]

    def get_tensor(self, name, shape):
        out = np.empty(int(np.prod(shape)), np.float32)
        _lib.check(self._lib.jcm_get_tensor(self.eng._h, name.encode(), ctypes.c_void_p(out.ctypes.data), out.size),
                   'jcm_get_tensor(%s)' % name)
        return out.reshape(shape)

    def get_params(self, like):
        """All stored parameters with the shapes of the dict `like` (what Saver.save would write)."""
        return {k: self.get_tensor(k, np.asarray(v).shape) for k, v in like.items()}
