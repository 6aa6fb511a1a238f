"""The handle itself -- creation and release, parameters, options, profile -- and the helpers every other module of the package calls through."""
import ctypes

import numpy as np
import torch

from .. import _lib


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


# contiguous host numpy array -> the pointer to its elements, as the library declares it; the caller keeps the array alive over the call
_f64p, _f32p, _i32p, _i64p, _u8p = ((lambda a, T=T: a.ctypes.data_as(ctypes.POINTER(T)))
                                    for T in (ctypes.c_double, ctypes.c_float, ctypes.c_int32, ctypes.c_int64, ctypes.c_uint8))


def _host_table(name, value):
    """shift, centre, ref: a host integer array as a contiguous int32 torch tensor on the host, range-checked, or the torch tensor given after its dtype check."""
    if not isinstance(value, torch.Tensor):
        a = np.asarray(value)
        if a.dtype.kind not in 'iu' or a.size and (a.min() < -2 ** 31 or a.max() >= 2 ** 31):
            raise ValueError('%s must hold int32 values, got %s' % (name, a.dtype))
        value = torch.from_numpy(np.ascontiguousarray(a.astype(np.int32)))
    if value.dtype != torch.int32:
        raise ValueError('%s must be int32, got %s' % (name, value.dtype))
    return value


def _host_index(who, idx):
    """The idx of an indexed entry -> a contiguous, non-empty 1-D np.int32 array; the entry point itself checks the RANGE, on the host."""
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
    return np.ascontiguousarray(idx)


def _lift(t, ndim, single):
    """The optional leading sequence axis on the way in: a tensor of ndim - 1 dims gains it in a `single` call (one whose maps came without)."""
    return t.unsqueeze(0) if single and isinstance(t, torch.Tensor) and t.dim() == ndim - 1 else t


def _drop(out, single):
    """... and on the way out: the result dict with axis 0 taken off every tensor of a `single` call."""
    return {k: v[0] for k, v in out.items()} if single else out


class Core:
    def __init__(self, device=0, precision='fp32', n_joints=9, stream=None, f32_conv=None, split_min_wgs=None, micro_batch=None,
                 conv9_fft=None, call_order=None, fft_single=None, fft_t16=None, fft_fuse=None, fft_tiles=None, fft_logits_rows=None):
        if not torch.cuda.is_available():
            raise RuntimeError('joint-cnn-mrf_amd needs an MI355X (gfx950) GPU; torch.cuda.is_available() is False and there is no CPU path')
        self._lib = lib = _lib.load()
        self.device = torch.device('cuda', device if isinstance(device, int) else torch.device(device).index or 0)
        self.n_joints = int(n_joints)
        self.precision = precision
        self._stream = stream if stream is not None else torch.cuda.current_stream(self.device)
        self._h = ctypes.c_void_p()
        _lib.check(lib.jcm_create(self.device.index, ctypes.c_void_p(self._stream.cuda_stream), ctypes.byref(self._h)), 'jcm_create')      # no handle yet: not _call's shape
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
        self._call('jcm_set_tensor', name.encode(), ctypes.c_void_p(ptr), arr, len(shape), what='jcm_set_tensor(%s)' % name)
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
        self._call('jcm_update_tensor', name.encode(), ctypes.c_void_p(a.ctypes.data), a.size, int(bool(refresh)), what='jcm_update_tensor(%s)' % name)

    def finalize(self):
        self._call('jcm_finalize')
        self._finalized = True

    # ------------------------------------------------------------------ helpers
    def _call(self, name, *args, what=None):      # entry `name` on this handle; a status other than JCM_OK raises under `what` (default: the name)
        _lib.check(getattr(self._lib, name)(self._h, *args), what or name)

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

    def _given_or_new(self, t, name, *shape, dtype=torch.float32):      # an output the caller may give (4-d); a given one's shape is the caller's to check
        return self._new(*shape, dtype=dtype) if t is None else self._chk(t, 4, name, dtype)

    @staticmethod
    def _p(t):
        return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)

    def _on_stream(self, *ts):
        cur = torch.cuda.current_stream(self.device)
        if cur != self._stream:
            self._stream.wait_stream(cur)
            for t in ts:
                t.record_stream(self._stream)

    # ------------------------------------------------------------------ options and profile
    def set_option(self, key, value):
        """jcm_set_option(key, value) -- include/jcm.h lists the keys."""
        self._call('jcm_set_option', key.encode(), int(value), what='jcm_set_option(%s)' % key)

    def get_option(self, key):
        """jcm_get_option(key): the value the handle holds."""
        v = ctypes.c_int64(0)
        self._call('jcm_get_option', key.encode(), ctypes.byref(v), what='jcm_get_option(%s)' % key)
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
        self._call('jcm_profile_read', scope.encode(), ctypes.byref(ms), ctypes.byref(n))
        return ms.value, n.value

    def conv_kernel_name(self, scope, B, H, W):
        """The HIP kernel a [B,H,W,Cin] launch of conv layer `scope` takes on this engine."""
        buf = ctypes.create_string_buffer(128)
        self._call('jcm_conv_kernel_name', scope.encode(), int(B), int(H), int(W), buf, 128)
        return buf.value.decode()

    def workspace_bytes(self):
        return int(self._lib.jcm_workspace_bytes(self._h))
