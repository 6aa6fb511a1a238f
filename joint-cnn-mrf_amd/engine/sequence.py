"""Clips: the temporal scans of a clip's heat maps, the frame-to-frame motion estimates that feed them, and the clip pose decode."""
import numpy as np
import torch

from .. import motion
from ._core import _drop, _f64p, _host_table, _lift


class Sequence:
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
        try:
            V, M, count, cells, tau = (self._chk(t.unsqueeze(0) if single and isinstance(t, torch.Tensor) else t, n, name, dt) for t, n, name, dt in (
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
        self._call('jcm_seq_pose_viterbi', self._p(V), self._p(M), self._p(count), self._p(cells), self._p(tau), S, T, P, self._p(out['index']),
                   self._p(out['coords']), self._p(out['frame_score']), self._p(out['maxes']), self._p(out['breaks']))
        return _drop(out, single)

    def _seq_args(self, hm, sigma, radius):
        """hm [T,HH,WW,K] or [S,T,HH,WW,K] -> (hm as [S,T,HH,WW,K], whether a sequence axis was added, host taps [K,2R+1], R)."""
        if not isinstance(hm, torch.Tensor) or hm.dim() not in (4, 5):
            raise ValueError('hm must be a device tensor [T,HH,WW,K] or [S,T,HH,WW,K]')
        single = hm.dim() == 4
        hm5 = self._chk(_lift(hm, 5, single), 5, 'hm')
        R, taps = motion.seq_kernel(sigma, radius, hm5.shape[4])
        return hm5, single, taps, R

    def _seq_shift(self, shift, S, T, single):
        """shift: int32 [T,2] (a 4-d hm) or [S,T,2] = (sy, sx), host or device -> a contiguous device int32 [S,T,2]."""
        shift = _lift(_host_table('shift', shift), 3, single)
        if tuple(shift.shape) != (S, T, 2):
            raise ValueError('shift must be [S,T,2] = %s (or [T,2] with a 4-d hm), got %s' % ((S, T, 2), tuple(shift.shape)))
        return shift.to(self.device).contiguous()

    def _seq_centre(self, centre, shift, S, T, HH, WW, single):
        """centre: int32 [T,HH,WW,2] (a 4-d hm) or [S,T,HH,WW,2] = (sy, sx) per cell, host or device -> a contiguous device int32 [S,T,HH,WW,2]."""
        if shift is not None:
            raise ValueError('centre and shift are two forms of one thing: a shift per cell or one per frame; give one of them')
        centre = _lift(_host_table('centre', centre), 5, single)
        if tuple(centre.shape) != (S, T, HH, WW, 2):
            raise ValueError('centre must be [S,T,HH,WW,2] = %s (or [T,HH,WW,2] with a 4-d hm), got %s' % ((S, T, HH, WW, 2), tuple(centre.shape)))
        return centre.to(self.device).contiguous()

    def _seq_lattice(self, shift, centre, S, T, HH, WW, single):
        """The plain / _moving / _centred choice of seq_filter and seq_viterbi -> (the entry name's suffix, the device table it takes behind rho: a tuple of one or none)."""
        if centre is not None:
            return '_centred', (self._seq_centre(centre, shift, S, T, HH, WW, single),)      # which refuses centre with shift
        if shift is not None:
            return '_moving', (self._seq_shift(shift, S, T, single),)
        return '', ()

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
        suffix, table = self._seq_lattice(shift, centre, S, T, HH, WW, single)
        if state is not None:
            state = self._chk(_lift(state, 4, single), 4, 'state', torch.float64)
            if tuple(state.shape) != (S, K, HH, WW):
                raise ValueError('state must be [S,K,HH,WW] = %s, got %s' % ((S, K, HH, WW), tuple(state.shape)))
        out = {'filtered': self._new(S, T, HH, WW, K), 'coords': self._new(S, T, 2, K, dtype=torch.int32), 'norm': self._new(S, T, K, dtype=torch.float64),
               'reset': self._new(S, T, K, dtype=torch.int32), 'state': self._new(S, K, HH, WW, dtype=torch.float64)}
        self._on_stream(hm5, *([state] if state is not None else []), *table, *out.values())
        self._call('jcm_seq_filter' + suffix, self._p(hm5), S, T, HH, WW, K, _f64p(taps), R, float(rho), *map(self._p, table), self._p(state),
                   self._p(out['filtered']), self._p(out['coords']), self._p(out['norm']), self._p(out['reset']), self._p(out['state']))
        return _drop(out, single)

    def seq_viterbi(self, hm, sigma, rho, radius=None, shift=None, centre=None):
        """The most probable track through a clip's heat maps (include/jcm.h: jcm_seq_viterbi); hm, sigma, rho and radius as for
        seq_filter.  Returns {'path' int32 [S,T,2,K] (row, col), 'maxes' float64 [S,T,K], 'breaks' int32 [S,T,K]}, device tensors without the S
        axis for a 4-d hm; nothing is read back.  The back-pointers (2 bytes per cell, frame, joint and sequence) live in the engine's
        workspace; a clip they do not fit in is a RuntimeError that names the bytes.
        shift: as for seq_filter (include/jcm.h: jcm_seq_viterbi_moving); 'path' is in every frame's own lattice, shift[0] is ignored.
        centre: as for seq_filter (include/jcm.h: jcm_seq_viterbi_centred); centre[0] is never read.  centre with shift is a ValueError."""
        hm5, single, taps, R = self._seq_args(hm, sigma, radius)
        S, T, HH, WW, K = hm5.shape
        suffix, table = self._seq_lattice(shift, centre, S, T, HH, WW, single)
        out = {'path': self._new(S, T, 2, K, dtype=torch.int32), 'maxes': self._new(S, T, K, dtype=torch.float64), 'breaks': self._new(S, T, K, dtype=torch.int32)}
        self._on_stream(hm5, *table, *out.values())
        self._call('jcm_seq_viterbi' + suffix, self._p(hm5), S, T, HH, WW, K, _f64p(taps), R, float(rho), *map(self._p, table),
                   self._p(out['path']), self._p(out['maxes']), self._p(out['breaks']))
        return _drop(out, single)

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
        self._call('jcm_frame_shift', self._p(x), T, H, W, y0, x0, ch, cw, int(search), self._p(prev), self._p(out['disp']), self._p(out['sad']))
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
        ref = _host_table('ref', ref)
        if ref.dim() != 2 or ref.shape[0] != T:
            raise ValueError('ref must be [T,R] = [%d,R], got %s' % (T, tuple(ref.shape)))
        ref = ref.to(self.device).contiguous()
        R = int(ref.shape[1])
        y0, x0, ch, cw = (int(v) for v in rect)
        out = {'flow': self._new(T, R, H // 8, W // 8, 2, dtype=torch.int32), 'sad': self._new(T, R, H // 8, W // 8, 2, dtype=torch.int32)}
        self._on_stream(x, ref, *out.values())
        self._call('jcm_frame_flow', self._p(x), T, H, W, y0, x0, ch, cw, int(search), self._p(ref), R, self._p(out['flow']), self._p(out['sad']))
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
        self._call('jcm_hm_flow_pool', self._p(hm), T, HH, WW, K, self._p(flow), N, _f64p(w), self._p(out))
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
        self._call('jcm_seq_smooth', self._p(hm5), S, T, HH, WW, K, _f64p(taps), R, float(rho), self._p(out.get('smoothed')), self._p(out['coords']),
                   self._p(out['conf']), self._p(out['norm']), self._p(out['reset']), self._p(out['mass']), self._p(out['cut']), self._p(out['trans']))
        return _drop(out, single)

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
            self._call('jcm_seq_smooth_lag', self._p(win['hm']), S, W, P, HH, WW, K, _f64p(taps), R, float(rho), L, int(flush), self._p(win['belief']), self._p(win['norm']),
                       self._p(win['reset']), self._p(out.get('smoothed')), self._p(out['coords']), self._p(out['conf']), self._p(out['mass']), self._p(out['cut']))
            out['norm'], out['reset'] = win['norm'][:, :E].contiguous(), win['reset'][:, :E].contiguous()
            out = _drop(out, single)
            out['lag'] = torch.clamp(torch.arange(W - 1, W - 1 - E, -1, dtype=torch.int32, device=self.device), max=L)
            out['state'] = None if flush else dict(sig, **{k: v[:, E:].contiguous() for k, v in win.items()})
        return out

    def seq_fit(self, hm, sigma=None, rho=None, iters=10, radius=16, fit_rho=True):
        """motion.seq_fit on this engine: sigma per joint and rho re-estimated on the clip's own maps (EM, one seq_smooth per iteration)."""
        return motion.seq_fit(self, hm, motion.SEQ_SIGMA if sigma is None else sigma, motion.SEQ_RHO if rho is None else rho, iters=iters, radius=radius,
                              fit_rho=fit_rho)

    def seq_tracks(self, hm, people, sigma, rho, radius=None, exclude=motion.SEQ_EXCLUDE, mode='viterbi', state=None, want_filtered=False):
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
        hm4 = self._chk(_lift(hm, 4, single), 4, 'hm')
        S, T, HH, WW = hm4.shape
        M, D = int(people), int(exclude)
        R, tap_row = motion.seq_kernel(sigma, radius, 1)
        n = max(M, 0)
        cells, v, f = motion.SEQ_KEYS[mode]
        out = {cells: self._new(S, n, T, 2, dtype=torch.int32), v: self._new(S, n, T, dtype=torch.float64), f: self._new(S, n, T, dtype=torch.int32),
               'value': self._new(S, n, T)}
        if mode == 'filter':
            if state is not None:
                state = self._chk(_lift(state, 3, single), 3, 'state', torch.float64)
                if tuple(state.shape) != (S, n, HH * WW):
                    raise ValueError('state must be [S,M,HH*WW] = %s, got %s' % ((S, n, HH * WW), tuple(state.shape)))
            out['state'] = self._new(S, n, HH * WW, dtype=torch.float64)
            if want_filtered:
                out['filtered'] = self._new(S, n, T, HH, WW)
            self._on_stream(hm4, *([state] if state is not None else []), *out.values())
            self._call('jcm_seq_tracks_filter', self._p(hm4), S, T, HH, WW, M, _f64p(tap_row), R, float(rho), D, self._p(state), self._p(out.get('filtered')),
                       self._p(out['coords']), self._p(out['norm']), self._p(out['reset']), self._p(out['state']), self._p(out['value']))
        else:
            self._on_stream(hm4, *out.values())
            self._call('jcm_seq_tracks_viterbi', self._p(hm4), S, T, HH, WW, M, _f64p(tap_row), R, float(rho), D, self._p(out['path']),
                       self._p(out['maxes']), self._p(out['breaks']), self._p(out['value']))
        return _drop(out, single)
