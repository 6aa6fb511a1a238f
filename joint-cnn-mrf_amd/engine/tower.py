"""The tower in one call -- forward, eval_forward, their mirrored and torso-inferring forms -- and what reads its heat maps: peaks, poses, detection rates."""
import numpy as np
import torch

from .. import _lib
from ._core import _f32p, _hm_size, _i32p


class Tower:
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
        self._call('jcm_det_curve', self._p(pred_coords), self._p(y), B, H, W, K, C, _f32p(rad), R,
                   self._p(out.get('true_coords')), self._p(out.get('norm_dist')), self._p(out['hits']))
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
        self._call('jcm_hm_peaks', self._p(hm), B, H, W, K, P, float(threshold), self._p(out['cells']), self._p(out['offsets']), self._p(out['scores']), self._p(out['count']))
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
        self._call('jcm_pose_decode', self._p(hm10), B, self._p(cells), self._p(count), P, self._p(out['index']), self._p(out['coords']),
                   self._p(out['score']), self._p(out['score0']), self._p(out.get('V')), self._p(out.get('M')))
        return out

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
            self._call('jcm_torso_infer', self._p(None), N, 60, 90, 9, self._p(cells), self._p(None), self._p(None), self._p(out['torso']))
            with torch.cuda.stream(self._stream):
                out['cell'] = torch.stack([cells[:, 0].clamp(0, 59), cells[:, 1].clamp(0, 89)], dim=1)
            return out
        self._chk(prob, 4, 'prob')
        B, H, W, K = prob.shape
        out = {'cell': self._new(B, 2, dtype=torch.int32), 'torso': self._new(B, H, W, 1)}
        if want_energy:
            out['energy'] = self._new(B, H, W)
        self._on_stream(prob, *out.values())
        self._call('jcm_torso_infer', self._p(prob), B, H, W, K, self._p(None), self._p(out.get('energy')), self._p(out['cell']), self._p(out['torso']))
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
        self._call(entry + ('_u8' if x.dtype == torch.uint8 else ''), self._p(x), self._p(maps), B, H, W, int(bool(use_sm)), self._p(r.get('pd_prob', scratch.get('pd_prob'))),
                   self._p(r.get('sm_prob', scratch.get('sm_prob'))), self._p(r['pd_coords']), self._p(r.get('sm_coords')), *([self._p(r['losses'])] if losses else []))
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
        self._call('jcm_mirror_pairs', self._p(x), int(x.dtype == torch.uint8), B, H, W, C, self._p(out))
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
        self._call('jcm_mirror_merge', self._p(hm), N // group, group, HH, WW, K, _i32p(table) if table is not None else None, self._p(out))
        return out
