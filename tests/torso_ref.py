"""The torso map from the part detector restated in float64 numpy (include/jcm.h: jcm_torso_infer); nothing here is shared with
the kernels.

    u_j(a) = softplus5(bn_sm(prob[a, j]))                                   from the RAW parameters, through oracle.jcm_oracle
    C_j(t) = sum_a e_{j|torso}[59 + (a_y - t_y), 89 + (a_x - t_x)] u_j(a)
    E(t)   = sum_j log(C_j(t) + 1e-6)

Three formulations of C_j:
  corr_loops    the plain quadruple loop over (t_y, t_x, a_y, a_x), for a rectangle of torso cells (5400 terms per cell in pure Python: the
                tests run it on a few cells);
  corr_windows  the same sum as ONE matrix product: the 60x90 window of the prior that starts at [59 - t_y, 89 - t_x], flattened, times u;
  corr_fft      the independent second formulation, scipy-free, through numpy.fft: the correlation theorem on the 120x180 frame,
                irfft2(conj(rfft2(e)) * rfft2(u padded)), read back at [(t_y - 59) mod 120, (t_x - 89) mod 180].  No index wraps: a - t + (59, 89)
                lies in [0,118] x [0,178], and u is zero outside the map.
tests/test_torso_cpu.py holds the three against each other (1e-12 relative) and pins sign and index convention by hand; tests/test_gpu_torso.py
takes corr_fft as the reference of the kernels."""
import numpy as np

from oracle import jcm_oracle as O

K, H, W = 9, 60, 90
PH, PW = 120, 180
DELTA = 1e-6
# Energy tolerance of the GPU tests: 4 x the largest |E_gpu - E_f64| measured on the MI355X over the inputs of test_gpu_torso.py::test_energy
# (see that test's docstring and DESIGN.md 4.15) -- the margin DESIGN.md 4.13 took: the terms of C_j are all positive, so the error is the
# rounding of a 5400-term sum and of nine logs, not cancellation; the headroom is for device log / exp differing by an ulp between compiler versions.
ENERGY_MEASURED = {'direct': 2.988e-5}      # the sharp scene, where E reaches -124.3 (an ulp of fp32 there is 7.6e-6); 1.1e-5 on the noise inputs (E ~ 40)
ENERGY_BOUND = {k: 4 * v for k, v in ENERGY_MEASURED.items()}
GAP_FLOOR = 2 * max(ENERGY_BOUND.values())      # a float64 top-2 gap above this decides the cell


def priors64(params):
    """[9,120,180] float64: softplus5 of the raw energy_<j>_torso."""
    return np.stack([O.softplus5(np.asarray(params['energy_%s_torso' % O.JOINT_NAMES[j]], np.float64).reshape(PH, PW)) for j in range(K)])


def lik64(prob, params):
    """prob [B,60,90,9] -> u [B,60,90,9] float64 with the first nine channels of bn_sm."""
    p9 = {k: np.asarray(v)[:K] for k, v in params.items() if k.startswith('bn_sm/')}
    return O.softplus5(O.bn_infer(np.asarray(prob, np.float64), p9, 'bn_sm'))


def corr_loops(e, u, ty_range, tx_range):
    """e [120,180], u [60,90] -> {(t_y, t_x): C(t)} by the definition, term by term."""
    out = {}
    for ty in ty_range:
        for tx in tx_range:
            s = 0.0
            for ay in range(H):
                for ax in range(W):
                    s += float(e[59 + (ay - ty), 89 + (ax - tx)]) * float(u[ay, ax])
            out[ty, tx] = s
    return out


def corr_windows(e, u):
    """e [120,180], u [n,60,90] -> C [n,60,90]: window (i, k) of e, 60x90, starts at [i, k] = [59 - t_y, 89 - t_x]."""
    win = np.lib.stride_tricks.sliding_window_view(e, (H, W))[:H, :W]                 # [60,90,60,90] view, i = 59 - t_y, k = 89 - t_x
    c = win.reshape(H * W, H * W) @ u.reshape(u.shape[0], H * W).T                   # [5400, n]
    return np.ascontiguousarray(c.T.reshape(u.shape[0], H, W)[:, ::-1, ::-1])


def corr_fft(e, u):
    """e [120,180], u [n,60,90] -> C [n,60,90] by the correlation theorem."""
    f = np.fft.irfft2(np.conj(np.fft.rfft2(e, (PH, PW)))[None] * np.fft.rfft2(u, (PH, PW)), (PH, PW))       # f[n] = sum_a e[a - n] u[a]
    return f[:, (np.arange(H) - (H - 1)) % PH][:, :, (np.arange(W) - (W - 1)) % PW]


def corr64(prob, params, corr=corr_fft):
    """-> C [B,9,60,90] float64."""
    e, u = priors64(params), lik64(prob, params)
    return np.stack([corr(e[j], u[:, :, :, j]) for j in range(K)], axis=1)


def energy64(C):
    """C [B,9,60,90] -> E [B,60,90] float64."""
    return np.log(C + DELTA).sum(axis=1)


def energy32(C):
    """The fixed-order fp32 sum of the nine logs of the definition, on the float64 C: every log rounded to fp32, then ((l_0 + l_1) + ..) + l_8 in fp32."""
    logs = np.log(C + DELTA).astype(np.float32)
    e = logs[:, 0]
    for j in range(1, K):
        e = (e + logs[:, j]).astype(np.float32)
    return e


def argmax_cells(E):
    """E [B,60,90] -> (cells int32 [B,2], gap [B]): the first-occurrence arg-max in row-major order and the distance to the second-highest value."""
    flat = E.reshape(E.shape[0], -1)
    i = flat.argmax(axis=1)
    top = np.sort(flat.astype(np.float64), axis=1)[:, -2:]
    return np.stack([i // W, i % W], axis=1).astype(np.int32), top[:, 1] - top[:, 0]


def blobs(cells):
    """cells [n,2] (any integers; clamped into the map) -> [n,60,90,1] fp32 through data.target_heat_maps."""
    from joint_cnn_mrf_amd import data
    c = np.asarray(cells).reshape(-1, 2).astype(np.int64)
    c = np.stack([np.clip(c[:, 0], 0, H - 1), np.clip(c[:, 1], 0, W - 1)], axis=1)
    return data.target_heat_maps(c[:, None, :])


def top_peaks(m, n):
    """m [60,90] -> the first n local maxima by jcm_hm_peaks' rule (value > 0; >= every 8-neighbour, > those of a smaller index), by (value
    descending, index ascending): [(row, col), ...]."""
    found = []
    for r in range(H):
        for c in range(W):
            v = m[r, c]
            if not v > 0:
                continue
            ok = True
            for dr in (-1, 0, 1):
                for dc in (-1, 0, 1):
                    rr, cc = r + dr, c + dc
                    if (dr or dc) and 0 <= rr < H and 0 <= cc < W:
                        ok &= bool(v > m[rr, cc]) if (rr * W + cc) < (r * W + c) else bool(v >= m[rr, cc])
            if ok:
                found.append((-v, r * W + c))
    return [(i // W, i % W) for _, i in sorted(found)[:n]]


def softmax_map(E):
    """E [60,90] -> spatial softmax, float64."""
    z = np.exp(E - E.max())
    return z / z.sum()


# ------------------------------------------------------------------ inputs shared by the CPU and the GPU tests
NOISE_SCALE = 8.0      # logits = NOISE_SCALE * N(0,1): the softmax keeps a handful of cells per map, so E has structure (at scale 3 it is flat to 1e-5)
NOISE_SEEDS = {1: 101, 3: 103, 33: 133}      # batch size -> seed; test_torso_cpu.py holds that the restatement's top-2 gap is clear of GAP_FLOOR on >= 90 % of each


def noise_prob(B, seed, scale=NOISE_SCALE):
    """[B,60,90,9] fp32: the spatial softmax of scale * N(0,1) logits."""
    return O.spatial_softmax(scale * np.random.RandomState(seed).standard_normal((B, H, W, K))).astype(np.float32)


def trained_params(seed=11):
    """Trained-like spatial-model parameters on the seeded synthetic priors (synth.make_sm_params(kind='trained'))."""
    from joint_cnn_mrf_amd import synth
    return synth.make_sm_params(synth.synthetic_priors(), 'trained', seed=seed)


def corner_prob():
    """[4,60,90,9] fp32: image i has, in every joint map, one cell of probability 1 in corner i -- (0,0), (0,89), (59,0), (59,89) -- and zeros
    elsewhere: the correlation then reads prior rows 0 / 118 and columns 0 / 178 at the opposite corners of the torso map."""
    p = np.zeros((4, H, W, K), np.float32)
    for i, (r, c) in enumerate(((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1))):
        p[i, r, c, :] = 1.0
    return p


def underflow_prob(B, seed):
    """[B,60,90,9] fp32: the softmax of 200 * N(0,1) logits -- all but one cell of a map (rarely two) underflow to 0."""
    return O.spatial_softmax(200.0 * np.random.RandomState(seed).standard_normal((B, H, W, K))).astype(np.float32)


def scene():
    """The planted two-person scene of tests/pose_ref.py at the part-detector-map level -> (prob [1,60,90,9] fp32, params, torso_a, torso_b)."""
    import pose_ref
    hm, params, _, _ = pose_ref.scene()
    return np.ascontiguousarray(hm[..., :K]), params, pose_ref.TORSO_A, pose_ref.TORSO_B


def one_person_scene():
    """The same scene with person B taken out of every map -> (prob [1,60,90,9], params, torso_a)."""
    import pose_ref
    prob, params, ta, tb = scene()
    for j, (dy, dx) in enumerate(pose_ref.SKELETON):
        r, c = tb[0] + dy, tb[1] + dx
        prob[0, r - 1:r + 2, c - 1:c + 2, j] = 0
    return prob, params, ta


def tie_scene():
    """Two EQUAL planted skeletons (every blob of height 1) at torso cells (20,30) and (40,60), Gaussian priors -> (prob [1,60,90,9], params,
    first, second).  E(first) and E(second) are sums of the same products, but in another order (the cells a are walked in row-major order and
    the two people sit at different a) and over windows that cut the far tails of the bumps differently: equal to ~1e-12 in float64, to rounding
    in fp32, NOT bit for bit.  What a test can hold on it: the cell is one of the two, and it is the first-occurrence arg-max of the energy the
    device itself returns.  The exact tie is flat_params() below."""
    import pose_ref
    from joint_cnn_mrf_amd import synth
    return _planted(((pose_ref.TORSO_A, 1.0), (pose_ref.TORSO_B, 1.0))), synth.make_sm_params(pose_ref.scene_priors(), 'init'), pose_ref.TORSO_A, pose_ref.TORSO_B


def _planted(people):
    """[1,60,90,9] fp32: for every (torso cell, height) a 3x3 blob (centre = height, ring = half of it) at each joint cell of pose_ref.SKELETON."""
    import pose_ref
    prob = np.zeros((1, H, W, K), np.float32)
    for t, h in people:
        for j, (dy, dx) in enumerate(pose_ref.SKELETON):
            r, c = t[0] + dy, t[1] + dx
            prob[0, r - 1:r + 2, c - 1:c + 2, j] = 0.5 * h
            prob[0, r, c, j] = h
    return prob


def flat_params():
    """Every energy 0 (a constant prior), identity bn_sm: C_j(t) = softplus5(0) * sum_a u_j(a) is the SAME sequence of operations on the same
    numbers for every t in any summation order that does not depend on the values -- an exact tie over all 5400 cells, in float64 and on the
    device; first occurrence in row-major order is (0,0)."""
    from joint_cnn_mrf_amd import synth
    return synth.make_sm_params({k: np.zeros((PH, PW)) for k in synth.pair_keys()}, 'init')


# The sharp scene: the planted skeletons of pose_ref with priors and bn_sm as a TRAINED model has them -- energies far below 0 off the bump
# (raw 12 * bump - 10: softplus5 gives 2.0 at the bump's centre, 0.025 one cell off, 1e-12 two cells off) and a BatchNorm that sends an empty cell
# far below 0 (scale 13.2, shift -10: u = 3.2 at a cell of height 1, 1.88 at 0.9, ~1e-8 on the rings, 4e-23 on empty cells).  Then C_j(t) + d is d
# = 1e-6 wherever joint j of no person explains t, E falls by 9 * log(6.4e6) = 141 within two cells of a torso, and spatial_softmax(E) is EXACTLY 0
# (exp underflows below -104) everywhere but around the planted people: with threshold 0.0 the local maxima are the people and nothing else,
# which is what 'count' of forward(people=M) counts.  Person A has height 1.0 in every map, person B 0.9.
SHARP_B = 0.9


def _sharp_params(bumps):
    from joint_cnn_mrf_amd import synth
    params = synth.make_sm_params({k: 12.0 * v - 10.0 for k, v in bumps.items()}, 'init')
    params['bn_sm/BatchNorm/gamma'] = np.full(10, 13.2 * np.sqrt(1.0 + 1e-3), np.float32)
    params['bn_sm/BatchNorm/beta'] = np.full(10, -10.0, np.float32)
    return params


def corner_params():
    """The sharp recipe with EVERY prior's bump at zero displacement, [59,89]: all nine joints of corner_prob() vote for the corner cell itself,
    so the arg-max (and the blob) of image i sits in corner i, decided by 9 * log(80) = 39, while E at the opposite corner reads the prior's
    far corner."""
    from joint_cnn_mrf_amd import synth
    yy, xx = np.mgrid[0:PH, 0:PW].astype(np.float64)
    bump = np.exp(-0.5 * (((yy - (H - 1)) / 1.5) ** 2 + ((xx - (W - 1)) / 1.5) ** 2))
    return _sharp_params({k: bump for k in synth.pair_keys()})


def sharp_scene(two=True):
    """-> (prob [1,60,90,9] fp32, params, torso_a, torso_b)."""
    import pose_ref
    from joint_cnn_mrf_amd import synth
    prob = _planted(((pose_ref.TORSO_A, 1.0), (pose_ref.TORSO_B, SHARP_B))[:2 if two else 1])
    params = _sharp_params(pose_ref.scene_priors())
    return prob, params, pose_ref.TORSO_A, pose_ref.TORSO_B
