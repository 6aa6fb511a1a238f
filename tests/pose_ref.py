"""Pose decoding restated in numpy (include/jcm.h: jcm_pose_decode), in two halves that share nothing with the kernels:

  tables64  V and M in float64 from the RAW parameters (energy_*, bias_*, bn_sm/*), through oracle.jcm_oracle.softplus5 / bn_infer;
  search32  the fixed-order sum over all P^K poses by broadcasting, in the dtype of the tables it is given (fp32 tables: the bits of the
            definition; float64 tables: the exact answer and its top-two margin), with the tie rule.

tests/test_pose_cpu.py pins both with hand-computed answers; tests/test_gpu_pose.py holds the kernels to them."""
import numpy as np

from oracle import jcm_oracle as O

K, H, W = 9, 60, 90
DELTA = 1e-6
# Table tolerance of the GPU tests: 4 x the largest |GPU - tables64| measured on the MI355X over the inputs of test_gpu_pose.py::test_tables
# (see that test's docstring and DESIGN.md 4.13); the headroom is for device log / exp differing by an ulp between compiler versions.
TABLE_MEASURED = 6.64e-7      # 6.638e-07: M of the 'init' parameters, P = 4, corner candidates (|M| <= 3.69)
TABLE_BOUND = 4 * TABLE_MEASURED


def pairs(k=K):
    """The unordered joint pairs (a < b) in lexicographic order: the rows of M."""
    return [(a, b) for a in range(k) for b in range(a + 1, k)]


def prior_at(e, cell_j, cell_c):
    """Where conv_mrf reads the 120x180 prior e for the displacement cell_j - cell_c (oracle.conv_mrf_pre on a one-hot map at cell_c, read at cell_j)."""
    return e[(H - 1) + (cell_j[0] - cell_c[0]), (W - 1) + (cell_j[1] - cell_c[1])]


def torso_cell(hm10_b):
    """First-occurrence flat arg-max of channel 9 (oracle.argmax_coords)."""
    i = int(np.argmax(hm10_b[:, :, K].reshape(-1)))
    return i // W, i - (i // W) * W


def tables64(hm10, params, cells, count):
    """hm10 [B,60,90,10] fp32, params: the raw spatial-model parameters, cells [B,9,P,2], count [B,9] -> V [B,9,P], M [B,36,P,P] float64;
    entries of a slot at or beyond count are 0."""
    hm10 = np.asarray(hm10)
    B, P = hm10.shape[0], cells.shape[2]
    u = O.softplus5(O.bn_infer(hm10.astype(np.float64), params, 'bn_sm'))                          # [B,60,90,10]
    sp = lambda key: O.softplus5(np.asarray(params[key], np.float64).reshape(params[key].shape[1], params[key].shape[2]))
    names = O.JOINT_NAMES
    e = {(j, c): sp('energy_%s_%s' % (names[j], names[c])) for j in range(K) for c in range(K + 1) if c != j}
    bs = {(j, c): sp('bias_%s_%s' % (names[j], names[c])) for j in range(K) for c in range(K + 1) if c != j}
    V = np.zeros((B, K, P))
    T = np.zeros((B, K, K, P, P))
    for b in range(B):
        t = torso_cell(hm10[b])
        for j in range(K):
            for pj in range(min(int(count[b, j]), P)):
                cj = tuple(int(v) for v in cells[b, j, pj])
                V[b, j, pj] = (np.log(u[b, cj[0], cj[1], j] + DELTA)
                               + np.log(prior_at(e[j, K], cj, t) * u[b, t[0], t[1], K] + bs[j, K][cj] + DELTA))
                for c in range(K):
                    if c == j:
                        continue
                    for pc in range(min(int(count[b, c]), P)):
                        cc = tuple(int(v) for v in cells[b, c, pc])
                        T[b, j, c, pj, pc] = np.log(prior_at(e[j, c], cj, cc) * u[b, cc[0], cc[1], c] + bs[j, c][cj] + DELTA)
    M = np.stack([T[:, a, c] + T[:, c, a].transpose(0, 2, 1) for a, c in pairs()], axis=1)
    return V, M


def _on(axes, a, n):
    """The array a, its axes placed on `axes` of an n-dimensional broadcast."""
    shape = [1] * n
    for ax, s in zip(axes, a.shape):
        shape[ax] = s
    return a.reshape(shape)


def all_scores(V, M):
    """V [k,P], M [k(k-1)/2,P,P] of one image -> S [P] * k, the score of every pose by the fixed-order sum, in the dtype of V:
    S_0 = V[0,p_0]; inc_i = (((V[i,p_i] + M[0,i,p_0,p_i]) + M[1,i,p_1,p_i]) + ..) + M[i-1,i,p_{i-1},p_i]; S_i = S_{i-1} + inc_i."""
    k, P = V.shape
    assert M.shape == (k * (k - 1) // 2, P, P) and M.dtype == V.dtype
    row = {ab: i for i, ab in enumerate(pairs(k))}
    S = V[0]
    for i in range(1, k):
        inc = _on((i,), V[i], i + 1)
        for a in range(i):
            inc = inc + _on((a, i), M[row[a, i]], i + 1)
        S = S[..., None] + inc
    assert S.dtype == V.dtype and S.shape == (P,) * k
    return S


def search_one(V, M, count):
    """V [k,P], M [k(k-1)/2,P,P], count [k] of one image -> (index [k] int32, score, score0, margin): the arg-max of all_scores over the
    poses with p_j < count[j]; ties to the lexicographically smallest pose; margin = best - second best score (inf when there is one pose).
    Some count 0: (-1 .., -inf, -inf, nan)."""
    k, P = V.shape
    dt = V.dtype
    count = np.minimum(np.maximum(np.asarray(count, np.int64), 0), P)
    if (count == 0).any():
        return np.full(k, -1, np.int32), dt.type(-np.inf), dt.type(-np.inf), float('nan')
    S = all_scores(V, M)
    valid = np.ones((), bool)
    for j in range(k):
        valid = valid & _on((j,), np.arange(P) < count[j], k)
    S = np.where(valid, S, dt.type(-np.inf))
    flat = S.reshape(-1)
    best = int(np.argmax(flat))                                   # first occurrence in C order: p_0 most significant
    index = np.array(np.unravel_index(best, S.shape), np.int32)
    if int(valid.sum()) > 1:
        rest = np.delete(flat, best)
        margin = float(flat[best]) - float(rest.max())
    else:
        margin = float('inf')
    return index, flat[best], S[(0,) * k], margin


def search32(V, M, count, cells=None):
    """Batched search_one: V [B,k,P], M [B,.,P,P], count [B,k] -> {'index' [B,k] int32, 'score' [B], 'score0' [B], 'margin' [B] float64} and,
    given cells [B,k,P,2], 'coords' [B,2,k] int32 (the chosen cells; -1 without a pose)."""
    r = [search_one(V[b], M[b], count[b]) for b in range(V.shape[0])]
    out = {'index': np.stack([x[0] for x in r]), 'score': np.array([x[1] for x in r], V.dtype), 'score0': np.array([x[2] for x in r], V.dtype),
           'margin': np.array([x[3] for x in r], np.float64)}
    if cells is not None:
        idx = out['index']
        got = np.take_along_axis(np.asarray(cells), np.maximum(idx, 0)[:, :, None, None].astype(np.int64), axis=2)[:, :, 0, :]      # [B,k,2]
        got = np.where(idx[:, :, None] < 0, -1, got)
        out['coords'] = got.transpose(0, 2, 1).astype(np.int32)
    return out


# ------------------------------------------------------------------ inputs shared by the CPU and the GPU tests
def noise_hm10(B, seed):
    """[B,60,90,10] fp32: the spatial softmax of 3 * N(0,1) logits on nine joint maps, and a torso blob (synth.make_torso)."""
    from joint_cnn_mrf_amd import synth
    logits = 3 * np.random.RandomState(seed).standard_normal((B, H, W, K))
    return np.concatenate([O.spatial_softmax(logits).astype(np.float32), synth.make_torso(B, seed=seed + 1)], axis=3).astype(np.float32)


def random_cells(B, P, seed):
    """P distinct random cells per (image, joint): cells [B,9,P,2] int32, count [B,9] = P."""
    rs = np.random.RandomState(seed)
    flat = np.stack([rs.choice(H * W, P, replace=False) for _ in range(B * K)]).reshape(B, K, P)
    return np.stack([flat // W, flat % W], axis=3).astype(np.int32), np.full((B, K), P, np.int32)


E2E_SEED = 77


def end_to_end_inputs():
    """The 32 random images of the end-to-end test against float64, P = 3 -> (hm10, cells, count)."""
    return (noise_hm10(32, E2E_SEED),) + random_cells(32, 3, E2E_SEED + 1)


# The planted two-person scene: a fixed skeleton (cell offsets of the nine joints from the torso), person A with the torso at (20,30), person B at
# (40,60); every joint map has a 3x3 blob at A's and at B's joint cell, B's higher on the two wrists, A's on the rest; the torso map is at A.
# The priors are one Gaussian bump per pair at the skeleton's displacement, height 1 (not normalised: main.py:477-487 takes the array as it is).
# SCENE_LOW / SCENE_SIGMA are the blob ratio and the bump width; with them the restatement's float64 margin of the all-A pose over the runner-up
# is SCENE_MARGIN (test_pose_cpu.py::test_planted_scene asserts it is at least 1e-2 and equal to this record).
SKELETON = [(-6, -5), (-1, -8), (4, -9), (-6, 5), (-1, 8), (4, 9), (6, -3), (6, 3), (-10, 0)]
WRISTS = (2, 5)
TORSO_A, TORSO_B = (20, 30), (40, 60)
SCENE_LOW, SCENE_SIGMA = 0.8, 1.5


def scene_priors():
    from joint_cnn_mrf_amd import synth
    off = SKELETON + [(0, 0)]
    yy, xx = np.mgrid[0:120, 0:180].astype(np.float64)
    out = {}
    for key in synth.pair_keys():
        j, c = (synth.JOINT_NAMES.index(n) for n in key.split('_'))
        dy, dx = off[j][0] - off[c][0], off[j][1] - off[c][1]
        out[key] = np.exp(-0.5 * (((yy - (H - 1 + dy)) / SCENE_SIGMA) ** 2 + ((xx - (W - 1 + dx)) / SCENE_SIGMA) ** 2))
    return out


def scene():
    """-> (hm10 [1,60,90,10] fp32, params ('init'), cells_a [9,2], cells_b [9,2])."""
    from joint_cnn_mrf_amd import synth
    hm = np.zeros((1, H, W, K + 1), np.float32)

    def blob(ch, cell, height):
        hm[0, cell[0] - 1:cell[0] + 2, cell[1] - 1:cell[1] + 2, ch] = 0.5 * height
        hm[0, cell[0], cell[1], ch] = height
    a = np.array([(TORSO_A[0] + dy, TORSO_A[1] + dx) for dy, dx in SKELETON], np.int32)
    b = np.array([(TORSO_B[0] + dy, TORSO_B[1] + dx) for dy, dx in SKELETON], np.int32)
    for j in range(K):
        blob(j, a[j], SCENE_LOW if j in WRISTS else 1.0)
        blob(j, b[j], 1.0 if j in WRISTS else SCENE_LOW)
    blob(K, TORSO_A, 1.0)
    return hm, synth.make_sm_params(scene_priors(), 'init'), a, b
