"""The float64 restatement of the torso inference (tests/torso_ref.py; include/jcm.h: jcm_torso_infer) pinned without a GPU: its
formulations against each other, the sign and the index convention by hand, the blob against data.target_heat_maps, and the properties of the
shared inputs that tests/test_gpu_torso.py relies on."""
import numpy as np
import pytest

import joint_cnn_mrf_amd  # noqa: F401
from joint_cnn_mrf_amd import data

import pose_ref
import torso_ref as T

K, H, W = T.K, T.H, T.W


@pytest.fixture(scope='module')
def noise():
    params = T.trained_params()
    prob = T.noise_prob(2, 5)
    return prob, params, T.priors64(params), T.lik64(prob, params)


def test_formulations_agree(noise):
    """Window product and correlation theorem on whole maps, the quadruple loop at the four corners and one interior cell: 1e-12 relative."""
    prob, params, e, u = noise
    for j in (0, 8):
        a, b = T.corr_windows(e[j], u[:, :, :, j]), T.corr_fft(e[j], u[:, :, :, j])
        assert a.shape == b.shape == (2, H, W)
        assert np.abs(a - b).max() <= 1e-12 * np.abs(a).max()
        loops = T.corr_loops(e[j], u[1, :, :, j], (0, 59), (0, 89))
        loops.update(T.corr_loops(e[j], u[1, :, :, j], (17,), (63,)))
        for (ty, tx), v in loops.items():
            assert abs(v - a[1, ty, tx]) <= 1e-12 * abs(v) and abs(v - b[1, ty, tx]) <= 1e-12 * abs(v), (j, ty, tx)
    C = T.corr64(prob, params)
    assert np.abs(C - T.corr64(prob, params, corr=T.corr_windows)).max() <= 1e-12 * C.max()
    assert np.abs(T.energy32(C) - T.energy64(C)).max() <= 9 * 2.0 ** -24 * 8 + 8 * 2.0 ** -24 * 64      # nine logs below 8, eight sums below 64


def _deltas(t_star, d, heights):
    """Joint j: a map that is `heights[j]` at a_j = t* + d_j and 0 elsewhere, a prior that is 1 at [59 + d_j, 89 + d_j] and 0 elsewhere."""
    e, u = np.zeros((K, 120, 180)), np.zeros((K, H, W))
    for j in range(K):
        u[j, t_star[0] + d[j][0], t_star[1] + d[j][1]] = heights[j]
        e[j, 59 + d[j][0], 89 + d[j][1]] = 1.0
    return e, u


def _energy(e, u):
    return T.energy64(np.stack([T.corr_fft(e[j], u[j][None]) for j in range(K)], axis=1))[0]


def test_known_answer_by_hand():
    """a_j - d_j = t* for every joint: C_j(t*) = u_j(a_j), C_j = 0 elsewhere, so E peaks exactly at t* with E(t*) = sum log(u_j(a_j) + d)."""
    t_star, d = (22, 41), pose_ref.SKELETON
    heights = [0.5 + 0.1 * j for j in range(K)]
    e, u = _deltas(t_star, d, heights)
    for j in range(K):
        a_j = (t_star[0] + d[j][0], t_star[1] + d[j][1])
        assert pose_ref.prior_at(e[j], a_j, t_star) == 1.0      # the convention of DESIGN.md 4.13: [59 + (joint - torso)]
        for corr in (T.corr_fft, T.corr_windows):
            C = corr(e[j], u[j][None])[0]
            assert abs(C[t_star] - heights[j]) <= 1e-14 and np.abs(np.delete(C.reshape(-1), t_star[0] * W + t_star[1])).max() <= 1e-14
        assert T.corr_loops(e[j], u[j], (t_star[0],), (t_star[1],))[t_star] == heights[j]
    E = _energy(e, u)
    assert np.unravel_index(E.argmax(), E.shape) == t_star
    assert abs(E[t_star] - sum(np.log(h + T.DELTA) for h in heights)) <= 1e-12
    assert np.abs(np.delete(E.reshape(-1), t_star[0] * W + t_star[1]) - K * np.log(T.DELTA)).max() <= 1e-6


def test_sign_of_the_displacement():
    """One prior off by one cell moves nothing; five of nine shifted by (+1, 0) move the peak to t* - (1, 0): t = a - d, the sign of
    pose_ref.prior_at(e, cell_joint, cell_torso)."""
    t_star, d = (22, 41), [tuple(v) for v in pose_ref.SKELETON]
    _, u = _deltas(t_star, d, [1.0] * K)
    one = list(d)
    one[3] = (d[3][0] + 1, d[3][1])
    e1, _ = _deltas(t_star, one, [1.0] * K)
    E = _energy(e1, u)
    assert np.unravel_index(E.argmax(), E.shape) == t_star
    most = [(dy + 1, dx) if j < 5 else (dy, dx) for j, (dy, dx) in enumerate(d)]
    e5, _ = _deltas(t_star, most, [1.0] * K)
    E = _energy(e5, u)
    moved = (t_star[0] - 1, t_star[1])
    assert np.unravel_index(E.argmax(), E.shape) == moved
    for j in range(5):
        a_j = (t_star[0] + d[j][0], t_star[1] + d[j][1])
        assert pose_ref.prior_at(e5[j], a_j, moved) == 1.0 and pose_ref.prior_at(e5[j], a_j, t_star) == 0.0


def test_blob_values():
    """Interior cell and the corners (0,0), (59,89), (0,89): the values of data.BLOB, cut at the border; out-of-range cells are clamped first."""
    cells = np.array([(30, 40), (0, 0), (59, 89), (0, 89), (-5, 200), (60, 90)])
    got = T.blobs(cells)
    assert got.shape == (6, H, W, 1) and got.dtype == np.float32
    want = data.target_heat_maps(np.array([(30, 40), (0, 0), (59, 89), (0, 89), (0, 89), (59, 89)])[:, None, :])
    assert np.array_equal(got, want)
    b = np.outer([1, 2, 1], [1, 2, 1]).astype(np.float32) / 16
    assert np.array_equal(got[0, 29:32, 39:42, 0], b) and got[0].sum() == 1.0
    assert np.array_equal(got[1, :2, :2, 0], b[1:, 1:]) and got[1].sum() == np.float32(9 / 16)
    assert np.array_equal(got[2, 58:, 88:, 0], b[:2, :2]) and np.array_equal(got[3, :2, 88:, 0], b[1:, :2])


def test_planted_scenes():
    """pose_ref.scene(): the arg-max is person A's torso cell and the top-2 peaks of softmax(E) are A's and B's.  The sharp scene (trained-like
    priors and bn_sm): the local maxima of softmax(E) above 0 are the people and nothing else -- two for two people, one for one -- which is what
    forward(people=M)['people']['count'] counts.  The tie scene is equal to 1e-12, not exactly."""
    prob, params, ta, tb = T.scene()
    E = T.energy64(T.corr64(prob, params))
    cell, gap = T.argmax_cells(E)
    assert tuple(cell[0]) == ta and gap[0] > 1e-2
    assert T.top_peaks(T.softmax_map(E[0]), 2) == [ta, tb]
    for two in (True, False):
        prob, params, ta, tb = T.sharp_scene(two)
        E = T.energy64(T.corr64(prob, params))
        cell, gap = T.argmax_cells(E)
        assert tuple(cell[0]) == ta and gap[0] > 1.0
        assert T.top_peaks(T.softmax_map(E[0]).astype(np.float32), 4) == ([ta, tb] if two else [ta])
    prob, params, ta, tb = T.tie_scene()
    E = T.energy64(T.corr64(prob, params))[0]
    assert abs(E[ta] - E[tb]) <= 1e-12 and np.sort(E.reshape(-1))[-3] < E[ta] - 1e-2
    E = T.energy64(T.corr64(T.noise_prob(1, 5), T.flat_params()))
    assert E.max() - E.min() <= 1e-12


@pytest.mark.parametrize('B', sorted(T.NOISE_SEEDS))
def test_noise_seeds_meet_the_cap(B):
    """The seeds of the GPU test: the restatement's top-2 gap exceeds GAP_FLOOR (twice the energy bound) on at least 90 % of the images (the
    planted scenes and the corner-peak inputs are decided on every image: test_planted_scenes, test_corner_inputs_are_decided)."""
    E = T.energy64(T.corr64(T.noise_prob(B, T.NOISE_SEEDS[B]), T.trained_params()))
    _, gap = T.argmax_cells(E)
    assert T.GAP_FLOOR > 0 and (gap <= T.GAP_FLOOR).mean() <= 0.10


def test_corner_inputs_are_decided():
    cell, gap = T.argmax_cells(T.energy64(T.corr64(T.corner_prob(), T.corner_params())))
    assert cell.tolist() == [[0, 0], [0, W - 1], [H - 1, 0], [H - 1, W - 1]] and (gap > 30).all()
