"""What test_gpu_front_end.py takes for granted, checked without a GPU: every row of its shape table has the property its reason claims (the
launchers' formulas of csrc/conv1_mfma.hip, restated in front_end_ref.conv1_geometry), the float64 reference agrees with an independent one, and
the kernel-name rule of jcm_conv_kernel_name for the Cin == 3 layers is the tower's size condition."""
import numpy as np
import pytest

import joint_cnn_mrf_amd  # noqa: F401
import front_end_ref as R


def test_every_table_row_has_the_property_its_reason_claims():
    rows = {r['hw']: r for r in R.SHAPES}
    assert len(rows) == len(R.SHAPES) == 9
    for r in R.SHAPES:
        H, W = r['hw']
        assert r['fused'] == R.fused_name_rule(H, W)
        assert r['pooled'] == (-(-(-(-H // 2)) // 2), -(-(-(-W // 2)) // 2))      # ceil(ceil(n / 2) / 2)
        if r['fused']:
            g = R.conv1_geometry(H, W)
            assert (g['patches'], g['last'], g['pooled']) == (r['patches'], r['last'], r['pooled'])
            assert g['pad'] == (1, 1)      # SAME, stride 2, even extent: 3 padded cells, 1 before and 2 after
    g = {hw: R.conv1_geometry(*hw) for hw in rows if rows[hw]['fused']}
    assert g[(4, 4)]['conv'] == (2, 2) and g[(4, 4)]['pooled'] == (1, 1) and g[(4, 4)]['patches'] == (1, 1)
    assert g[(8, 36)]['patches'] == (1, 2) and g[(8, 36)]['last'][1] == 2 and g[(8, 36)]['pooled'][1] - R.PATCH // 2 == 1      # one pooled column in patch 2
    assert g[(36, 32)]['patches'] == (2, 1) and g[(36, 32)]['last'][0] == 2 and g[(36, 32)]['pooled'][0] - R.PATCH // 2 == 1     # one pooled row in patch 2
    assert g[(32, 32)]['patches'] == (1, 1) and g[(32, 32)]['last'] == (R.PATCH, R.PATCH)
    assert g[(64, 96)]['patches'] == (2, 3) and g[(64, 96)]['last'] == (R.PATCH, R.PATCH)
    assert g[(60, 92)]['patches'] == (2, 3) and g[(60, 92)]['last'] == (14, 14)
    assert min(g[(120, 184)]['patches']) >= 3      # a patch with a neighbour on every side
    # the generic rows: SAME padding of a stride-2 5x5 window is asymmetric on an even extent, symmetric on an odd one
    from oracle import jcm_oracle as O
    assert O.same_padding(30, 5, 2) == (15, 1, 2) and O.same_padding(44, 5, 2) == (22, 1, 2) and O.same_padding(45, 5, 2) == (23, 2, 2)
    assert O.same_padding(15, 2, 2) == (8, 0, 1) and O.same_padding(23, 2, 2) == (12, 0, 1) and O.same_padding(22, 2, 2) == (11, 0, 0)
    for sub in R.SUBS:      # the image extents of every case are multiples of sub: the tower sub-samples such an image, it does not resize it
        for r in R.SHAPES:
            assert R.tower_takes_fused(sub * r['hw'][0], sub * r['hw'][1], sub) == r['fused']


def test_the_persistent_case_cannot_be_resident_at_once():
    c = R.PERSISTENT
    g = R.conv1_geometry(*c['hw'])
    ntiles = c['B'] * g['patches'][0] * g['patches'][1]
    assert g['patches'] == (4, 4) and ntiles == 2560 > c['resident_max'] == 2048
    assert c['B'] <= 65535      # conv1_mfma_pool_f32_kernel puts the image index on blockIdx.y
    assert max(c['compare']) == c['B'] - 1 and min(c['compare']) == 0


@pytest.mark.parametrize('row', R.SHAPES, ids=lambda r: '%dx%d' % r['hw'])
def test_reference_equals_an_independent_one(row):
    H, W = row['hw']
    p = R.front_end_params()
    x = np.random.RandomState(H * 1000 + W).standard_normal((1, H, W, 3))
    ref = R.conv1_pool_ref(x, p, 'conv1_fullres')
    other = R.conv1_pool_torch(x, p, 'conv1_fullres')
    assert ref.shape == other.shape == (1,) + row['pooled'] + (64,)
    assert np.abs(ref - other).max() <= 1e-12 * np.abs(ref).max()
    # ... and sub-sampling is plain striding
    x2 = np.random.RandomState(7).standard_normal((1, 2 * H, 2 * W, 3))
    assert np.array_equal(R.conv1_pool_ref(x2, p, 'conv1_halfres', sub=2), R.conv1_pool_ref(x2[:, ::2, ::2], p, 'conv1_halfres'))


def test_kernel_name_rule_is_the_towers_size_condition():
    for H in range(1, 65):
        for W in range(1, 65):
            for sub in R.SUBS:
                assert R.fused_name_rule(H, W) == R.tower_takes_fused(sub * H, sub * W, sub), (H, W, sub)
    assert not R.fused_name_rule(30, 44) and not R.fused_name_rule(30, 45) and R.fused_name_rule(32, 44)
