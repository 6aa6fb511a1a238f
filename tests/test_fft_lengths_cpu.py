"""The case table of tests/test_gpu_fft_lengths.py, held to the source it restates and to the conditions it is generated for (no GPU)."""
import os
import re

import fft_lengths_ref as R

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'joint-cnn-mrf_amd', 'csrc')

# (kernel size, axis, length, kind) the route's size limit H + ks - 1 <= 192 excludes: a 9x9 layer stops at 184, so it neither fills the 192-point
# transform (188) nor reaches the odd size one short of it (187); the 5x5 layers run both
EXCLUDED = {(9, 'ny', 192, 'fill'), (9, 'ny', 192, 'odd'), (9, 'nx', 192, 'fill'), (9, 'nx', 192, 'odd')}


def _source(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def test_lengths_are_those_of_the_source():
    """A length added to or removed from kLens (csrc/conv_fft.hip) must show up here: the sweep is generated from the restated table."""
    m = re.search(r'static const int kLens\[\] = \{([0-9, ]+)\};', _source('conv_fft.hip'))
    assert m, 'the initialiser of kLens was not found in conv_fft.hip'
    assert tuple(int(v) for v in m.group(1).split(',')) == R.KLENS
    assert list(R.KLENS) == sorted(set(R.KLENS)) and all(n % 2 == 0 for n in R.KLENS)


def test_sizing_rule_is_that_of_the_source():
    """sizes_of's non-circular form: both kernel sizes, the limit, and the H + 4 / W + 4 padding."""
    src = _source('conv_fft.hip')
    assert 'return (ks == 9 || ks == 5) && H + ks - 1 <= 192 && W + ks - 1 <= 192 && pick(H + 4, &s->NY) && pick(W + 4, &s->NX);' in src
    assert R.sizes_of(60, 90, 9) == (64, 96) and R.sizes_of(64, 92, 9) == (72, 96) and R.sizes_of(120, 180, 5) == (128, 192)
    assert R.sizes_of(184, 16, 9) == (192, 20) and R.sizes_of(185, 16, 9) is None and R.sizes_of(16, 185, 9) is None
    assert R.sizes_of(188, 188, 5) == (192, 192) and R.sizes_of(189, 16, 5) is None and R.sizes_of(16, 16, 7) is None


def test_register_kernel_lengths_are_those_of_the_launchers():
    """REG_NY / REG_NX (where fft_reg = 0 selects another kernel) against the launchers of conv_fft_reg_inv.hip."""
    src = _source('conv_fft_reg_inv.hip')
    cols = src[src.index('bool cfft_cols_inv_reg('):src.index('static bool launch_rows_inv_reg')]
    assert tuple(sorted(int(v) for v in re.findall(r'case (\d+): CI_LAUNCH', cols))) == R.REG_NY
    rows = src[src.index('bool cfft_rows_inv_reg('):]
    assert tuple(sorted(int(v) for v in re.findall(r'if \(NX == (\d+)', rows))) == R.REG_NX


def test_swept_sizes():
    assert R.swept_sizes(20, 9) == [16, 15, 5] and R.swept_sizes(24, 5) == [20, 19, 17] and R.swept_sizes(128, 9) == [124, 123, 97]
    assert R.swept_sizes(192, 5) == [188, 187, 125] and R.swept_sizes(192, 9) == [184, 125]
    for ks in R.KERNEL_SIZES:
        for n in R.KLENS:
            for s in R.swept_sizes(n, ks):
                assert R.pick(s + R.PAD) == n and R.allowed(s, ks)


def test_cases_cover_every_length_on_both_axes():
    cs = R.cases()
    print('%d cases (%d with 9x9 filters)' % (len(cs), sum(c.ks == 9 for c in cs)))
    assert len(cs) < 250
    assert len(set(cs)) == len(cs) and len(set(R.case_id(c) for c in cs)) == len(cs)
    for c in cs:
        assert R.sizes_of(c.H, c.W, c.ks) is not None, c
        assert max(c.H, c.W) <= 188 and c.cin % 64 == 0
        assert c.B == (3 if c.kind == 'fill' and c.H * c.W < 20000 else 1), c
    for ks in R.KERNEL_SIZES:
        for axis, idx in (('ny', 0), ('nx', 1)):
            for n in R.KLENS:
                # the swept axis alone, so that a length is not 'covered' by the 20-point transform of the other axis (16 x 16 belongs to both sweeps)
                mine = [c for c in cs if c.ks == ks and R.sizes_of(c.H, c.W, ks)[idx] == n and (c.set == axis or (c.H, c.W) == (R.SMALL, R.SMALL))]
                assert mine, (ks, axis, n)
                sizes = [(c.H, c.W)[idx] for c in mine]
                for kind, size in (('fill', n - R.PAD), ('odd', n - R.PAD - 1)):
                    assert (size in sizes) != ((ks, axis, n, kind) in EXCLUDED), (ks, axis, n, kind)
                assert (n - R.PAD) % 2 == 0 and (n - R.PAD - 1) % 2 == 1
                assert max(sizes) == R.largest_allowed(n, ks)
                assert min(sizes) == (R.prev_len(n) - R.PAD + 1 if R.prev_len(n) else 5)      # the first map that needs n: the most zero padding
    # every excluded combination is one the limit refuses
    for ks, axis, n, kind in EXCLUDED:
        assert not R.allowed(n - R.PAD - (kind == 'odd'), ks)
    # the filling cases carry the odd batch
    assert all(c.B == 3 for c in cs if c.set in ('ny', 'nx') and c.kind == 'fill')


def test_diagonal_and_tail_sets():
    diag = R.diag_cases()
    assert [R.sizes_of(c.H, c.W, c.ks) for c in diag] == [(20, 24), (36, 40), (60, 64), (72, 100), (128, 192)]
    assert all(c.ks == 5 and c.H + R.PAD == R.sizes_of(c.H, c.W, 5)[0] and c.W + R.PAD == R.sizes_of(c.H, c.W, 5)[1] for c in diag)
    assert [c.B for c in diag] == [3, 3, 3, 3, 1]
    tail = R.tail_cases()
    assert sorted(set((R.sizes_of(c.H, c.W, c.ks)[0], c.cout) for c in tail)) == [(64, 9), (64, 72), (64, 136), (128, 9), (128, 72), (128, 136)]
    assert all(c.cin == 128 and c.W == R.SMALL and c.H + R.PAD == c.n and c.B == 3 for c in tail)
    # which cases the fft_reg = 0 arm runs on other kernels: every NX-sweep case has 20-point columns (a register kernel), the NY sweep only at REG_NY
    assert all(R.has_register_kernel(c) for c in R.cases() if c.set == 'nx')
    assert sorted(set(c.n for c in R.cases() if c.set == 'ny' and R.has_register_kernel(c))) == sorted(R.REG_NY)
    assert [R.has_register_kernel(c) for c in tail] == [True, True, True, False, False, False]
