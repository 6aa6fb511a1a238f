"""The transform-length table of the frequency-domain convolution (csrc/conv_fft.hip: kLens, pick, sizes_of without the overlap-save windows),
restated in plain Python, and the layer shapes that walk it: every length as the column length NY and as the row length NX, for both kernel
sizes, at the map sizes where a length can go wrong -- the map that fills its transform, the odd map one short of it, and the first map that
needs the length.  No GPU, no torch: tests/test_fft_lengths_cpu.py holds the table to the source and the cases to their conditions,
tests/test_gpu_fft_lengths.py runs them against float64."""
from collections import namedtuple

KLENS = (20, 24, 28, 32, 36, 40, 50, 60, 64, 72, 96, 100, 128, 192)
PAD = 4             # the circular convolution is H + 4 rows by W + 4 columns for both kernel sizes
LIMIT = 192         # H + ks - 1 <= 192, W + ks - 1 <= 192
KERNEL_SIZES = (5, 9)
SMALL = 16          # the axis that is not swept: a 20-point transform

# lengths whose inverse pass exists as a register kernel besides the LDS one (conv_fft_reg_inv.hip: cfft_cols_inv_reg, cfft_rows_inv_reg); the
# row kernels store channel pairs (even Cout), the 32-point one writes fp32 only; columns with 32-channel blocks (NY > 100) stay on the LDS kernel
REG_NY = (20, 32, 36, 64)
REG_NX = (28, 32, 50, 96)


def pick(need):
    return next((v for v in KLENS if v >= need), None)


def allowed(size, ks):
    return size + ks - 1 <= LIMIT


def sizes_of(H, W, ks):
    """(NY, NX) of an H x W map, or None where the route refuses it."""
    if ks not in KERNEL_SIZES or not allowed(H, ks) or not allowed(W, ks):
        return None
    ny, nx = pick(H + PAD), pick(W + PAD)
    return None if ny is None or nx is None else (ny, nx)


def prev_len(n):
    i = KLENS.index(n)
    return KLENS[i - 1] if i else None


def largest_allowed(n, ks):
    """The largest map size of length n that the size limit lets through."""
    return min(n - PAD, LIMIT - ks + 1)


def kind_of(size, n):
    """fill: the map fills the transform; odd: one short of it (an unpaired last row / an odd last column); pad: anything smaller."""
    return 'fill' if size + PAD == n else 'odd' if size + PAD + 1 == n else 'pad'


def swept_sizes(n, ks):
    """Sizes on the swept axis for length n: n - 4, n - 5, and the first size that needs n (5 for the shortest length); a size the limit refuses
    becomes the largest allowed size of that length; duplicates dropped."""
    first = prev_len(n) - PAD + 1 if prev_len(n) else 5
    out = []
    for s in (n - PAD, n - PAD - 1, first):
        if not allowed(s, ks):
            s = largest_allowed(n, ks)
        if s not in out:
            out.append(s)
    return out


# set: 'ny' / 'nx' (the sweeps), 'diag' (both axes fill), 'tail' (channel tails); n: the length the case is for (diag: NY); kind: of the swept axis
Case = namedtuple('Case', 'set n kind B H W cin cout ks')


def case_id(c):
    return '%s%d_%s_B%d_%dx%d_%d-%d_k%d' % (c.set, c.n, c.kind, c.B, c.H, c.W, c.cin, c.cout, c.ks)


def sweep_cases():
    out, seen = [], set()
    for ks in KERNEL_SIZES:
        for axis in ('ny', 'nx'):
            for n in KLENS:
                for s in swept_sizes(n, ks):
                    kind = kind_of(s, n)
                    H, W = (s, SMALL) if axis == 'ny' else (SMALL, s)
                    if (H, W, ks) in seen:      # 16 x 16 belongs to both sweeps
                        continue
                    seen.add((H, W, ks))
                    out.append(Case(axis, n, kind, 3 if kind == 'fill' else 1, H, W, 64, 64, ks))
    return out


def diag_cases():
    """Both axes fill at once (5x5: the only kernel size that fills 192)."""
    return [Case('diag', H + PAD, 'fill', B, H, W, 64, 64, 5) for B, H, W in ((3, 16, 20), (3, 32, 36), (3, 56, 60), (3, 68, 96), (1, 124, 188))]


def tail_cases():
    """Channel tails at NY = 64 (register inverse columns) and NY = 128 (LDS inverse columns on 32-channel blocks), the map filling in y: Cout 9 / 72 / 136
    leave pad64(Cout) - Cout = 55 / 56 / 56 channels that no map holds; Cin 128 is two 64-channel blocks."""
    return [Case('tail', n, 'fill', 3, n - PAD, SMALL, 128, cout, 9) for n in (64, 128) for cout in (9, 72, 136)]


def cases():
    return sweep_cases() + diag_cases() + tail_cases()


def has_register_kernel(c):
    """Does fft_reg = 1 select a register kernel somewhere in this layer of an fp32 handle?  (Where it does not, fft_reg = 0 runs the very same kernels.)"""
    ny, nx = sizes_of(c.H, c.W, c.ks)
    return ny in REG_NY or (nx in REG_NX and c.cout % 2 == 0)
