"""GPU tests of the exact top-N statistics kernel (csrc/plda_dense_kernels.hip topn_stats_kernel) through xv_topn_stats, on
crafted rows.  Rows of integers (or of whole multiples of the smallest denormal) with N a power of two make every sum exact in
every order: the mean must then be the reference's bits and the standard deviation within one rounding of the square root,
which checks the SELECTION whatever the order of the sums.  Random rows check the sums against the long-double reference."""
import os
import re

import numpy as np
import pytest

import asnorm_ref as A
import helpers as H

pytestmark = pytest.mark.gpu

_HDR = open(os.path.join(H.ROOT, H.PKG_NAME, "csrc", "plda_dense_kernels.h")).read()
_MAX = re.search(r"\bkTopnMaxCols = (\d+) << (\d+);", _HDR)
MAX_COLS = int(_MAX.group(1)) << int(_MAX.group(2))
U53 = 2.0 ** -53
LD = np.longdouble
COLS = [2, 63, 64, 65, 255, 256, 257]       # around one wave's stride and around the four waves' first full round


def _ns(c):
    """N: 2, C - 1, C and every power of two up to C"""
    return sorted({n for n in [2, c - 1, c] + [1 << k for k in range(1, 12)] if 2 <= n <= c})


def _pow2(n):
    return n & (n - 1) == 0


def _check_exact(P, rows, n, what):
    """rows: integers small enough for every sum of every order to be exact when n is a power of two"""
    rows = np.atleast_2d(np.asarray(rows, np.float64))
    mean, std = P.asnorm.topn_stats(rows, n)
    rm, rs, _ = A.topn_stats(rows, n)
    if _pow2(n):
        rm64, rs64 = rm.astype(np.float64), rs.astype(np.float64)
        assert np.all(rm64.astype(LD) == rm), "the reference mean is a float64"
        assert np.array_equal(mean, rm64) and not np.signbit(mean[mean == 0]).any(), (what, n, mean, rm64)
        assert np.all(np.abs(std - rs64) <= np.spacing(rs64)), (what, n, std, rs64)
    else:
        _check_bounds(rows, n, mean, std, what)


def _check_bounds(rows, n, mean, std, what):
    """The mean: a sum of n terms in some order and a division, (n - 1) + 1 roundings of at most u sum |x| each, within the
    (n + 1) u sum |x| asked of it (sum |x| over the selected values).
    The deviation, two-pass: with dm the mean's error, sum (x - mean')^2 = sum (x - mean)^2 + n dm^2, so the computed root is
    sqrt(sigma^2 (1 + e) + dm^2) with e from the subtraction (2, squared), the n multiply-adds (n + 1), the division and the
    root (1 + 1): |sigma' - sigma| <= (n / 2 + 3) u sigma + dm, dm <= (n + 1) u sum |x| / n; one more unit on sigma for the
    second order and the reference."""
    rm, rs, mag = A.topn_stats(rows, n)
    bm = (n + 1) * U53 * mag
    bs = (n / 2 + 4) * U53 * rs + (n + 1) * U53 * mag / n
    em, es = np.abs(mean.astype(LD) - rm), np.abs(std.astype(LD) - rs)
    assert np.all(em <= bm) and np.all(es <= bs), (what, n, float((em / np.maximum(bm, LD(1e-300))).max()),
                                                    float((es / np.maximum(bs, LD(1e-300))).max()))
    return float((em[bm > 0] / bm[bm > 0]).max(initial=0)), float((es[bs > 0] / bs[bs > 0]).max(initial=0))


def _crafted(c, rng):
    """name -> row of c integers"""
    rows = {
        "all equal": np.full(c, 7.0),
        "ascending": np.arange(c, dtype=np.float64) - c // 2,
        "descending": c // 3 - np.arange(c, dtype=np.float64),
        "random": rng.integers(-1000, 1001, c).astype(np.float64),
        "few values": rng.integers(-2, 3, c).astype(np.float64),            # ties everywhere, whatever N is
    }
    signs = rng.integers(-3, 4, c).astype(np.float64)
    signs[rng.random(c) < 0.3] = -0.0
    signs[rng.random(c) < 0.2] = 0.0
    rows["mixed signs and both zeros"] = signs
    rows["negative zeros only"] = np.full(c, -0.0)
    return rows


@pytest.mark.parametrize("c", COLS)
def test_crafted_integer_rows_select_exactly(c):
    P = H.pkg()
    rng = np.random.default_rng(c)
    for name, row in _crafted(c, rng).items():
        for n in _ns(c):
            _check_exact(P, row, n, (name, c))


def test_ties_that_straddle_the_nth_place():
    """The n-th largest value is held by several columns, some of which are taken: the values decide the statistics, so every
    count of ties taken is checked through them; the columns taken are the lowest by the rule, which no statistic can see
    (equal values are equal), so that half of the rule is the restatement's."""
    P = H.pkg()
    for c in (65, 257):
        for n_above in (0, 1, 3):
            for n_ties in (2, 5, c - 8):
                row = np.full(c, -50.0)
                idx = np.random.default_rng(c + n_above + n_ties).permutation(c)
                row[idx[:n_above]] = 90.0 + np.arange(n_above)
                row[idx[n_above:n_above + n_ties]] = 10.0
                for n in sorted({2, 4, 8} | {n_above + 1, n_above + n_ties - 1, n_above + n_ties, n_above + n_ties + 1}):
                    if 2 <= n <= c:
                        _check_exact(P, row, n, ("ties", c, n_above, n_ties))


def test_denormals_and_neighbours_in_the_last_mantissa_bit():
    P = H.pkg()
    tiny = np.float64(5e-324)
    rng = np.random.default_rng(4)
    # whole multiples of 256 denormal units: sums and the division by N <= 256 are exact; the squares underflow, so the
    # deviation is 0 where the reference's is of the order of the values: within sqrt of the underflow threshold, 2^-537
    row = (rng.integers(-40, 41, 300) * 256).astype(np.float64) * tiny
    assert np.all(np.abs(row) < 2.3e-308) and (row != 0).any()
    for n in (2, 64, 256):
        mean, std = P.asnorm.topn_stats(row[None], n)
        rm, rs, _ = A.topn_stats(row[None], n)
        assert mean[0] == np.float64(rm[0]) and np.float64(rm[0]).astype(LD) == rm[0] and abs(std[0] - np.float64(rs[0])) <= 2.0 ** -537
    # 1 + k 2^-52, k odd: the sum of the largest two is exact and names them (7 and 5 -> 1 + 6 2^-52; any other pair differs)
    for c in (64, 257):
        row = np.full(c, 1.0 - 2.0 ** -53)
        at = rng.permutation(c)[:4]
        row[at] = 1.0 + np.array([7, 5, 3, 1]) * 2.0 ** -52
        mean, std = P.asnorm.topn_stats(row[None], 2)
        assert mean[0] == 1.0 + 6 * 2.0 ** -52 and std[0] == 2.0 ** -52
        row[at[0]] = -(1.0 + 7 * 2.0 ** -52)                       # the same bits with the sign set are the smallest
        mean, std = P.asnorm.topn_stats(row[None], 2)
        assert mean[0] == 1.0 + 4 * 2.0 ** -52 and std[0] == 2.0 ** -52


def test_the_largest_row_and_the_sizes_beyond_the_limits():
    P = H.pkg()
    row = np.random.default_rng(9).integers(-1000, 1001, MAX_COLS).astype(np.float64)
    for n in (2, 1024):
        _check_exact(P, row, n, "the widest row")
    L = P.lib()
    out = np.zeros(2)
    args = lambda cols, n: (0, row.ctypes.data, 1, cols, n, out[:1].ctypes.data, out[1:].ctypes.data, None)   # noqa: E731
    assert L.xv_topn_stats(*args(MAX_COLS + 1, 2)) == P.XV_ERR_ARG and b"kTopnMaxCols" in L.xv_last_error()
    assert L.xv_topn_stats(*args(100, 1)) == P.XV_ERR_ARG and L.xv_topn_stats(*args(100, 101)) == P.XV_ERR_ARG
    assert L.xv_topn_stats(*args(100, 100)) == P.XV_OK and out[0] == row[:100].mean()


@pytest.mark.parametrize("c", [2, 65, 257, 3000, 16384])
def test_random_rows_are_within_the_bounds_of_the_sums(c):
    P = H.pkg()
    rng = np.random.default_rng(c)
    rows = rng.standard_normal((6, c)) * np.array([1e-3, 1.0, 1.0, 50.0, 1e6, 1.0])[:, None] + np.array([0, 0, 30, -400, 0, 1e9])[:, None]
    worst = (0.0, 0.0)
    for n in sorted({2, min(c, 300), c - 1, c} - {0, 1}):
        mean, std = P.asnorm.topn_stats(rows, n)
        w = _check_bounds(rows, n, mean, std, c)
        worst = (max(worst[0], w[0]), max(worst[1], w[1]))
    print("topn_stats_kernel, %d columns: worst error / bound: mean %.3g, deviation %.3g" % (c, worst[0], worst[1]))


def test_a_row_gives_the_same_bits_alone_and_anywhere_in_a_batch():
    P = H.pkg()
    rng = np.random.default_rng(33)
    for c, n in ((257, 100), (1000, 300)):
        row = rng.standard_normal(c) * 40
        alone = P.asnorm.topn_stats(row[None], n)
        for pos in (0, 1, 16, 31, 32):
            batch = rng.standard_normal((33, c)) * 40
            batch[pos] = row
            mean, std = P.asnorm.topn_stats(batch, n)
            assert mean[pos] == alone[0][0] and std[pos] == alone[1][0]
