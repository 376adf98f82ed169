"""GPU tests of the scoring back-end's kernels, one launch at a time, at every template instance and tile edge:
csrc/plda_kernels.hip (rankk_kernel, chunk_sum_kernel, segment_sum64_kernel, plda_transform_kernel<J>, plda_enroll_kernel,
plda_score_kernel) and the back-end part of csrc/kernels.hip (backend_gemm_kernel<RF>, backend_rowwise_kernel,
segment_mean_kernel), through scatter_stats, plda_transform, plda_score, backend_apply and segment_mean.

Equality wherever the inputs give every summation order the same bits (small integers, segment lengths that are powers of two);
elsewhere a bound per element, made of the reference's own terms and a count of the roundings the kernel performs, with the
count's derivation next to it.  The shapes sit on, below and above the tile constants, which are read from the sources: a
change of a constant moves the cases with it.  The inputs and their preconditions are checked without a GPU in
tests/test_backend_kernels_ref.py."""
import math
import os
import re

import numpy as np
import pytest

import helpers as H
import plda_ref as R

pytestmark = pytest.mark.gpu

_CSRC = os.path.join(H.ROOT, H.PKG_NAME, "csrc")
_PLDA = open(os.path.join(_CSRC, "plda_kernels.hip")).read() + open(os.path.join(_CSRC, "plda_kernels.h")).read()
_KERN = open(os.path.join(_CSRC, "kernels.hip")).read()


def _const(src, name):
    return int(re.search(r"\b%s = (\d+)\b" % name, src).group(1))


TILE = _const(_PLDA, "kTile")            # output tile of the rank-k products
KS = _const(_PLDA, "kKs")                # rows per LDS stage of the rank-k products
AHEAD = _const(_PLDA, "kSumAhead")       # rows a segment sum loads before it adds them
TR_ROWS = 4 * _const(_PLDA, "kTrRows")   # rows per workgroup of TransformIvector: 4 waves of kTrRows
MAX_DIM = _const(_PLDA, "kPldaMaxDim")
VB = _const(_KERN, "kBkVB")              # vectors per workgroup of the back-end GEMM
KT = _const(_KERN, "kBkKT")              # its K tile
MAX_RF = _const(_KERN, "kBkMaxRF")       # 16-row fragments of the largest instance: above 16 kBkMaxRF rows, the blocked path
CHUNK_CAP = int(re.search(r"if \(c > (\d+)\) c = \1;", _PLDA).group(1))                    # Chunking(): at most so many chunks,
CHUNK_ROWS = int(re.search(r"by_rows = \(n_rows \+ \d+\) / (\d+);", _PLDA).group(1))       # of at least so many rows
J_INSTANCES = sorted(set(int(j) for j in re.findall(r"hipLaunchKernelGGL\(plda_transform_kernel<(\d+)>", _PLDA)))
RF_INSTANCES = sorted(set(int(r) for r in re.findall(r"XV_LAUNCH\(backend_gemm_kernel<(\d+)>", _KERN)))
WAVE = 64                                # lanes of a gfx950 wavefront: a lane owns outputs lane + 64 j
U53 = 2.0 ** -53                         # the unit roundoff of float64
LD = np.longdouble


def _worst(err, bound):
    """largest error / bound over the elements whose bound is not 0 (where it is 0, the assertion asks for equality)"""
    err, bound = np.asarray(err, np.float64), np.asarray(bound, np.float64)
    return float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0


# ------------------------------------------------------------------------------------------------ scatter statistics
SCATTER_DIMS = [1, TILE - 1, TILE, TILE + 1, 2 * TILE - 1, 2 * TILE, 2 * TILE + 1, 200]
# listed rows: one, the LDS stage, one chunk against two (CHUNK_ROWS rows and one more), an odd count, three chunks
SCATTER_ROWS = [1, KS - 1, KS, KS + 1, CHUNK_ROWS - 1, CHUNK_ROWS, CHUNK_ROWS + 1, 97, 2 * CHUNK_ROWS + 2]
# rows at which Chunking()'s cap on the chunk count binds: one more than CHUNK_CAP chunks of CHUNK_ROWS rows (4100 for 64 x 64),
# and exactly CHUNK_CAP chunks of CHUNK_ROWS rows, the largest chunk count there is
SCATTER_CAP_ROWS = [CHUNK_CAP * CHUNK_ROWS + 4, CHUNK_CAP * CHUNK_ROWS]
# segment counts, for the fp64-row path (one row per segment): its stage and its first chunk edge
SCATTER_SEGS = [KS - 1, KS, KS + 1, CHUNK_ROWS, CHUNK_ROWS + 1]
POW2_LENGTHS = [0, 1, 2, 4, 8, 64, 128]
ODD_LENGTHS = [0, 1, 2, 3, 5, AHEAD - 1, AHEAD, AHEAD + 1, 2 * AHEAD + 1]


def _scatter_lengths(dims, cap_dim, allowed):
    """(dim, segment lengths) of every case of the two scatter tests"""
    for dim in dims:
        for total in SCATTER_ROWS + (SCATTER_CAP_ROWS if dim == cap_dim else []):
            rng = np.random.default_rng(7919 * dim + total)
            yield dim, R.ragged_lengths(rng, [a for a in allowed if a], total=total)
        for count in SCATTER_SEGS:
            rng = np.random.default_rng(104729 * dim + count)
            yield dim, R.ragged_lengths(rng, [a for a in allowed if a <= 8], count=count)     # short ones: the count is the point


def exact_scatter_cases():
    """(dim, x, segments): integer rows in [-8, 8], lengths that are powers of two, first and last segment empty"""
    for dim, lengths in _scatter_lengths(SCATTER_DIMS, TILE + 1, POW2_LENGTHS):
        rng = np.random.default_rng(dim + 31 * len(lengths) + sum(lengths))
        n_table = 3 if sum(lengths) < 2 else 37
        yield dim, R.integer_vectors(dim + sum(lengths), n_table, dim), R.segments_of_lengths(rng, lengths, n_table)
    yield TILE + 1, R.integer_vectors(1, 5, TILE + 1), []                                   # n_seg = 0
    yield TILE + 1, R.integer_vectors(2, 5, TILE + 1), [[], [], [], [], []]                 # every segment empty


def bounded_scatter_cases():
    """(dim, x, segments): random float32 rows, lengths around kSumAhead among many others"""
    a = AHEAD
    for dim, lengths in list(_scatter_lengths([TILE + 1, 2 * TILE + 1], TILE + 1, ODD_LENGTHS)) + \
            [(d, [2 * a + 1, 0, a - 1, a, 0, a + 1, 3, 5, 0, 0, 2 * a + 1, a]) for d in (TILE + 1, 2 * TILE + 1)]:
        rng = np.random.default_rng(3 * dim + 31 * len(lengths) + sum(lengths))
        x = (rng.standard_normal((211, dim)) * 2 + 0.5).astype(np.float32)
        yield dim, x, R.segments_of_lengths(rng, lengths, len(x))


def test_scatter_stats_of_integers_are_exact_at_every_tile_stage_and_chunk_edge():
    """rankk_kernel + chunk_sum_kernel on both row kinds and segment_sum64_kernel: integer rows and power-of-two segment
    lengths make every product, every sums / n and every partial sum of any order exact, so the three outputs have one set
    of bits and a wrong mask, a dropped stage, a lost chunk or a wrong mirror tile changes them."""
    P = H.pkg()
    seen_rows, seen_segs = set(), set()
    for dim, x, segs in exact_scatter_cases():
        r_tot, r_sums, r_bet, largest = R.scatter_stats_exact(x, segs)
        assert largest < 2 ** 53, "a precondition of the test's inputs: every absolute partial sum is below 2^53"
        s_tot, sums, s_bet = P.scatter_stats(x, segs)
        what = "dim %d, %d rows in %d segments" % (dim, sum(len(s) for s in segs), len(segs))
        assert sums.shape == r_sums.shape and np.array_equal(sums, r_sums), what
        assert np.array_equal(s_tot, r_tot), what
        assert np.array_equal(s_bet, r_bet), what
        assert np.array_equal(s_tot, s_tot.T) and np.array_equal(s_bet, s_bet.T), what
        if segs and not any(segs):
            assert not s_tot.any() and not s_bet.any() and not sums.any()
        seen_rows.add(sum(len(s) for s in segs))
        seen_segs.add(len(segs))
    assert seen_rows >= set(SCATTER_ROWS + SCATTER_CAP_ROWS + [0]) and seen_segs >= set(SCATTER_SEGS + [0])


def test_scatter_stats_of_random_rows_stay_within_elementwise_bounds():
    """sums: equal to the sequential float64 add loop in list order, for every segment of a ragged list.

    s_tot[i][j] = sum over the K listed rows of x_ri x_rj.  A product of two float32 is exact in float64, so an fma adds an exact
    term and rounds once.  A chunk with r rows of its own (the rows that pad its last stage are zeros and add exactly) rounds
    r - 1 times, the first fma adding to 0; chunk_sum_kernel then adds C partials with C - 1 roundings, its first add being to 0
    as well.  Every chunk holds a row, so r + C - 1 <= K, and a term meets at most K - 1 roundings:
    |error| <= ((1 + u)^(K - 1) - 1) sum |x_ri x_rj|.  (K + 2) u leaves three units for the terms of second order, for the
    rounding of the bound's own sum and for the longdouble reference (2^-11 u per operation).

    s_bet[i][j] = sum over the K segments of s_i (s_j / n): one rounding for the quotient, one per fma (the product is no longer
    exact, but the fma rounds product and sum at once), r of them in a chunk of r segments, and C - 1 in the chunk sum:
    1 + r + C - 1 <= K + 1 roundings, and (K + 4) u leaves the same three units.  Empty segments add exact zeros and still
    count in K.  The reference is formed from the device's own sums, which the first assertion has pinned."""
    P = H.pkg()
    worst_tot = worst_bet = 0.0
    for dim, x, segs in bounded_scatter_cases():
        what = "dim %d, %d rows in %d segments" % (dim, sum(len(s) for s in segs), len(segs))
        s_tot, sums, s_bet = P.scatter_stats(x, segs)
        assert np.array_equal(sums, R.sequential_sums(x, segs)), what
        rows = x[np.concatenate([np.asarray(s, np.int64) for s in segs])].astype(np.float64)
        ref = rows.astype(LD).T @ rows.astype(LD)
        bound = (len(rows) + 2) * U53 * (np.abs(rows).T @ np.abs(rows))
        err = np.abs(s_tot.astype(LD) - ref).astype(np.float64)
        worst_tot = max(worst_tot, _worst(err, bound))
        assert np.all(err <= bound), what
        n = np.array([len(s) for s in segs], np.float64)
        nz = n > 0
        ref = (sums[nz].astype(LD) / n[nz, None].astype(LD)).T @ sums[nz].astype(LD)
        bound = (len(segs) + 4) * U53 * ((np.abs(sums[nz]) / n[nz, None]).T @ np.abs(sums[nz]))
        err = np.abs(s_bet.astype(LD) - ref).astype(np.float64)
        worst_bet = max(worst_bet, _worst(err, bound))
        assert np.all(err <= bound), what
        assert np.array_equal(s_tot, s_tot.T) and np.array_equal(s_bet, s_bet.T), what
    print("rankk_kernel + chunk_sum_kernel: worst error / bound %.3g (s_tot), %.3g (s_bet)" % (worst_tot, worst_bet))


# ------------------------------------------------------------------------------------------------ TransformIvector
# every instance at its smallest and its largest dimension; the first one below its width as well; the last with whole lane
# groups masked (one group above the previous instance), one output in its last group, and one below the maximum
TRANSFORM_DIMS = sorted({1, WAVE - 1, MAX_DIM - 1, (J_INSTANCES[-2] + 1) * WAVE, (J_INSTANCES[-1] - 1) * WAVE + 1}
                        | {lo * WAVE + 1 for lo in [0] + J_INSTANCES[:-1]} | {j * WAVE for j in J_INSTANCES})
# one partial block (its masked rows read num = 1), the block edge, and a third block
TRANSFORM_ROWS = [1, TR_ROWS - 1, TR_ROWS, TR_ROWS + 1, 2 * TR_ROWS + 1]


def transform_instance(dim):
    """the J of the plda_transform_kernel instance that launch_plda_transform picks"""
    return min(j for j in J_INSTANCES if j * WAVE >= dim)


def transform_case(dim, n):
    """(x, T, offset, psi, num, y): integers, and the transformed vectors y = offset + T x in int64"""
    t, offset, psi = R.integer_plda_model(dim, dim)
    x = R.integer_vectors(1000 * dim + n, n, dim)
    num = np.array([(1.0, 3.0, 17.0)[(i + n) % 3] for i in range(n)])
    y = x.astype(np.int64) @ t.astype(np.int64).T + offset.astype(np.int64)
    return x, t, offset, psi, num, y


def test_transform_of_integers_is_exact_and_its_scale_within_a_few_roundings():
    """normalize=False: y = offset + T x is an integer below 2^24, whatever the order of the fma chain: equality.

    The scale is still returned.  With simple=False a lane owns J' terms y^2 / (psi + 1 / num); y^2 is exact, 1 / num, the sum and
    the quotient round once each: 3 roundings per term, each of relative size u because every quantity is positive.  The lane
    adds its terms with J' - 1 roundings (the first add is to 0), the xor tree has six levels, dim / ss rounds once and the
    square root once: (3 + J' - 1 + 6 + 1 + 1) u = (J' + 10) u, all over positive terms, so relative to the result.  The
    square root halves the 3 + J' - 1 + 6 + 1 units it is handed; the half not used is the room for the terms of second order
    and the longdouble reference.  With simple=True the sum of squares is exact and three roundings are left (two square
    roots and a quotient): the same bound holds with more room."""
    P = H.pkg()
    worst = {}
    for dim in TRANSFORM_DIMS:
        j = transform_instance(dim)
        for n in TRANSFORM_ROWS:
            x, t, offset, psi, num, y_int = transform_case(dim, n)
            assert np.abs(y_int).max() < 2 ** 24 and y_int.any(axis=1).all(), "a precondition of the test's inputs"
            for simple in (False, True):
                y, scale = P.plda_transform(x, t, offset, psi, num, normalize=False, simple=simple)
                assert y.dtype == np.float32 and np.array_equal(y, y_int), (dim, n, simple)
                ref = R.transform_ivector_ld(x, t, offset, psi, num, simple=simple)[1]
                rel = (np.abs(scale.astype(LD) - ref) / ref).astype(np.float64)
                worst[j] = max(worst.get(j, 0.0), float(rel.max()) / ((j + 10) * U53))
                assert np.all(rel <= (j + 10) * U53), (dim, n, simple, rel.max() / U53)
    print("plda_transform_kernel<J>: worst scale error / bound " + ", ".join("J=%d %.3g" % kv for kv in sorted(worst.items())))


def test_normalised_transform_is_within_one_float32_ulp_at_every_instance():
    """normalize=True, both kinds of normalisation: y scale is rounded to float32 once, so it is the rounded longdouble value
    or its neighbour"""
    P = H.pkg()
    differ = total = 0
    for dim in TRANSFORM_DIMS:
        for n in TRANSFORM_ROWS:
            x, t, offset, psi, num, _ = transform_case(dim, n)
            for simple in (False, True):
                y, scale = P.plda_transform(x, t, offset, psi, num, normalize=True, simple=simple)
                ry, rscale = R.transform_ivector_ld(x, t, offset, psi, num, simple=simple)
                want = (ry * rscale[:, None]).astype(np.float32)
                ulp = np.spacing(np.abs(want))
                assert np.all(np.abs(y.astype(np.float64) - want.astype(np.float64)) <= ulp), (dim, n, simple)
                differ += int((y != want).sum())
                total += y.size
    print("plda_transform_kernel<J>, normalised: %d of %d outputs are the neighbour of the rounded reference" % (differ, total))


def test_transform_refuses_a_dimension_above_the_largest_instance():
    P = H.pkg()
    x, t, offset, psi, num, _ = transform_case(MAX_DIM + 1, 1)
    with pytest.raises(P.XvError, match="dimension larger than %d" % MAX_DIM):
        P.plda_transform(x, t, offset, psi, num)


# ------------------------------------------------------------------------------------------------ LogLikelihoodRatio
SCORE_DIMS = [1, WAVE - 1, WAVE, WAVE + 1, 150, MAX_DIM]      # idle lanes, one full wave, a second pass, the recipe's, the largest
SCORE_N_U = [1, 3, 4, 5]                                      # plda_enroll_kernel: 4 rows per workgroup
SCORE_TRIALS = [1, 3, 4, 5, 257]                              # plda_score_kernel: 4 trials per workgroup
SCORE_N_V = 3


def score_units(dim):
    """k of the bound k u (A + B + C + D), with A = 1/2 sum |log(1 + psi)|, B = 1/2 sum |log var|, C = 1/2 sum (v - m)^2 / var and
    D = 1/2 sum v^2 / (1 + psi), for the inputs of R.scoring_case: psi is 0 or in [2, 6], num in [1, 3].  Where psi is 0, both
    logarithms, m and 1 / var are exact (0, 0, 0 and 1).  Elsewhere, in units of u and to first order:

    the tail that every term goes through: the lane's chain of J = ceil(dim / 64) adds or fmas, six tree levels, and the two
        operations of the final  const - s1 / 2 + s2 / 2:                                                            J + 8
    A:  1 + psi rounds once, which moves the logarithm by u, at most u / log 3 < 1 of itself; the device's log is allowed 2 ulp
        = 4 u (ROCm documents 1 ulp for the double-precision log; the doubling is margin); the difference of the two
        logarithms rounds once:                                                                         1 + 4 + 1 = 6
    B:  with q = psi / (n psi + 1) (two roundings below, one for the quotient), var = 1 + q carries 1 + 3 q / (1 + q) < 2.5
        (q < 6 / 7); the logarithm moves by that, at most 2.5 / log(1 + 2 / 7) < 10 of itself; 4 for the log, 1 for the
        difference:                                                                                    10 + 4 + 1 = 15
    C:  1 / var carries 3.5; df = v - m rounds once, so df^2 carries 2, and the product df df rounds once: 6.5.  m = n psi /
        (n psi + 1) u carries 5, which moves df by 5 u |m|, not by a multiple of df: the term moves by 5 u |m df| / var, and with
        |m| <= |v| + |df| and |v df| <= (v^2 + df^2) / 2 that is at most 5 u (3 df^2 / 2 + v^2 / 2) / var: 15 more on C, and
        5 (1 + psi) / var <= 5 * 7 * 19 / 25 < 27 on D:                                                    6.5 + 15 = 21.5
    D:  v^2 is exact, 1 / (1 + psi) rounds twice (on the host), and the 27 from above:                        2 + 27 = 29

    The largest is D's; one more unit covers the terms of second order and the longdouble reference: k = 29 + J + 8 + 1."""
    return 38 + math.ceil(dim / WAVE)


def _trials(rng, n_u, n_trials):
    tr = np.stack([rng.integers(0, n_u, n_trials), rng.integers(0, SCORE_N_V, n_trials)], 1)
    tr[:min(n_u, n_trials), 0] = np.arange(n_u)[::-1][:min(n_u, n_trials)]       # the last enrolment row first
    return tr


def test_llr_of_every_trial_is_within_a_bound_made_of_its_own_terms():
    P = H.pkg()
    worst = 0.0
    for dim in SCORE_DIMS:
        k = score_units(dim)
        for n_u in SCORE_N_U:
            u, num_u, v, psi = R.scoring_case(100 * dim + n_u, dim, n_u, SCORE_N_V)
            assert 1.0 in num_u and (n_u < 2 or 2.5 in num_u) and (dim == 1 or (psi == 0).any())
            assert np.all((psi == 0) | ((psi >= 2) & (psi <= 6))) and np.all((num_u >= 1) & (num_u <= 3)), \
                "the ranges that score_units() counts on"
            ref_all, size_all = R.llr_ld(u, num_u, v, psi)
            for n_trials in SCORE_TRIALS:
                tr = _trials(np.random.default_rng(dim + n_u + n_trials), n_u, n_trials)
                got = P.plda_score(u, num_u, v, psi, tr)
                ref, bound = ref_all[tr[:, 0], tr[:, 1]], k * U53 * size_all[tr[:, 0], tr[:, 1]].astype(np.float64)
                # the older test of this kernel allows 1e-9 (1 + |ref|): this bound is at least 1000 times tighter
                assert np.all(1000 * bound <= 1e-9 * (1 + np.abs(ref.astype(np.float64)))), (dim, n_u)
                err = np.abs(got.astype(LD) - ref).astype(np.float64)
                worst = max(worst, _worst(err, bound))
                assert np.all(err <= bound), (dim, n_u, n_trials, float((err / bound).max()))
    print("plda_enroll_kernel + plda_score_kernel: worst error / bound %.3g" % worst)


def test_llr_bits_do_not_depend_on_the_trial_order_and_no_trials_give_no_scores():
    P = H.pkg()
    u, num_u, v, psi = R.scoring_case(5, WAVE + 1, 5, SCORE_N_V)
    tr = _trials(np.random.default_rng(6), 5, SCORE_TRIALS[-1])
    got = P.plda_score(u, num_u, v, psi, tr)
    assert np.array_equal(P.plda_score(u, num_u, v, psi, tr[::-1])[::-1], got)
    perm = np.random.default_rng(7).permutation(len(tr))
    assert np.array_equal(P.plda_score(u, num_u, v, psi, tr[perm]), got[perm])
    none = P.plda_score(u, num_u, v, psi, np.zeros((0, 2), np.int32))                  # n_trials = 0, n_u > 0
    assert none.shape == (0,) and none.dtype == np.float64


# ------------------------------------------------------------------------------------------------ backend_apply
# every instance at its largest row count and one row above it (the next instance, or the blocked path), the smallest counts,
# one below the largest, and above it: one row, one whole fragment (vector stores at an offset) and two blocks and a bit
BACKEND_ROWS = sorted({1, 15, 16, 17, 16 * MAX_RF - 1, 16 * MAX_RF + 16, 2 * 16 * MAX_RF + 3}
                      | {16 * rf for rf in RF_INSTANCES} | {16 * rf + 1 for rf in RF_INSTANCES})
BACKEND_DIMS = [1, KT - 1, KT, KT + 1, 2 * KT + 1]
BACKEND_N = [1, 15, 16, 17, VB - 1, VB, VB + 1, 2 * VB + 1]


def backend_instance(rows):
    """the RF of the backend_gemm_kernel instance for a launch of so many rows"""
    return min(rf for rf in RF_INSTANCES if 16 * rf >= rows)


def backend_case(n, dim, rows, affine, with_mean=True):
    """(x, mean, T, y): x, mean and the linear part of T in {-1, 0, 1}, the affine column in [-3, 3], y = T (x - mean) (+ b) in
    int64.  Without the affine column a vector in the middle equals the mean: its y is the zero vector."""
    rng = np.random.default_rng(((n * 1009 + dim) * 1013 + rows) * 2 + affine)
    x = rng.integers(-1, 2, (n, dim)).astype(np.float32)
    mean = rng.integers(-1, 2, dim).astype(np.float32) if with_mean else None
    t = rng.integers(-1, 2, (rows, dim + 1)).astype(np.float32)
    t[:, dim] = rng.integers(-3, 4, rows)
    if not affine:
        t = np.ascontiguousarray(t[:, :dim])
        x[n // 2] = mean if with_mean else 0
    xc = x.astype(np.int64) - (mean.astype(np.int64) if with_mean else 0)
    y = xc @ t[:, :dim].astype(np.int64).T + (t[:, dim].astype(np.int64) if affine else 0)
    return x, mean, t, y


def backend_cases(affine):
    """(n, dim, rows): every row count with every dim, n going round its list; then every n with every dim at three row counts
    (one instance with vector stores, one with scalar stores, the blocked path)"""
    i = 0
    for rows in BACKEND_ROWS:
        for dim in BACKEND_DIMS:
            yield BACKEND_N[i % len(BACKEND_N)], dim, rows
            i += 1
    for rows in (16, 16 * RF_INSTANCES[2] + 1, 16 * MAX_RF + 1):
        for n in BACKEND_N:
            for dim in BACKEND_DIMS:
                yield n, dim, rows


def _ulps(got, want):
    """the largest |got - want| in units of the float32 spacing at want"""
    want = np.asarray(want, np.float32)
    return float((np.abs(got.astype(np.float64) - want) / np.spacing(np.abs(want))).max())


def _check_ratio(ratio, out, y_int, scaleup, normalized, what):
    """ss = |y|^2 is an integer below 2^24, exact in float32 in any order, so the ratio is sqrtf(ss) (/ sqrtf(rows)): compared
    with that float32 restatement to one float32 ulp and not for equality, because kernels.hip is not built with the flag that
    makes the device's divide and square root correctly rounded.  The normalised vector is y * (1 / ratio) of the device's own
    ratio, to one float32 ulp for the same reason; a zero vector comes back as zeros with ratio 0.  Returns the two distances
    in ulps."""
    ss = (y_int * y_int).sum(1)
    assert ss.max() < 2 ** 24, "a precondition of the test's inputs"
    want = np.sqrt(ss.astype(np.float32))
    if scaleup:
        want = want / np.sqrt(np.float32(y_int.shape[1]))
    assert want.dtype == np.float32
    ulps_ratio = _ulps(ratio, want)
    assert ulps_ratio <= 1, (what, scaleup)
    assert np.array_equal(ratio == 0, ss == 0), what
    if not normalized:
        return ulps_ratio, 0.0
    inv = np.divide(1.0, ratio.astype(np.float64), out=np.ones(len(ratio)), where=ratio != 0)
    ulps_out = _ulps(out, (y_int * inv[:, None]).astype(np.float32))
    assert ulps_out <= 1, (what, scaleup)
    assert not out[ss == 0].any(), what
    return ulps_ratio, ulps_out


@pytest.mark.parametrize("affine", [False, True])
def test_backend_apply_of_integers_at_every_instance_and_tile_edge(affine):
    """backend_gemm_kernel<RF> at every instance, both store epilogues, the K tile and the workgroup edge, and the blocked path
    above 16 kBkMaxRF rows with backend_rowwise_kernel behind it.  x, mean and T in {-1, 0, 1}: y is an integer, the same in any
    order of the MFMA accumulation: equality."""
    P = H.pkg()
    zeros, worst = 0, np.zeros(2)
    for i, (n, dim, rows) in enumerate(backend_cases(affine)):
        x, mean, t, y = backend_case(n, dim, rows, affine, with_mean=i % 3 != 2)
        what = "n %d, dim %d, rows %d" % (n, dim, rows)
        zeros += int((~y.any(axis=1)).sum())
        out, ratio = P.backend_apply(x, mean=mean, transform=t, normalize=False, return_ratio=True)
        assert out.dtype == np.float32 and out.shape == y.shape and np.array_equal(out, y), what
        worst = np.maximum(worst, _check_ratio(ratio, out, y, True, False, what))
        for scaleup in (True, False):
            out, ratio = P.backend_apply(x, mean=mean, transform=t, normalize=True, scaleup=scaleup, return_ratio=True)
            worst = np.maximum(worst, _check_ratio(ratio, out, y, scaleup, True, what))
    assert affine or zeros > 0
    print("backend_gemm_kernel<RF>: worst distance in float32 ulps %.3g (ratio), %.3g (normalised vector)" % tuple(worst))


def test_backend_rowwise_kernel_alone():
    """no transform: subtraction and normalisation, one wave per vector and four vectors per workgroup"""
    P = H.pkg()
    worst = np.zeros(2)
    for dim in (1, WAVE - 1, WAVE, WAVE + 1):
        for n in (1, 3, 4, 5):
            rng = np.random.default_rng(10 * dim + n)
            x = rng.integers(-1, 2, (n, dim)).astype(np.float32)
            mean = rng.integers(-1, 2, dim).astype(np.float32)
            x[n // 2] = mean
            y = x.astype(np.int64) - mean.astype(np.int64)
            assert np.array_equal(P.backend_apply(x, mean=mean), y)
            for scaleup in (True, False):
                out, ratio = P.backend_apply(x, mean=mean, normalize=True, scaleup=scaleup, return_ratio=True)
                worst = np.maximum(worst, _check_ratio(ratio, out, y, scaleup, True, "n %d, dim %d" % (n, dim)))
                assert not out[n // 2].any() and ratio[n // 2] == 0
    print("backend_rowwise_kernel: worst distance in float32 ulps %.3g (ratio), %.3g (normalised vector)" % tuple(worst))


@pytest.mark.parametrize("rows", [16 * RF_INSTANCES[2] + 1, 16 * MAX_RF + 16])
def test_a_vector_has_the_same_bits_alone_and_anywhere_in_a_batch(rows):
    """the GEMM path (one launch, and the blocked path with the row-wise pass behind it) on random float32 data"""
    P = H.pkg()
    rng = np.random.default_rng(rows)
    n, dim = VB + 1, KT + 1
    x = (rng.standard_normal((n, dim)) * 3).astype(np.float32)
    mean = rng.standard_normal(dim).astype(np.float32)
    t = (rng.standard_normal((rows, dim + 1)) / np.sqrt(dim)).astype(np.float32)
    batch, ratio = P.backend_apply(x, mean=mean, transform=t, normalize=True, return_ratio=True)
    for p in (0, 15, 16, VB - 1, VB):
        alone, r1 = P.backend_apply(x[p:p + 1], mean=mean, transform=t, normalize=True, return_ratio=True)
        assert np.array_equal(alone[0], batch[p]) and r1[0] == ratio[p], p


# ------------------------------------------------------------------------------------------------ segment_mean
def test_segment_mean_equals_the_sequential_loop_around_its_column_stride():
    """segment_mean_kernel strides the columns by its 256 threads: dims below, at and above that, both accumulators"""
    P = H.pkg()
    block = int(re.search(r"segment_mean_kernel<float>, dim3\(a\.n_seg\), dim3\((\d+)\)", _KERN).group(1))
    for dim in (1, block - 1, block, block + 1):
        rng = np.random.default_rng(dim)
        x = (rng.standard_normal((40, dim)) * 300).astype(np.float32)
        segs = R.segments_of_lengths(rng, [0, 1, 2, 7, 0, 64, 3, 0], len(x))
        for acc64 in (False, True):
            got = P.segment_mean(x, segs, acc64=acc64)
            for s, g in zip(segs, got):
                if not s:
                    assert not g.any()
                    continue
                if acc64:
                    acc = np.zeros(dim)
                    for i in s:
                        acc += x[i].astype(np.float64)
                    want = (acc * (1.0 / len(s))).astype(np.float32)
                else:
                    acc = x[s[0]].copy()
                    for i in s[1:]:
                        acc = (acc + x[i]).astype(np.float32)
                    want = acc * np.float32(1.0 / len(s))
                assert np.array_equal(g, want), (dim, acc64, len(s))
