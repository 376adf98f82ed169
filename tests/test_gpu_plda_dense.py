"""GPU tests of the dense PLDA scoring kernels (csrc/plda_dense_kernels.hip: plda_dense_enroll_kernel, plda_dense_test_kernel,
plda_dense_gemm_kernel) through xv_plda_score_dense and xv_plda_cohort_stats: every element against the long-double ratio
within a bound made of its own terms, at the dimension and tile edges; position independence bit for bit; agreement with the
per-trial kernel."""
import math
import os
import re

import numpy as np
import pytest

import asnorm_ref as A
import helpers as H
import plda_ref as R
from test_gpu_backend_kernels import score_units

pytestmark = pytest.mark.gpu

_HDR = open(os.path.join(H.ROOT, H.PKG_NAME, "csrc", "plda_dense_kernels.h")).read()
_PLDA = open(os.path.join(H.ROOT, H.PKG_NAME, "csrc", "plda_kernels.h")).read()


def _const(src, name):
    return int(re.search(r"\b%s = (\d+)\b" % name, src).group(1))


TILE_M, TILE_N = _const(_HDR, "kDenseTileM"), _const(_HDR, "kDenseTileN")
MAX_DIM = _const(_PLDA, "kPldaMaxDim")
U53 = 2.0 ** -53
LD = np.longdouble
DIMS = [1, 2, 3, 5, 64, 150, 200, 511, 512]
NUMS = (1.0, 2.0, 7.5)


def dense_units(dim):
    """k of the bound k u (sum |A1 v| + sum |A2 v^2| + R), R = 1/2 sum |log(1 + psi)| + 1/2 sum |log var| + 1/2 sum m^2 / var (r
    term by term: its error is a multiple of its terms, which cancel in r itself), for psi 0 or in [2, 6] and num in [1, 7.5].
    The size is made of the EXPANDED terms: where v is close to m they are large and cancel, and (v - m)^2 / var says nothing
    about the roundings they went through.  Where psi is 0 every term is exact (m = 0, var = 1, A1 = A2 = 0, both logarithms 0).
    Elsewhere, in units of u = 2^-53 and to first order:

    preparation
      n psi + 1 carries 2; g = n psi / (n psi + 1): 1 + 1 + 2 = 4; m = g u: 5
      q = psi / (n psi + 1): 3; var = 1 + q: 3 q / (1 + q) + 1 < 2.5 (q < 6 / 7); 1 / var: 3.5
      A1 = m / var: 5 + 3.5 + 1 = 9.5
      A2 = (1 / (1 + psi) - 1 / var) / 2: the first quotient carries 2 (host), the second 3.5, the difference rounds once; of the
        difference itself, 1 / (1 + psi) is at most (1 / psi + 1 / (n psi) + 1 / (n psi^2)) <= 1.25 and 1 / var at most
        (1 + 1 / psi)(1 + 1 / (n psi)) <= 2.25 times:                                       2 * 1.25 + 3.5 * 2.25 + 1 < 11.5
      v and v^2 are exact (fp32 values)
    the product: one chain of 2 dim multiply-adds (the padding adds exact zeros), a product and a sum each, counted as
      separately rounded in case the matrix core does not fuse them:                                          2 dim + 1
    the addend r, relative to R: log(1 + psi) as in score_units (6); log var moves by 2.5 / log(var) of itself, and var >= 1.125
      (n <= 7.5, psi >= 2), so by less than 22, plus 4 for the device's logarithm and 1 for the difference: 27; m^2 / var as
      m A1 carries 14.5; each sum is a lane's chain of J = ceil(dim / 64) and six tree levels, and r = lg / 2 - q / 2 rounds at
      most twice:                                                                                         27 + J + 8
    the final addition of r rounds once, on everything:                                                               1

    The three groups of terms carry 9.5 + 2 dim + 2, 11.5 + 2 dim + 2 and 36 + J; one more unit covers the second order and the
    reference:  k = max(2 dim + 14.5, 37 + J)."""
    return max(2 * dim + 14.5, 37 + math.ceil(dim / 64))


def _case(seed, dim, n_u, n_v):
    u, _, v, psi = R.scoring_case(seed, dim, n_u, n_v)
    num_u = np.array([NUMS[(k + seed) % 3] for k in range(n_u)])
    assert np.all((psi == 0) | ((psi >= 2) & (psi <= 6))) and num_u.min() >= 1 and num_u.max() <= 7.5, "the ranges dense_units() counts on"
    return u, num_u, v, psi


def _check(P, u, num_u, v, psi, what):
    got = P.asnorm.plda_score_dense(u, num_u, v, psi)
    ref = A.dense_llr(u, num_u, v, psi)[0]
    bound = (dense_units(u.shape[1]) * U53 * A.expanded_size(u, num_u, v, psi)).astype(np.float64)
    err = np.abs(got.astype(LD) - ref).astype(np.float64)
    assert got.shape == (len(u), len(v)) and np.all(err <= bound), (what, float((err / bound).max()))
    return float((err / bound).max())


@pytest.mark.parametrize("dim", DIMS)
def test_every_score_is_within_a_bound_made_of_its_expanded_terms(dim):
    P = H.pkg()
    worst = 0.0
    for n_u in (1, 15, 16, 17):
        for n_v in (1, 15, 16, 17):
            u, num_u, v, psi = _case(1000 * dim + 20 * n_u + n_v, dim, n_u, n_v)
            assert n_u < 3 or set(num_u) == set(NUMS)
            worst = max(worst, _check(P, u, num_u, v, psi, (dim, n_u, n_v)))
    print("plda_dense kernels, dim %d: worst error / bound %.3g" % (dim, worst))


@pytest.mark.parametrize("dim", [5, 150])
def test_the_workgroup_tile_edges_in_both_directions(dim):
    P = H.pkg()
    worst = 0.0
    for n_u, n_v in [(TILE_M - 1, 3), (TILE_M, 3), (TILE_M + 1, 3), (3, TILE_N - 1), (3, TILE_N), (3, TILE_N + 1),
                     (2 * TILE_M + 1, 2 * TILE_N + 1)]:
        u, num_u, v, psi = _case(7 * dim + n_u + n_v, dim, n_u, n_v)
        worst = max(worst, _check(P, u, num_u, v, psi, (dim, n_u, n_v)))
    print("plda_dense kernels at the tile edges, dim %d: worst error / bound %.3g" % (dim, worst))


def test_where_the_test_vector_is_the_class_mean_the_bound_still_holds():
    """v = m rounded to fp32: (v - m)^2 / var is next to nothing while the expanded terms are as large as ever."""
    P = H.pkg()
    u, num_u, v, psi = _case(77, 150, 17, 17)
    m = (num_u[:, None] * psi / (num_u[:, None] * psi + 1.0) * u).astype(np.float32)
    _check(P, u, num_u, m, psi, "v = m")


def test_a_dimension_above_the_largest_is_refused_and_an_empty_table_writes_nothing():
    P = H.pkg()
    u, num_u, v, psi = _case(3, 8, 4, 5)
    big = np.zeros((2, MAX_DIM + 1), np.float32)
    with pytest.raises(P.XvError, match="dimension larger than %d" % MAX_DIM) as e:
        P.asnorm.plda_score_dense(big, np.ones(2), big, np.ones(MAX_DIM + 1))
    assert e.value.status == P.XV_ERR_ARG
    assert P.asnorm.plda_score_dense(u[:0], num_u[:0], v, psi).shape == (0, 5) and P.asnorm.plda_score_dense(u, num_u, v[:0], psi).shape == (4, 0)
    # nothing is written: a guarded buffer handed to the C entry stays as it was
    L = P.lib()
    buf = np.full(8, 123.0)
    uf, vf, ps = np.ascontiguousarray(u), np.ascontiguousarray(v), np.ascontiguousarray(psi)
    assert L.xv_plda_score_dense(0, uf.ctypes.data, num_u.ctypes.data, 0, vf.ctypes.data, 5, 8, ps.ctypes.data, buf.ctypes.data, None) == 0
    assert L.xv_plda_score_dense(0, uf.ctypes.data, num_u.ctypes.data, 4, vf.ctypes.data, 0, 8, ps.ctypes.data, buf.ctypes.data, None) == 0
    assert np.all(buf == 123.0)


@pytest.mark.parametrize("dim", [3, 150, 512])
def test_a_score_does_not_depend_on_where_its_pair_sits(dim):
    P = H.pkg()
    rng = np.random.default_rng(dim)
    n_u, n_v = TILE_M + 7, TILE_N + 9
    u, num_u, v, psi = _case(11 * dim, dim, n_u, n_v)
    full = P.asnorm.plda_score_dense(u, num_u, v, psi)
    pu, pv = rng.permutation(n_u), rng.permutation(n_v)
    assert np.array_equal(P.asnorm.plda_score_dense(u[pu], num_u[pu], v[pv], psi), full[np.ix_(pu, pv)])
    su, sv = np.sort(rng.choice(n_u, 5, replace=False)), np.sort(rng.choice(n_v, 3, replace=False))
    assert np.array_equal(P.asnorm.plda_score_dense(u[su], num_u[su], v[sv], psi), full[np.ix_(su, sv)])
    assert np.array_equal(P.asnorm.plda_score_dense(u[-1:], num_u[-1:], v[-1:], psi), full[-1:, -1:])


@pytest.mark.parametrize("dim", [3, 150])
def test_rows_and_columns_of_the_statistics_see_the_same_scores(dim, monkeypatch):
    """by_column = 0 on (u, v) and by_column = 1 on the same tables are the statistics of the matrix and of its transpose: both
    equal xv_topn_stats of the matrix the dense entry returns, so the exchanged operands gave the same bits."""
    P = H.pkg()
    n_u, n_v = TILE_M + 3, TILE_N + 5
    u, num_u, v, psi = _case(13 * dim, dim, n_u, n_v)
    full = P.asnorm.plda_score_dense(u, num_u, v, psi)
    for n in (2, 17):
        by_row, by_col = P.asnorm.plda_cohort_stats(u, num_u, v, psi, n), P.asnorm.plda_cohort_stats(u, num_u, v, psi, n, by_column=True)
        want_row, want_col = P.asnorm.topn_stats(full, n), P.asnorm.topn_stats(np.ascontiguousarray(full.T), n)
        assert all(np.array_equal(a, b) for a, b in zip(by_row, want_row)) and all(np.array_equal(a, b) for a, b in zip(by_col, want_col))
    # n = all columns, a small workspace: the mean over a whole row is the same number whichever operand gave the rows
    monkeypatch.setenv("XVEC_PLDA_DENSE_WORKSPACE", str(8 * n_u * 5))
    assert np.array_equal(P.asnorm.plda_cohort_stats(u, num_u, v, psi, n_u, by_column=True)[0], P.asnorm.topn_stats(np.ascontiguousarray(full.T), n_u)[0])


@pytest.mark.parametrize("dim", [1, 64, 150, 512])
def test_the_dense_and_the_per_trial_kernel_agree_within_the_sum_of_their_bounds(dim):
    P = H.pkg()
    u, num_u, v, psi = R.scoring_case(5 * dim, dim, 17, 19)            # num in [1, 3]: what score_units() counts on
    dense = P.asnorm.plda_score_dense(u, num_u, v, psi)
    pairs = np.stack(np.meshgrid(np.arange(17), np.arange(19), indexing="ij"), -1).reshape(-1, 2)
    trial = P.plda_score(u, num_u, v, psi, pairs).reshape(17, 19)
    size_trial = A.dense_llr(u, num_u, v, psi)[1]
    bound = (dense_units(dim) * U53 * A.expanded_size(u, num_u, v, psi) + score_units(dim) * U53 * size_trial).astype(np.float64)
    diff = np.abs(dense.astype(LD) - trial.astype(LD)).astype(np.float64)
    print("dense against per-trial, dim %d: worst difference / bound %.3g" % (dim, float((diff / bound).max())))
    assert np.all(diff <= bound)
