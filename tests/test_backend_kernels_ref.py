"""The CPU half of tests/test_gpu_backend_kernels.py: the input builders of tests/plda_ref.py, the preconditions that the exact
cases rest on (partial sums below 2^53 in float64 and below 2^24 in float32), the np.longdouble restatements against the
float64 ones, and that no instance of a templated kernel is left without a case."""
import numpy as np

import plda_ref as R
import test_gpu_backend_kernels as G


def test_the_constants_were_found_and_every_instance_has_a_case():
    assert G.J_INSTANCES[-1] * G.WAVE == G.MAX_DIM and G.RF_INSTANCES[-1] == G.MAX_RF
    assert len(G.J_INSTANCES) > 1 and len(G.RF_INSTANCES) > 2
    assert min(G.TILE, G.KS, G.AHEAD, G.TR_ROWS, G.VB, G.KT, G.CHUNK_CAP, G.CHUNK_ROWS) > 1
    assert {G.transform_instance(d) for d in G.TRANSFORM_DIMS} == set(G.J_INSTANCES)
    assert max(G.TRANSFORM_DIMS) == G.MAX_DIM
    rows = [r for r in G.BACKEND_ROWS if r <= 16 * G.MAX_RF]
    assert {G.backend_instance(r) for r in rows} == set(G.RF_INSTANCES)
    for rf in G.RF_INSTANCES:                                 # vector stores (rows a multiple of 4) and scalar stores
        assert {r % 4 == 0 for r in rows if G.backend_instance(r) == rf} == {False, True}
    assert {r % 4 == 0 for r in G.BACKEND_ROWS if r > 16 * G.MAX_RF} == {False, True}


def test_ragged_lengths_and_segments():
    rng = np.random.default_rng(1)
    for total in (1, 17, 130, 4100):
        lengths = R.ragged_lengths(rng, [1, 2, 4, 8, 64, 128], total=total)
        assert sum(lengths) == total and lengths[0] == 0 and lengths[-1] == 0 and set(lengths) <= {0, 1, 2, 4, 8, 64, 128}
    assert 0 in R.ragged_lengths(rng, [1, 2, 4, 8, 64, 128], total=130)[1:-1]
    for count in (2, 15, 65):
        lengths = R.ragged_lengths(rng, [0, 3, 5], count=count)
        assert len(lengths) == count and lengths[0] == 0 and lengths[-1] == 0 and set(lengths) <= {0, 3, 5}
    segs = R.segments_of_lengths(rng, [0, 1, 3, 64, 0, 8], 20)
    assert [len(s) for s in segs] == [0, 1, 3, 64, 0, 8] and all(0 <= i < 20 for s in segs for i in s)
    assert all(a >= b for a, b in zip(segs[3], segs[3][1:])) and len(set(segs[3])) < 64      # a descending run with repeats


def test_exact_scatter_cases_keep_every_partial_sum_exact_and_match_the_float64_restatement():
    n_cases = 0
    for dim, x, segs in G.exact_scatter_cases():
        assert np.abs(x).max() <= 8 and (not segs or (not segs[0] and not segs[-1]))
        assert {len(s) for s in segs} <= set(G.POW2_LENGTHS)
        s_tot, sums, s_bet, largest = R.scatter_stats_exact(x, segs)
        assert largest < 2 ** 53
        f_tot, f_sums, f_bet = R.scatter_stats(x, segs)
        assert np.array_equal(s_tot, f_tot) and np.array_equal(sums, f_sums) and np.array_equal(s_bet, f_bet)
        n_cases += 1
    assert n_cases > 100


def test_bounded_scatter_cases_hold_the_lengths_around_the_load_ahead():
    seen = set()
    for dim, x, segs in G.bounded_scatter_cases():
        seen |= {len(s) for s in segs}
        assert x.dtype == np.float32
    a = G.AHEAD
    assert seen >= {0, 3, 5, a - 1, a, a + 1, 2 * a + 1}
    x = np.random.default_rng(3).standard_normal((9, 4)).astype(np.float32)
    segs = [[], [8, 8, 1, 0], [2]]
    np.testing.assert_allclose(R.sequential_sums(x, segs), R.scatter_stats(x, segs)[1], rtol=1e-15)


def test_transform_cases_are_integers_below_2_to_the_24_and_never_zero():
    for dim in G.TRANSFORM_DIMS:
        for n in G.TRANSFORM_ROWS:
            x, t, offset, psi, num, y = G.transform_case(dim, n)
            assert np.abs(t).max() <= 4 and np.abs(x).max() <= 8 and np.array_equal(t, np.round(t)) and np.array_equal(offset, np.round(offset))
            assert np.all(psi >= 0) and (psi == 0).any() and set(num) <= {1.0, 3.0, 17.0}
            assert np.abs(y).max() < 2 ** 24 and y.any(axis=1).all()
            assert np.array_equal(R.transform_ivector_ld(x, t, offset, psi, num)[0], y)
    assert {v for n in G.TRANSFORM_ROWS for v in G.transform_case(1, n)[4]} == {1.0, 3.0, 17.0}


def test_backend_cases_keep_the_sum_of_squares_below_2_to_the_24():
    for affine in (False, True):
        for n, dim, rows in G.backend_cases(affine):
            x, mean, t, y = G.backend_case(n, dim, rows, affine)
            assert set(np.unique(x)) <= {-1, 0, 1} and set(np.unique(t[:, :dim])) <= {-1, 0, 1} and set(np.unique(mean)) <= {-1, 0, 1}
            assert t.shape == (rows, dim + affine) and (y * y).sum(1).max() < 2 ** 24
            assert affine or not y[n // 2].any()
    cases = set(G.backend_cases(False))
    assert {r for _, _, r in cases} == set(G.BACKEND_ROWS) and {d for _, d, _ in cases} == set(G.BACKEND_DIMS)
    assert {n for n, _, _ in cases} == set(G.BACKEND_N)


def test_longdouble_restatements_agree_with_the_float64_ones():
    rng = np.random.default_rng(11)
    for dim in (1, 7, 150):
        mean = rng.standard_normal(dim)
        t = np.linalg.qr(rng.standard_normal((dim, dim)))[0] * rng.uniform(0.5, 2.0, dim)[:, None]
        psi = np.sort(rng.uniform(0.0, 6.0, dim))[::-1]
        psi[-1] = 0.0
        x = (rng.standard_normal((9, dim)) * 3).astype(np.float32)
        num = np.array([(1, 3, 17)[i % 3] for i in range(9)], np.float64)
        for simple in (False, True):
            y, scale = R.transform_ivector_ld(x, t, -(t @ mean), psi, num, simple=simple)
            ry, rscale = R.transform_ivector(x, mean, t, psi, num, normalize=False, simple=simple)
            np.testing.assert_allclose(scale.astype(np.float64), rscale, rtol=1e-12)
            np.testing.assert_allclose(y.astype(np.float64), ry, rtol=1e-5, atol=1e-5)         # ry is rounded to float32
            rn = R.transform_ivector(x, mean, t, psi, num, normalize=True, simple=simple)[0]
            np.testing.assert_allclose((y * scale[:, None]).astype(np.float64), rn, rtol=1e-5, atol=1e-5)
        u, num_u, v, psi = R.scoring_case(dim, dim, 4, 3)
        llr, size = R.llr_ld(u, num_u, v, psi)
        for k in range(4):
            for j in range(3):
                ref = R.llr(u[k], num_u[k], v[j], psi)
                assert abs(float(llr[k, j]) - ref) <= 1e-12 * float(size[k, j])
                assert abs(ref) <= float(size[k, j])


def test_scoring_cases_stay_in_the_ranges_the_bound_counts_on_and_the_bound_is_1000_times_tighter_than_the_old_one():
    for dim in G.SCORE_DIMS:
        for n_u in G.SCORE_N_U:
            u, num_u, v, psi = R.scoring_case(100 * dim + n_u, dim, n_u, G.SCORE_N_V)
            assert u.dtype == np.float32 and v.dtype == np.float32
            assert np.all((psi == 0) | ((psi >= 2) & (psi <= 6))) and np.all((num_u >= 1) & (num_u <= 3))
            llr, size = R.llr_ld(u, num_u, v, psi)
            bound = G.score_units(dim) * G.U53 * size.astype(np.float64)
            assert np.all(1000 * bound <= 1e-9 * (1 + np.abs(llr.astype(np.float64)))), (dim, n_u)
    # the constants of score_units()'s derivation, at the corners of those ranges
    q = lambda n, p: p / (n * p + 1)
    assert 1 / np.log(3.0) < 1 and 1 + 3 * q(1, 6) / (1 + q(1, 6)) < 2.5 and 2.5 / np.log(1 + q(3, 2)) < 10
    assert max(5 * (1 + p) / (1 + q(n, p)) for n in (1, 3) for p in (2, 6)) < 27
