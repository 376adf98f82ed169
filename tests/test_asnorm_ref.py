"""CPU tests of tests/asnorm_ref.py, the restatement that the GPU tests of adaptive score normalisation compare with: what it
computes is checked here against properties that need no other implementation."""
import numpy as np

import asnorm_ref as A
import plda_ref as R

LD = np.longdouble


def _case(seed=5, dim=10, n_train=6, n_test=9, n_cohort=14):
    u, num_u, v, psi = R.scoring_case(seed, dim, n_train, n_test + n_cohort)
    return u, num_u, v[:n_test], v[n_test:], psi


def _close(a, b, tol=LD(1e-15)):
    a, b = np.asarray(a).astype(LD), np.asarray(b).astype(LD)
    return bool(np.all(np.abs(a - b) <= tol * (1 + np.abs(b))))


def test_top_n_of_the_whole_cohort_is_plain_s_norm():
    train, num, test, cohort, psi = _case()
    pairs = [(e, t) for e in range(len(train)) for t in range(len(test))]
    raw = A.dense_llr(train, num, test, psi)[0].reshape(-1)
    s_e, s_t = A.cohort_scores(train, num, test, cohort, psi)
    direct = A.snorm_direct(raw, pairs, s_e, s_t)
    for top_n in (len(cohort), len(cohort) + 1, 1000):
        out, _, _ = A.asnorm(raw, pairs, train, num, test, cohort, psi, top_n)
        assert _close(out, direct)
    # and a smaller N is something else
    out, _, _ = A.asnorm(raw, pairs, train, num, test, cohort, psi, 3)
    assert not _close(out, direct, LD(1e-6))


def test_the_two_cohort_matrices_score_the_pairs_the_formula_names():
    train, num, test, cohort, psi = _case(seed=6)
    s_e, s_t = A.cohort_scores(train, num, test, cohort, psi)
    assert s_e.shape == (len(train), len(cohort)) and s_t.shape == (len(test), len(cohort))
    assert _close(s_e[2, 5], R.llr(train[2], num[2], cohort[5], psi), LD(1e-12))
    assert _close(s_t[4, 7], R.llr(cohort[7], 1.0, test[4], psi), LD(1e-12))


def test_a_constant_added_to_a_row_moves_the_mean_and_leaves_the_deviation():
    rng = np.random.default_rng(1)
    x = rng.integers(-50, 50, (4, 40)).astype(np.float64)
    for n in (2, 7, 40):
        m0, s0, _ = A.topn_stats(x, n)
        m1, s1, _ = A.topn_stats(x + 1024.0, n)
        assert np.array_equal(m1, m0 + 1024) and _close(s1, s0)


def test_a_duplicated_cohort_score_below_the_threshold_changes_nothing():
    rng = np.random.default_rng(2)
    row = rng.permutation(np.arange(30.0))
    n = 8                                           # the threshold is 22: 21 and everything below it is out
    for dup in (0.0, 5.0, 21.0):
        more = np.concatenate([row[:11], [dup], row[11:]])
        a, b = A.topn_stats(row[None], n), A.topn_stats(more[None], n)
        assert all(np.array_equal(p, q) for p, q in zip(a, b))
    assert list(row[A.topn_select(row, n)]) == [v for v in row if v >= 22]
    more = np.concatenate([row, [25.5]])            # above the threshold it pushes the 22 out
    assert A.topn_stats(more[None], n)[0][0] == A.topn_stats(row[None], n)[0][0] + LD(25.5 - 22) / n


def test_the_tie_rule_takes_the_lowest_columns():
    assert list(A.topn_select([1.0, 3.0, 3.0, 2.0, 3.0], 2)) == [1, 2]
    assert list(A.topn_select([1.0, 3.0, 3.0, 2.0, 3.0], 3)) == [1, 2, 4]
    assert list(A.topn_select([1.0, 3.0, 3.0, 2.0, 3.0], 4)) == [1, 2, 3, 4]
    assert list(A.topn_select([5.0, 5.0, 5.0, 5.0], 2)) == [0, 1]
    assert list(A.topn_select([2.0, 7.0, 2.0, 2.0, 9.0], 4)) == [0, 1, 2, 4]       # the ties straddle the 4th place
    assert list(A.topn_select([-0.0, 0.0, -1.0, 0.0], 2)) == [0, 1]               # -0 == +0: the column decides
    assert list(A.topn_select([0.0, -0.0, 1.0, -0.0], 3)) == [0, 1, 2]
    assert list(A.topn_select(np.arange(6.0), 2)) == [4, 5] and list(A.topn_select(-np.arange(6.0), 2)) == [0, 1]
    mean, std, mag = A.topn_stats([[-0.0, -0.0, -1.0]], 2, np.float64)
    assert mean[0] == 0 and not np.signbit(mean[0]) and std[0] == 0 and mag[0] == 0   # zeros are +0 in the sums


def test_mean_and_two_pass_deviation_and_the_symmetric_formula():
    mean, std, mag = A.topn_stats([[1.0, -9.0, 5.0, 3.0, -7.0]], 3)
    assert mean[0] == 3 and _close(std[0], np.sqrt(LD(8) / 3)) and mag[0] == 9
    mean, std, mag = A.topn_stats([[1.0, -9.0, 5.0, 3.0, -7.0]], 5)
    assert _close(mean[0], LD(-7) / 5) and mag[0] == 25
    assert A.symmetric(LD(4), LD(1), LD(2), LD(-2), LD(3)) == (LD(1.5) + LD(2)) / 2
    case = R.scoring_case(3, 4, 2, 3)
    assert np.all(A.expanded_size(*case) >= np.abs(A.dense_llr(*case)[0]))   # the terms' magnitudes bound their sum
