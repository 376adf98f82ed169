"""numpy restatement of adaptive score normalisation for the tests: the all-pairs PLDA ratio, the exact top-N
selection with the project's tie rule, the two-pass statistics and the symmetric formula.

  S_e[e][c] = LLR(e with num_e examples, c)        the speaker against the cohort
  S_t[t][c] = LLR(c with one example, t)           the cohort against the utterance
  top-N of a row: the N largest values; among values equal to the N-th largest, the lowest columns (-0 counts as +0)
  mu = sum / N, sigma = sqrt(sum (x - mu)^2 / N)   (population standard deviation, the second sum after the first)
  out = 1/2 ((s - mu_e) / sigma_e + (s - mu_t) / sigma_t)

N = the cohort size is plain S-norm.  Everything runs in np.longdouble unless a dtype is given.
"""
import numpy as np

import plda_ref as R

LD = np.longdouble


def dense_llr(u, num_u, v, psi):
    """(llr, size) [n_u, n_v] of plda_ref.llr_ld: the ratio of every pair in long double, and the magnitudes of its terms in
    the per-trial form."""
    return R.llr_ld(u, num_u, v, psi)


def expanded_size(u, num_u, v, psi):
    """[n_u, n_v]: the magnitudes of the terms of the expanded form S = r + sum A1 v + sum A2 v^2 that the dense kernel adds up,
    sum_d |A1 v| + sum_d |A2 v^2| + (1/2 sum |log(1 + psi)| + 1/2 sum |log var| + 1/2 sum m^2 / var), r taken term by term."""
    u = np.atleast_2d(np.asarray(u)).astype(LD)
    v = np.atleast_2d(np.asarray(v)).astype(LD)
    psi = np.asarray(psi).astype(LD)[None, :]
    n = np.broadcast_to(np.asarray(num_u).astype(LD), (len(u),))[:, None]
    m = n * psi / (n * psi + 1) * u
    var = 1 + psi / (n * psi + 1)
    a1 = m / var
    a2 = (1 / (1 + psi) - 1 / var) / 2
    r_abs = (np.abs(np.log(1 + psi)).sum() + np.abs(np.log(var)).sum(1) + (m * m / var).sum(1)) / 2
    return np.abs(a1) @ np.abs(v).T + np.abs(a2) @ (v * v).T + r_abs[:, None]


def topn_select(row, n):
    """The columns of the n largest values of a row, ascending: by value (numerically: -0 == +0), then by column."""
    row = np.asarray(row)
    order = np.lexsort((np.arange(len(row)), -(row + 0)))   # last key first: descending value, then ascending column
    return np.sort(order[:n])


def topn_stats(x, n, dtype=LD):
    """(mean, std, abs_sum) per row of x [rows, cols]: the statistics of its n largest values in `dtype`, and the sum of their
    absolute values (what the error bounds are made of)."""
    x = np.atleast_2d(np.asarray(x))
    mean, std, mag = np.empty(len(x), dtype), np.empty(len(x), dtype), np.empty(len(x), dtype)
    for i, row in enumerate(x):
        sel = row[topn_select(row, n)].astype(dtype) + dtype(0)   # -0 -> +0
        if np.all(sel == sel[0]):                                  # one value: it is the mean, whatever n x / n rounds to
            mean[i], std[i] = sel[0], 0
        else:
            mean[i] = sel.sum() / dtype(n)
            std[i] = np.sqrt(((sel - mean[i]) ** 2).sum() / dtype(n))
        mag[i] = np.abs(sel).sum()
    return mean, std, mag


def symmetric(s, mu_e, sigma_e, mu_t, sigma_t):
    return ((s - mu_e) / sigma_e + (s - mu_t) / sigma_t) / 2


def cohort_scores(train, num_train, test, cohort, psi):
    """(S_e [n_train, n_cohort], S_t [n_test, n_cohort]) in long double."""
    s_e = dense_llr(train, num_train, cohort, psi)[0]
    s_t = dense_llr(cohort, np.ones(len(cohort)), test, psi)[0].T
    return s_e, s_t


def asnorm(raw, pairs, train, num_train, test, cohort, psi, top_n):
    """The normalised score of every trial pairs[i] = (training row, test row) with raw score raw[i]; also the statistics:
    (out, (mu_e, sigma_e), (mu_t, sigma_t)), the statistics per row of the two tables."""
    s_e, s_t = cohort_scores(train, num_train, test, cohort, psi)
    top_n = min(top_n, len(cohort))
    mu_e, sd_e, _ = topn_stats(s_e, top_n)
    mu_t, sd_t, _ = topn_stats(s_t, top_n)
    pairs = np.asarray(pairs).reshape(-1, 2)
    raw = np.asarray(raw).astype(LD)
    with np.errstate(divide="ignore", invalid="ignore"):
        out = symmetric(raw, mu_e[pairs[:, 0]], sd_e[pairs[:, 0]], mu_t[pairs[:, 1]], sd_t[pairs[:, 1]])
    return out, (mu_e, sd_e), (mu_t, sd_t)


def snorm_direct(raw, pairs, s_e, s_t):
    """Plain S-norm from whole rows, without any selection: numpy's mean and std."""
    pairs = np.asarray(pairs).reshape(-1, 2)
    raw = np.asarray(raw).astype(LD)
    return ((raw - s_e.mean(1)[pairs[:, 0]]) / s_e.std(1)[pairs[:, 0]] + (raw - s_t.mean(1)[pairs[:, 1]]) / s_t.std(1)[pairs[:, 1]]) / 2
