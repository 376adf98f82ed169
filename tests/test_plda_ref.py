"""CPU checks of the PLDA restatement (tests/plda_ref.py) against formulations that are independent of it: a dense
joint-Gaussian likelihood ratio, a known two-covariance model, the defining properties of LDA and a brute-force EER."""
import numpy as np
import pytest

import plda_ref as R


def _log_normal(z, cov):
    sign, logdet = np.linalg.slogdet(cov)
    assert sign > 0
    return -0.5 * (logdet + z @ np.linalg.solve(cov, z) + len(z) * np.log(2 * np.pi))


@pytest.mark.parametrize("n", [1, 3, 10])
def test_llr_is_the_joint_gaussian_likelihood_ratio(n):
    rng = np.random.default_rng(n)
    dim = 12
    psi = np.sort(rng.uniform(0.05, 8.0, dim))[::-1]
    P, I = np.diag(psi), np.eye(dim)
    same = np.block([[P + I / n, P], [P, I + P]])
    diff = np.block([[P + I / n, np.zeros((dim, dim))], [np.zeros((dim, dim)), I + P]])
    for _ in range(5):
        u, v = rng.standard_normal(dim) * 2, rng.standard_normal(dim) * 2
        z = np.concatenate([u, v])
        ref = _log_normal(z, same) - _log_normal(z, diff)
        assert abs(R.llr(u, n, v, psi) - ref) < 1e-9 * (1 + abs(ref))


def _two_covariance_data(rng, n_spk, dim, lo=2, hi=12):
    a = np.linalg.qr(rng.standard_normal((dim, dim)))[0]
    b_true = a @ np.diag(np.geomspace(20.0, 0.5, dim)) @ a.T          # well-separated between-class eigenvalues
    c = rng.standard_normal((dim, dim)) / np.sqrt(dim)
    w_true = c @ c.T + 0.5 * np.eye(dim)
    mu = rng.standard_normal(dim) * 3
    lb, lw = np.linalg.cholesky(b_true), np.linalg.cholesky(w_true)
    rows, segs = [], []
    for _ in range(n_spk):
        y = mu + lb @ rng.standard_normal(dim)
        k = int(rng.integers(lo, hi + 1))
        segs.append(list(range(len(rows), len(rows) + k)))
        rows.extend(y + (lw @ rng.standard_normal((dim, k))).T)
    return np.array(rows), segs, w_true, b_true


def test_plda_em_recovers_a_known_two_covariance_model():
    rng = np.random.default_rng(7)
    x, segs, w_true, b_true = _two_covariance_data(rng, 2000, 20)
    s_tot, sums, s_bet = R.scatter_stats(x, segs)
    mean, t, psi, w, b = R.plda_em(sums, [len(s) for s in segs], s_tot, s_bet)
    np.testing.assert_allclose(t @ w @ t.T, np.eye(20), atol=1e-9)
    np.testing.assert_allclose(t @ b @ t.T, np.diag(psi), atol=1e-8 * psi.max())
    assert np.all(np.diff(psi) <= 0)
    ref = np.sort(np.linalg.eigvals(np.linalg.solve(w_true, b_true)).real)[::-1]
    np.testing.assert_allclose(psi, ref, rtol=0.12)
    assert np.median(np.abs(psi / ref - 1)) < 0.05
    # the model's own whitening of the true within-class covariance is close to I
    np.testing.assert_allclose(t @ w_true @ t.T, np.eye(20), atol=0.1)


def _lda_setup(seed=3, dim=30, n_spk=80):
    rng = np.random.default_rng(seed)
    x, segs, _, _ = _two_covariance_data(rng, n_spk, dim, 3, 8)
    spk = np.empty(len(x), np.int64)
    for k, s in enumerate(segs):
        spk[s] = k
    return x.astype(np.float32), segs, spk


def test_lda_whitens_within_and_diagonalises_between():
    x, segs, spk = _lda_setup()
    m = R.lda(x, spk, 12)
    assert m.shape == (12, 31) and m.dtype == np.float32
    xc = x.astype(np.float64) - x.astype(np.float64).mean(0)
    s_tot, _, s_bet = R.scatter_stats(xc, segs)
    within, between = (s_tot - s_bet) / len(x), s_bet / len(x)
    L = m[:, :-1].astype(np.float64)
    np.testing.assert_allclose(L @ within @ L.T, np.eye(12), atol=1e-5)
    pb = L @ between @ L.T
    d = np.diag(pb)
    np.testing.assert_allclose(pb - np.diag(d), 0, atol=1e-5 * d.max())
    assert np.all(np.diff(d) <= 1e-6 * d.max())
    # the offset column centres the data: the projected mean is zero
    np.testing.assert_allclose(m[:, :-1] @ x.mean(0) + m[:, -1], 0, atol=1e-4)


def _scores(lda_m, x, segs, enroll, test, trials):
    def proj(v):
        y = v.astype(np.float64) @ lda_m[:, :-1].T.astype(np.float64) + lda_m[:, -1]
        return y * (np.sqrt(y.shape[1]) / np.linalg.norm(y, axis=1))[:, None]
    mean, t, psi = R.plda(proj(x), segs)
    u, _ = R.transform_ivector(proj(enroll), mean, t, psi, num=3)
    v, _ = R.transform_ivector(proj(test), mean, t, psi)
    return np.array([R.llr(u[i], 3, v[j], psi) for i, j in trials])


def test_lda_row_signs_do_not_change_plda_scores():
    x, segs, spk = _lda_setup(5)
    m = R.lda(x, spk, 10)
    enroll, test = x[:6], x[-9:]
    trials = [(i, j) for i in range(6) for j in range(9)]
    ref = _scores(m, x, segs, enroll, test, trials)
    flipped = m.copy()
    flipped[[0, 3, 7]] *= -1
    np.testing.assert_allclose(_scores(flipped, x, segs, enroll, test, trials), ref, atol=1e-10, rtol=1e-10)


def _eer_brute(tgt, non):
    """The same EER, as a threshold sweep over the target scores with unsorted counts: the first target rank p whose
    false-alarm count (non-targets >= the p-th smallest target score) is at most floor(|non| p / |tgt|)."""
    tgt = np.asarray(tgt, np.float32)
    non = np.asarray(non, np.float32)
    ranked = np.sort(tgt)
    for p in range(len(tgt) - 1):
        fa = int((non >= ranked[p]).sum())
        if fa <= int(len(non) * p / len(tgt)):
            return p / len(tgt), float(ranked[p])
    return (len(tgt) - 1) / len(tgt), float(ranked[-1])


@pytest.mark.parametrize("tgt,non,expect", [
    ([5, 6, 7], [1, 2, 3], (0.0, 5.0)),                     # every target above every non-target
    ([0.5], [3, 4, -1], (0.0, 0.5)),                        # a single target
    ([1, 1, 1, 1], [1, 1, 1, 1], (0.75, 1.0)),              # ties everywhere
    ([1, 2], [3, 4], (0.5, 2.0)),                           # every target below every non-target
    ([1, 3, 5, 7], [0, 2, 4, 6], (0.5, 5.0)),               # interleaved
    ([2, 2, 3, 9], [2, 2, 1, 0, 5], (0.5, 3.0)),            # ties at the threshold
])
def test_eer_known_answers(tgt, non, expect):
    e, thr = R.eer(tgt, non)
    assert (e, thr) == pytest.approx(expect)
    assert (e, thr) == pytest.approx(_eer_brute(tgt, non))


def test_eer_matches_the_brute_force_sweep_on_random_lists():
    rng = np.random.default_rng(11)
    for _ in range(200):
        nt, nn = int(rng.integers(1, 30)), int(rng.integers(1, 60))
        tgt = np.round(rng.normal(1.0, 1.0, nt), 1)              # coarse values: many ties
        non = np.round(rng.normal(0.0, 1.0, nn), 1)
        e, thr = R.eer(tgt, non)
        be, bthr = _eer_brute(tgt, non)
        assert e == pytest.approx(be) and thr == bthr
    with pytest.raises(ValueError):
        R.eer([1.0], [])
