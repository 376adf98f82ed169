"""CPU checks of tests/plda_adapt_ref.py (the restatement of ivector-adapt-plda) against forms that do not use its
eigenvector choices: the covariances a PLDA model stands for, Sigma_w = T^-1 T^-T and Sigma_b = T^-1 diag(psi) T^-T, and
the excess E of the adaptation covariance over the model's total covariance (plda_adapt_ref.excess)."""
import numpy as np
import pytest

import plda_adapt_ref as A


def _model(rng, dim):
    mean = rng.standard_normal(dim) * 0.3
    t = np.linalg.qr(rng.standard_normal((dim, dim)))[0] * rng.uniform(0.5, 2.0, dim)[:, None]
    psi = np.sort(rng.uniform(0.05, 6.0, dim))[::-1]
    return mean, t, psi


def _in_domain(rng, mean, t, psi, n, shift=0.4, up=(3.0, 2.0, 1.6), down=(0.3, 0.5)):
    """Vectors with the model's total covariance, except that a few directions carry more variance and a few less, and
    the mean moved by `shift` (in units of the total standard deviation)."""
    dim = len(mean)
    tm = t / np.sqrt(1.0 + psi)[:, None]
    r = np.linalg.qr(rng.standard_normal((dim, dim)))[0]
    scale = np.ones(dim)
    scale[: len(up)] = np.sqrt(up)
    scale[len(up): len(up) + len(down)] = np.sqrt(down)
    z = rng.standard_normal((n, dim)) * scale
    x = np.linalg.solve(tm, (z @ r.T).T).T + mean + shift * np.linalg.solve(tm, r[:, -1])
    return x.astype(np.float32)


def _close(a, b, rtol):
    assert np.abs(a - b).max() <= rtol * np.abs(b).max(), np.abs(a - b).max() / np.abs(b).max()


@pytest.mark.parametrize("dim", [5, 40])
def test_data_like_the_model_changes_no_covariance(dim):
    rng = np.random.default_rng(dim)
    mean, t, psi = _model(rng, dim)
    tm = t / np.sqrt(1.0 + psi)[:, None]
    r = np.linalg.qr(rng.standard_normal((dim, dim)))[0]
    ti = np.linalg.inv(tm)
    sigma = ti @ r @ np.diag(rng.uniform(0.2, 0.95, dim)) @ r.T @ ti.T       # every s_i < 1 where the total is I
    n = 1000
    m, v = n * mean, n * (sigma + np.outer(mean, mean))
    mean2, t2, psi2, s = A.adapt(n, m, v, mean, t, psi, within_covar_scale=0.75, between_covar_scale=0.25)
    assert s.max() < 1.0
    np.testing.assert_allclose(mean2, mean, rtol=1e-12, atol=1e-15)
    w, b = A.implied_covariances(t, psi)
    w2, b2 = A.implied_covariances(t2, psi2)
    _close(w2, w, 1e-10)
    _close(b2, b, 1e-10)
    np.testing.assert_allclose(psi2, np.sort(psi)[::-1], rtol=1e-9)      # the same model, up to the transform's rows


@pytest.mark.parametrize("within,between", [(0.3, 0.7), (0.75, 0.25), (1.0, 0.0)])
@pytest.mark.parametrize("dim", [6, 50])
def test_adapted_covariances_are_the_old_ones_plus_the_scaled_excess(dim, within, between):
    rng = np.random.default_rng(100 + dim)
    mean, t, psi = _model(rng, dim)
    x = _in_domain(rng, mean, t, psi, 4000)
    n, m, v = A.stats(x)
    mean2, t2, psi2, s = A.adapt(n, m, v, mean, t, psi, within_covar_scale=within, between_covar_scale=between)
    assert s.max() > 1.0 and s.min() < 1.0                                  # both kinds of directions occur
    assert np.all(np.diff(s) <= 0)
    x64 = x.astype(np.float64)
    mu = x64.mean(0)
    np.testing.assert_allclose(mean2, mu, rtol=1e-12, atol=1e-14)
    d = mu - mean
    sigma = np.cov(x64.T, bias=True) + np.outer(d, d)
    e = A.excess(sigma, t, psi)
    w, b = A.implied_covariances(t, psi)
    w2, b2 = A.implied_covariances(t2, psi2)
    _close(w2, w + within * e, 1e-9)
    _close(b2, b + between * e, 1e-9)
    # a valid PLDA model: T' makes the adapted within-class covariance I and the between-class one diag(psi')
    _close(t2 @ (w + within * e) @ t2.T, np.eye(dim), 1e-9)
    _close(t2 @ (b + between * e) @ t2.T, np.diag(psi2), 1e-9)
    assert np.all(np.diff(psi2) <= 0) and psi2.min() >= 0


def test_mean_diff_scale_adds_exactly_the_outer_product_of_the_shift():
    rng = np.random.default_rng(7)
    dim = 12
    mean, t, psi = _model(rng, dim)
    n, m, v = A.stats(_in_domain(rng, mean, t, psi, 2000, shift=1.5))
    out = {}
    for mds in (0.0, 1.0):
        mean2, _, _, s, it = A.adapt(n, m, v, mean, t, psi, mean_diff_scale=mds, internals=True)
        ti = np.linalg.inv(it["tm"])
        out[mds] = (mean2, ti @ it["p"] @ np.diag(s) @ it["p"].T @ ti.T, it["d"])   # the covariance that was diagonalised
    np.testing.assert_array_equal(out[0.0][0], out[1.0][0])
    d = out[1.0][2]
    assert np.linalg.norm(d) > 0.1
    _close(out[1.0][1] - out[0.0][1], np.outer(d, d), 1e-9)


def test_no_vectors_is_an_error():
    rng = np.random.default_rng(1)
    mean, t, psi = _model(rng, 4)
    with pytest.raises(ValueError):
        A.adapt(0, np.zeros(4), np.zeros((4, 4)), mean, t, psi)


def test_filter_scp_keeps_lines_whose_first_field_is_listed():
    keys = ["spkA x target\n", "spkC y nontarget\n", "\n"]
    lines = ["spkA u1 1.5\n", "spkB u1 0.2\n", "spkC u9 -3\n", "spkA u2 0.1\n", "spkAA u2 7\n"]
    assert A.filter_scp(keys, lines) == ["spkA u1 1.5\n", "spkC u9 -3\n", "spkA u2 0.1\n"]
