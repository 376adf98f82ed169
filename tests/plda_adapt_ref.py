"""fp64 numpy restatement of ivector-adapt-plda (stage 2 of egs/sre/v2/run_sre16.sh: unsupervised adaptation of an
out-of-domain PLDA model to unlabelled in-domain vectors) for the tests.

Semantics are upstream Kaldi's [UPSTREAM, recalled]: ivectorbin/ivector-adapt-plda.cc and PldaUnsupervisedAdaptor in
ivector/plda.cc.  Neither is vendored in the reference; parity with Kaldi itself stays unpinned, as for plda_ref.py.

  stats:     every vector read as float and added with weight 1 in fp64: n, m = sum x, V = sum x x^T
  1.         mu = m / n, S = V / n - mu mu^T, d = mu - mean, S += mean_diff_scale d d^T; the new mean is mu
  2.         T' = diag(1 / sqrt(1 + psi)) T (the model's total covariance is I there)
  3.         T' S T'^T = P diag(s) P^T, s descending
  4.         W = diag(1 / (1 + psi)), B = diag(psi / (1 + psi)); W2 = P^T W P, B2 = P^T B P;
             for every i with s_i > 1: W2[i, i] += within (s_i - 1), B2[i, i] += between (s_i - 1)
  5.         Wm = P W2 P^T, Bm = P B2 P^T, Wm = C C^T, C^-1 Bm C^-T = Q diag(psi') Q^T (descending)
  6.         transform' = Q^T C^-1 T', psi' (Plda::ComputeDerivedVars recomputes the offset)
"""
import numpy as np

from plda_ref import eig_desc


def stats(x):
    """(n, m, V) of vectors x [n, dim] (float32, accumulated in fp64)."""
    x = np.asarray(x, np.float32).astype(np.float64)
    return len(x), x.sum(0), x.T @ x


def adapt(n, m, v, mean, transform, psi, mean_diff_scale=1.0, within_covar_scale=0.3, between_covar_scale=0.7,
          internals=False):
    """PldaUnsupervisedAdaptor::UpdatePlda: (mean', transform', psi', s), and with internals also a dict of the
    intermediate quantities (sigma, tm, P, C)."""
    if n < 1:
        raise ValueError("no adaptation vectors")
    mean = np.asarray(mean, np.float64)
    transform = np.asarray(transform, np.float64)
    psi = np.asarray(psi, np.float64)
    mu = np.asarray(m, np.float64) / n
    sigma = np.asarray(v, np.float64) / n - np.outer(mu, mu)
    d = mu - mean
    sigma = sigma + mean_diff_scale * np.outer(d, d)
    tm = transform / np.sqrt(1.0 + psi)[:, None]
    s, p = eig_desc(tm @ sigma @ tm.T)
    w2 = p.T @ np.diag(1.0 / (1.0 + psi)) @ p
    b2 = p.T @ np.diag(psi / (1.0 + psi)) @ p
    for i in range(len(s)):
        if s[i] > 1.0:
            w2[i, i] += within_covar_scale * (s[i] - 1.0)
            b2[i, i] += between_covar_scale * (s[i] - 1.0)
    wm = p @ w2 @ p.T
    bm = p @ b2 @ p.T
    c = np.linalg.cholesky((wm + wm.T) / 2)
    ci = np.linalg.inv(c)
    psi_new, q = eig_desc(ci @ bm @ ci.T)
    t_new = q.T @ ci @ tm
    if internals:
        return mu, t_new, psi_new, s, dict(sigma=sigma, tm=tm, p=p, c=c, d=d)
    return mu, t_new, psi_new, s


def implied_covariances(transform, psi):
    """The within- and between-class covariances a PLDA model stands for: T^-1 T^-T and T^-1 diag(psi) T^-T."""
    ti = np.linalg.inv(np.asarray(transform, np.float64))
    return ti @ ti.T, ti @ np.diag(np.asarray(psi, np.float64)) @ ti.T


def excess(sigma, transform, psi):
    """E = T'^-1 P diag(max(s - 1, 0)) P^T T'^-T from an eigendecomposition of T' sigma T'^T of its own: the part of the
    adaptation covariance that the model's total covariance does not explain (a matrix function, so it does not depend on
    how degenerate eigenvectors are chosen)."""
    tm = np.asarray(transform, np.float64) / np.sqrt(1.0 + np.asarray(psi, np.float64))[:, None]
    a = tm @ sigma @ tm.T
    s, u = np.linalg.eigh((a + a.T) / 2)
    f = u @ np.diag(np.maximum(s - 1.0, 0.0)) @ u.T
    ti = np.linalg.inv(tm)
    return ti @ f @ ti.T


def filter_scp(keys_lines, lines):
    """utils/filter_scp.pl <id-list> <in>: the lines of `lines` whose first field is the first field of a line of
    `keys_lines`, in their own order."""
    keep = {ln.split()[0] for ln in keys_lines if ln.split()}
    return [ln for ln in lines if ln.split() and ln.split()[0] in keep]
