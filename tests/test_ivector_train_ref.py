"""The numpy restatement of i-vector extractor training (tests/ivector_train_ref.py) against itself.  No GPU."""
import numpy as np
import pytest

import ivector_ref as R
import ivector_train_ref as T


def _utts(seed, n, G, D, lo=5, hi=30):
    rng = np.random.default_rng(seed)
    out = []
    for u in range(n):
        frames = int(rng.integers(lo, hi))
        x = rng.normal(size=(frames, D)).astype(np.float32)
        post = []
        for _ in range(frames):
            k = int(rng.integers(1, min(3, G) + 1))
            w = rng.random(k).astype(np.float32)
            post.append((rng.permutation(G)[:k].astype(np.int32), (w / w.sum()).astype(np.float32)))
        out.append((x, post))
    return out


def test_the_statistics_of_two_halves_add_up_to_the_whole():
    model = R.random_model(3, 4, 5, 6)
    utts = _utts(1, 12, 4, 5)
    whole, ab = T.accumulate(utts, model, with_abs=True)
    halves = T.add_stats(T.accumulate(utts[:5], model), T.accumulate(utts[5:], model))
    assert whole["num_ivectors"] == halves["num_ivectors"] == 12
    for k in ("gamma", "Y", "R", "S", "ivector_sum", "ivector_scatter", "auxf", "frames"):
        err = np.max(np.abs(np.asarray(whole[k]) - np.asarray(halves[k])) - 12 * 2.0 ** -53 * np.asarray(ab[k]))
        assert err <= 0, (k, err)


def test_the_objective_of_an_utterance_is_the_bound_written_with_the_full_posterior():
    """auxf_post against the same bound computed as E_q[log p(x, y)] - E_q[log q(y)] by its closed form through other products"""
    model = R.random_model(5, 3, 4, 5)
    (x, post), = _utts(2, 1, 3, 4)
    e = T.e_step(x, post, model)
    S, p = 5, model["prior_offset"]
    e0 = np.zeros(S)
    e0[0] = p
    m, var, Q, l = e["m"], e["var"], e["Q"], e["l"]
    # with Q m = l: l_a.m - m'Q_a m/2 - tr(Var Q_a)/2 - (|m - p e0|^2 + tr Var)/2 + logdet Var/2 + S/2 = l.m/2 - p^2/2 + logdet Var/2
    closed = 0.5 * l @ m - 0.5 * p * p + 0.5 * e["logdet"]
    assert abs(e["auxf_post"] - closed) <= 64 * 2.0 ** -53 * e["auxf_post_abs"]


def test_the_m_step_on_statistics_of_an_exact_model_returns_that_model():
    """Statistics built so that Y_g = M_g R_g and S_g = M_g R_g M_g' + gamma_g Sigma_g, with i-vector moments of mean p e_0 and unit
    covariance: every part of the update is then at its fixed point."""
    rng = np.random.default_rng(7)
    G, D, S = 3, 4, 5
    model = R.random_model(11, G, D, S)
    p = model["prior_offset"]
    st = T.zero_stats(G, D, S)
    n = 500.0
    e0 = np.zeros(S)
    e0[0] = p
    st["num_ivectors"] = n
    st["ivector_sum"] = n * e0
    st["ivector_scatter"] = R.pack(n * (np.eye(S) + np.outer(e0, e0)))
    for g in range(G):
        A = rng.normal(size=(S, S))
        Rg = 200.0 * (A @ A.T / S + np.eye(S))
        st["gamma"][g] = 150.0 + 10 * g
        st["R"][g] = R.pack(Rg)
        st["Y"][g] = model["M"][g] @ Rg
        cov = np.linalg.inv(R.unpack(model["sigma_inv"][g], D))
        st["S"][g] = R.pack(model["M"][g] @ Rg @ model["M"][g].T + st["gamma"][g] * cov)
    out = T.m_step(st, model, variance_floor_factor=1e-3, diagonalize=False)
    assert out["eig_floored"] == 0 and out["var_floored"] == 0 and out["prior_floored"] == 0
    assert abs(out["prior_offset"] - p) < 1e-12 * p
    # V is orthogonal with V e_0 = e_0: the columns 1.. of M may be rotated among themselves, M M' and column 0 may not change
    for g in range(G):
        np.testing.assert_allclose(out["M"][g][:, 0], model["M"][g][:, 0], rtol=0, atol=1e-11)
        np.testing.assert_allclose(out["M"][g] @ out["M"][g].T, model["M"][g] @ model["M"][g].T, rtol=0, atol=1e-10)
    np.testing.assert_allclose(out["sigma_inv"], model["sigma_inv"], rtol=0, atol=1e-9)
    assert abs(out["impr_proj"]) < 1e-9 and abs(out["impr_var"]) < 1e-9 and abs(out["impr_prior"]) < 1e-9


def test_the_prior_update_whitens_the_ivectors():
    model = R.random_model(3, 4, 5, 6)
    st = T.accumulate(_utts(4, 40, 4, 5), model)
    out = T.m_step(st, model, gaussian_min_count=1.0)
    V, e0 = out["V"], np.eye(6)[0]
    np.testing.assert_allclose(V @ out["mu"], out["prior_offset"] * e0, atol=1e-12 * np.linalg.norm(V) * np.linalg.norm(out["mu"]) * 6)
    np.testing.assert_allclose(V @ out["C"] @ V.T, np.eye(6), atol=1e-9)


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_five_passes_of_em_raise_the_bound_on_every_pass(seed):
    utts, model = T.em_data(seed)
    objf, floored = [], []
    for it in range(5):
        st, ab = T.accumulate(utts, model, with_abs=True)
        objf.append((st["auxf"] / st["frames"], len(utts) * 2.0 ** -53 * ab["auxf"] / st["frames"]))
        out = T.m_step(st, model, variance_floor_factor=1e-3)
        floored.append(out["eig_floored"])
        model = {k: out[k] for k in ("w_vec", "M", "sigma_inv", "prior_offset")}
    print(seed, [o[0] for o in objf], floored)
    for (a, _), (b, tol) in zip(objf, objf[1:]):
        assert b >= a - tol, objf


def test_the_generator_of_init_is_standard_normal_and_repeats():
    a, b = T.init_normal(5, 4000), T.init_normal(5, 4000)
    assert np.array_equal(a, b) and not np.array_equal(a[:100], T.init_normal(6, 100))
    assert abs(a.mean()) < 4 / np.sqrt(4000) and abs(a.std() - 1) < 0.05
