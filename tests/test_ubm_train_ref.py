"""The restatement of full-covariance UBM training (tests/ubm_train_ref.py) against closed forms.  No device, no binaries."""
import numpy as np

import ubm_ref as R
import ubm_train_ref as T

F = np.float32


def one_gaussian(D, seed=0):
    """weights, Sigma^-1 mu, packed Sigma^-1 of one standard-normal Gaussian"""
    return np.ones(1, F), np.zeros((1, D), F), R.pack(np.eye(D)).astype(F)[None]


def whole_data_stats(x, flags=7):
    T_ = len(x)
    return T.acc_stats(x, np.arange(T_), np.zeros(T_, np.int64), np.ones(T_, F), 1, flags)


def moments(est, D):
    """(means [G, D], covariances [G, D, D]) of an estimate"""
    sig = np.stack([np.linalg.inv(R.unpack(p, D)) for p in est["inv_covars"]])
    return np.einsum("gij,gj->gi", sig, est["means_invcovars"].astype(np.float64)), sig


def test_one_gaussian_with_posterior_one_gives_the_sample_mean_and_covariance():
    rng = np.random.default_rng(1)
    D = 5
    x = (rng.normal(size=(400, D)) @ rng.normal(size=(D, D)) + 3.0).astype(F)
    occ, mean, cov = whole_data_stats(x)
    assert occ[0] == 400.0
    est = T.fgmm_est(*one_gaussian(D), occ, mean, cov)
    mu, sig = moments(est, D)
    x64 = x.astype(np.float64)
    np.testing.assert_allclose(mu[0], x64.mean(0), rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(sig[0], np.cov(x64.T, bias=True), rtol=1e-4, atol=1e-5)
    assert est["weights"].tolist() == [1.0] and est["removed"] == [] and est["floored"] == (0, 0)
    assert est["objf_after"] > est["objf_before"]


def test_a_rank_deficient_covariance_gets_its_null_space_floored():
    rng = np.random.default_rng(2)
    D, rank = 6, 4
    x = (rng.normal(size=(300, rank)) @ rng.normal(size=(rank, D))).astype(F)   # float32 rounding leaves about 1e-14 off the plane
    occ, mean, cov = whole_data_stats(x)
    s = np.linalg.eigvalsh(np.cov(x.astype(np.float64).T, bias=True))
    assert s[D - rank] > 0.01 and s[D - rank - 1] < 1e-9
    for max_condition, variance_floor in ((1e5, 1e-3), (1e5, 0.005), (100.0, 1e-3)):
        floor = max(variance_floor, s.max() / max_condition)
        want = int((s < floor).sum())
        assert want >= D - rank
        est = T.fgmm_est(*one_gaussian(D), occ, mean, cov, max_condition=max_condition, variance_floor=variance_floor)
        assert est["floored"] == (want, 1)
        got = np.sort(np.linalg.eigvalsh(moments(est, D)[1][0]))
        np.testing.assert_allclose(got, np.sort(np.maximum(s, floor)), rtol=1e-4)
        np.testing.assert_allclose(got[:want], floor, rtol=1e-4)
        assert ("WARNING", "%d variances floored in 1 Gaussians." % want) in est["log"]
    assert T.fgmm_est(*one_gaussian(D), occ, mean, cov)["floored"] == (D - rank, 1)   # the defaults floor exactly the null space


def test_removal_and_the_last_gaussian_is_kept():
    w, means, b, ic = R.random_full_model(3, 3, 4)
    x = R.frames_around(4, means[:1], 500)
    frame = np.arange(500)
    # Gaussian 0 has everything, 1 has two frames' worth, 2 nothing
    gauss = np.zeros(500, np.int64)
    gauss[:2] = 1
    occ, mean, cov = T.acc_stats(x, frame, gauss, np.ones(500, F), 3, 7)
    est = T.fgmm_est(w, b, ic, occ, mean, cov)
    assert est["removed"] == [1, 2] and len(est["weights"]) == 1 and est["weights"][0] == 1.0
    assert [t for l, t in est["log"] if "removing Gaussian" in t] == [
        "Too little data - removing Gaussian (weight 0.004, occupation count 2, vector size 4)",
        "Too little data - removing Gaussian (weight 0, occupation count 0, vector size 4)"]
    kept = T.fgmm_est(w, b, ic, occ, mean, cov, remove_low_count_gaussians=False)
    assert kept["removed"] == [] and len(kept["weights"]) == 3
    np.testing.assert_allclose(kept["weights"], np.array([0.996, 0.004, 1e-5]) / (1.0 + 1e-5), rtol=1e-6)
    assert np.array_equal(kept["inv_covars"][1:], ic[1:]) and np.array_equal(kept["means_invcovars"][1:], b[1:])
    # nothing has enough data: the first G - 1 go, the last one stays as it was
    est = T.fgmm_est(w, b, ic, occ, mean, cov, min_gaussian_occupancy=1000.0)
    assert est["removed"] == [0, 1] and est["weights"].tolist() == [1.0]
    assert np.array_equal(est["inv_covars"][0], ic[2]) and np.array_equal(est["means_invcovars"][0], b[2])
    assert any("it is the last Gaussian: i = 2" in t for _, t in est["log"])


def test_update_flags_v_alone_applies_the_mean_shift_correction():
    rng = np.random.default_rng(5)
    D = 3
    x = (rng.normal(size=(600, D)) * [1.0, 2.0, 0.5] + [4.0, -1.0, 0.0]).astype(F)
    occ, mean, cov = whole_data_stats(x)
    w, b, ic = one_gaussian(D)   # the old mean is 0
    est = T.fgmm_est(w, b, ic, occ, mean, cov, update_flags="v")
    mu, sig = moments(est, D)
    x64 = x.astype(np.float64)
    np.testing.assert_allclose(mu[0], 0.0, atol=1e-6)                      # the mean is kept ...
    np.testing.assert_allclose(sig[0], x64.T @ x64 / 600, rtol=1e-4)     # ... and the covariance is taken about it
    m = x64.mean(0)
    np.testing.assert_allclose(sig[0], np.cov(x64.T, bias=True) + np.outer(m, m), rtol=1e-4)
    # m alone: the covariance stays the identity
    est = T.fgmm_est(w, b, ic, occ, mean, cov, update_flags="m")
    mu, sig = moments(est, D)
    np.testing.assert_allclose(mu[0], m, rtol=1e-5)
    assert np.array_equal(est["inv_covars"], ic)


def test_flags_are_augmented_and_gate_the_accumulators():
    assert [T.augment_flags(T.parse_flags(s)) for s in ("w", "m", "v", "mw", "vw", "mvw")] == [4, 5, 7, 5, 7, 7]
    x = np.arange(12, dtype=F).reshape(4, 3)
    occ, mean, cov = T.acc_stats(x, [0, 1, 3], [1, 1, 0], [0.5, 0.25, 1.0], 2, T.parse_flags("w"))
    assert occ.tolist() == [1.0, 0.75] and not mean.any() and not cov.any()
    occ, mean, cov = T.acc_stats(x, [0, 1, 3], [1, 1, 0], [0.5, 0.25, 1.0], 2, T.parse_flags("m"))
    assert mean[1].tolist() == [0.75, 1.5, 2.25] and not cov.any()
    occ, mean, cov = T.acc_stats(x, [0, 1, 3], [1, 1, 0], [0.5, 0.25, 1.0], 2, T.parse_flags("v"))
    assert np.array_equal(R.unpack(cov[0], 3), np.outer(x[3], x[3]))


def test_the_accumulator_file_round_trips():
    rng = np.random.default_rng(6)
    occ, mean, cov = rng.uniform(1, 9, 3), rng.normal(size=(3, 4)), rng.normal(size=(3, 10))
    for binary in (True, False):
        for flags in (4, 5, 7):
            got = T.read_accs(T.accs_bytes(occ, mean, cov, flags, binary))
            assert (got["dim"], got["num_gauss"], got["flags"]) == (4, 3, flags)
            assert np.array_equal(got["occ"], occ.astype(F)) and np.array_equal(got["mean"], mean.astype(F))
            assert np.array_equal(got["cov"], cov.astype(F) if flags & 2 else np.zeros((3, 10), F))


def test_two_em_passes_do_not_lower_the_likelihood():
    w, means, b, ic = R.random_full_model(7, 4, 5)
    x = R.frames_around(8, means, 1500, noise=1.5)
    # start from a perturbed model; all 4 Gaussians are selected, so this is exact EM and the likelihood cannot fall
    start = R.random_full_model(9, 4, 5, spread=2.0)
    w, b, ic = start[0], start[2], start[3]
    likes = []
    for _ in range(3):
        occ, mean, cov, ll = T.e_step(x, w, b, ic, 4)
        likes.append(ll / len(x))
        est = T.fgmm_est(w, b, ic, occ, mean, cov, remove_low_count_gaussians=False, min_gaussian_occupancy=1.0)
        assert est["objf_after"] >= est["objf_before"]
        w, b, ic = est["weights"], est["means_invcovars"], est["inv_covars"]
    assert likes[1] >= likes[0] and likes[2] >= likes[1], likes
