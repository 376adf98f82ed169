"""The host side of i-vector extractor training (ivector-extractor-init, -sum-accs, -est and the statistics file) through the C ABI
and the binaries, against the restatement (tests/ivector_train_ref.py).  No device is opened."""
import os
import subprocess

import numpy as np
import pytest

import helpers as H
import ivector_ref as R
import ivector_train_ref as T
import ubm_ref as UR

P = H.pkg()
BIN = os.path.join(H.ROOT, H.PKG_NAME, "bin")
U53 = 2.0 ** -53


def run(args, stdin=None):
    env = dict(os.environ, PATH=BIN + os.pathsep + os.environ.get("PATH", ""), HIP_VISIBLE_DEVICES="")
    return subprocess.run([os.path.join(BIN, args[0])] + list(args[1:]), input=stdin, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, timeout=120)


def ubm(seed=2, G=4, D=5):
    rng = np.random.default_rng(seed)
    w = rng.uniform(0.5, 1.5, G)
    ic = np.zeros((G, D * (D + 1) // 2), np.float32)
    for g in range(G):
        A = rng.normal(size=(D, D))
        ic[g] = R.pack(A @ A.T / D + np.eye(D)).astype(np.float32)
    return (w / w.sum()).astype(np.float32), rng.normal(size=(G, D)).astype(np.float32), ic


# ------------------------------------------------------------------------------------------------------------------- init
def test_ivex_init_repeats_for_a_seed_and_starts_from_the_ubm_means():
    w, b, ic = ubm()
    a1, a2, other = P.ivex_init(w, b, ic, 7, seed=3), P.ivex_init(w, b, ic, 7, seed=3), P.ivex_init(w, b, ic, 7, seed=4)
    assert a1["M"].tobytes() == a2["M"].tobytes() and a1["M"].tobytes() != other["M"].tobytes()
    assert a1["prior_offset"] == 100.0
    assert np.array_equal(a1["w_vec"], w.astype(np.float64)) and np.array_equal(a1["sigma_inv"], ic.astype(np.float64))
    for g in range(4):
        sinv = R.unpack(ic[g].astype(np.float64), 5)
        mean = np.linalg.solve(sinv, b[g].astype(np.float64))
        tol = np.linalg.cond(sinv) * 5 * 8 * U53 * np.linalg.norm(mean)   # a solve through Cholesky and one through LU, 5 x 5
        assert np.all(np.abs(a1["M"][g][:, 0] * 100.0 - mean) <= tol)
    # the documented generator: the other columns are its draws (libm's log and cos may differ in the last place or two)
    want = T.init_normal(3, 4 * 5 * 7).reshape(4, 5, 7)
    assert np.all(np.abs(a1["M"][:, :, 1:] - want[:, :, 1:]) <= 8 * U53 * np.maximum(np.abs(want[:, :, 1:]), 1.0))
    assert np.array_equal(other["M"][:, :, 0], a1["M"][:, :, 0])


def test_ivector_extractor_init_the_binary_writes_a_model_and_refuses_weights(tmp_path):
    w, b, ic = ubm()
    src, dst = tmp_path / "final.ubm", tmp_path / "0.ie"
    src.write_bytes(UR.full_gmm_bytes(w, b, ic))
    r = run(["ivector-extractor-init", "--ivector-dim=6", "--use-weights=false", "--seed=9", str(src), str(dst)])
    assert r.returncode == 0, r.stderr
    got = P.ivex_read(str(dst))
    want = P.ivex_init(w, b, ic, 6, seed=9)
    assert got["M"].tobytes() == want["M"].tobytes() and got["prior_offset"] == 100.0
    r = run(["ivector-extractor-init", "--use-weights=true", str(src), str(dst)])
    assert r.returncode == 255 and b"--use-weights=true is not built" in r.stderr
    r = run(["ivector-extractor-init", "--ivector-dim=1025", str(src), str(dst)])
    assert r.returncode == 255 and b"1025" in r.stderr and b"1024" in r.stderr


# ------------------------------------------------------------------------------------------------------------------- the file
def small_stats(seed, G=3, D=4, S=5, variances=True):
    rng = np.random.default_rng(seed)
    st = T.zero_stats(G, D, S, variances)
    for k in ("gamma", "Y", "R", "S", "ivector_sum", "ivector_scatter"):
        if st[k] is not None:
            st[k] = rng.normal(size=st[k].shape)
    st["num_ivectors"], st["auxf"], st["frames"] = 17.0, float(rng.normal()), float(rng.uniform(10, 20))
    return st


def same_stats(a, b):
    return all((a[k] is None and b[k] is None) or np.array_equal(a[k], b[k]) for k in a)


@pytest.mark.parametrize("variances", [True, False])
def test_the_statistics_file_round_trips_binary_text_binary(tmp_path, variances):
    st = small_stats(1, variances=variances)
    b1, t1, b2 = (str(tmp_path / n) for n in ("a.acc", "a.txt", "b.acc"))
    P.ivex_stats_write(b1, st, binary=True)
    assert same_stats(P.ivex_stats_read(b1), st)
    r = run(["ivector-extractor-sum-accs", "--binary=false", b1, t1])
    assert r.returncode == 0, r.stderr
    assert open(t1, "rb").read(2) != b"\0B"
    r = run(["ivector-extractor-sum-accs", "--binary=true", t1, b2])
    assert r.returncode == 0, r.stderr
    assert open(b1, "rb").read() == open(b2, "rb").read()


def test_sum_accs_adds_in_argument_order_and_writes_to_its_last_argument(tmp_path):
    sts = [small_stats(s) for s in (1, 2, 3)]
    for st, scale in zip(sts, (1.0, 1e16, -1e16)):   # an order of addition shows in the bits
        st["gamma"] = st["gamma"] * scale
    names = [str(tmp_path / ("%d.acc" % i)) for i in range(3)]
    for n, st in zip(names, sts):
        P.ivex_stats_write(n, st)
    out = str(tmp_path / "sum.acc")
    r = run(["ivector-extractor-sum-accs", "--parallel=true", names[0], names[1], "cat %s |" % names[2], out])
    assert r.returncode == 0, r.stderr
    got = P.ivex_stats_read(out)
    want = T.add_stats(T.add_stats(sts[0], sts[1]), sts[2])
    assert same_stats(got, want)
    assert not np.array_equal(got["gamma"], sts[0]["gamma"] + (sts[1]["gamma"] + sts[2]["gamma"]))
    for n, st in zip(names, sts):
        assert same_stats(P.ivex_stats_read(n), st)   # the inputs are inputs
    P.ivex_stats_write(names[1], small_stats(4, S=6))
    r = run(["ivector-extractor-sum-accs", names[0], names[1], out])
    assert r.returncode == 255 and b"cannot be added" in r.stderr


# ------------------------------------------------------------------------------------------------------------------- est
def generated_stats(seed, G, D, S, n_utts, low_count=None, rank_deficient=False):
    """statistics of random utterances through the restatement; low_count: that Gaussian is never hit; rank_deficient: the
    utterances are so few that R_g has eigenvalues under lambda_max / 1e4"""
    rng = np.random.default_rng(seed)
    model = R.random_model(seed + 100, G, D, S)
    if rank_deficient:
        model["prior_offset"] = 1000.0   # m m' dominates the scatter: cond(R_g) is far above 1e4 and the floor is live
    utts = []
    for u in range(n_utts):
        frames = int(rng.integers(20, 40))
        x = (rng.normal(size=(frames, D)) * 2).astype(np.float32)
        post = []
        for _ in range(frames):
            g = int(rng.integers(0, G))
            if low_count is not None and g == low_count:
                g = (g + 1) % G
            post.append((np.array([g], np.int32), np.array([1.0], np.float32)))
        utts.append((x, post))
    return model, T.accumulate(utts, model)


def check_est(model, st, **opts):
    """M, Sigma^-1 and the prior offset of the library against the restatement's.  What is compared of M is what the prior update
    leaves determined: column 0 and M M' (the other columns are fixed up to the signs and, among equal eigenvalues, rotations of
    eigenvectors).  Bounds, u = 2^-53:
      M        the update solves with R_g through an eigen-decomposition: relative error cond(R_g) S u per Householder/QL sweep, 8 for
               the sweeps; the prior transform adds the same with cond(C), the i-vector covariance.
      Sigma^-1 raw_g inherits M's relative error through M R M' and Y M' (4 products), the inverse multiplies by cond(Sigma_g), and
               the floor's eigen-decomposition adds cond(F) D u.
      the improvements (log lines) are differences of objectives: each moves by the relative error of what it is made of (M for the
               projections, twice, since it is quadratic; Sigma^-1 for the variances; the eigenvalues of C, relative error
               8 cond(C) S u each, for the prior, S logarithms of them) times the sum of the absolute values of its terms."""
    want = T.m_step(st, model, **opts)
    got = P.ivex_est(st, model["w_vec"], model["M"], model["sigma_inv"], model["prior_offset"], **opts)
    G, D, S = model["M"].shape
    for k in ("eig_floored", "var_floored", "var_floored_gauss", "prior_floored"):
        assert got[k] == want[k], k
    assert got["gauss_updated"] == int(want["updated"].sum()) and got["gauss_skipped"] == G - int(want["updated"].sum())
    cond_c = np.linalg.cond(want["C"])
    assert abs(got["prior_offset"] - want["prior_offset"]) <= 8 * cond_c * S * U53 * want["prior_offset"]
    worst = eps_m_max = eps_s_max = 0.0
    for g in range(G):
        eps_m = 8 * (want["cond_R"][g] + cond_c) * S * U53
        a, b = got["M"][g], want["M"][g]
        nm = np.linalg.norm(b)
        e0 = np.abs(a[:, 0] - b[:, 0]).max() / (eps_m * nm)
        e1 = np.abs(a @ a.T - b @ b.T).max() / (2 * eps_m * nm * nm)
        sg, sw = R.unpack(got["sigma_inv"][g], D), R.unpack(want["sigma_inv"][g], D)
        cond_s = np.linalg.cond(sw)
        cond_f = np.linalg.cond(want["F"]) if want["F"] is not None else 1.0
        eps_s = cond_s * (4 * eps_m * max(1.0, np.abs(st["Y"][g]).sum() * nm / max(np.linalg.norm(want["raw"][g]), 1e-300)) + 8 * cond_f * D * U53)
        e2 = np.abs(sg - sw).max() / (eps_s * np.linalg.norm(sw))
        worst = max(worst, e0, e1, e2)
        assert e0 <= 1 and e1 <= 1 and e2 <= 1, (g, e0, e1, e2)
        if want["updated"][g]:
            eps_m_max, eps_s_max = max(eps_m_max, eps_m), max(eps_s_max, eps_s)
    eps_c = 8 * cond_c * S * U53
    tol = dict(impr_proj=(4 * eps_m_max + 8 * S * U53) * want["abs_proj"], impr_var=(4 * eps_s_max + 8 * D * U53) * want["abs_var"],
               impr_prior=eps_c * want["abs_prior"] + 0.5 * S * eps_c * want["num_ivectors"] / want["frames"])
    for k in ("impr_proj", "impr_var", "impr_prior"):
        worst = max(worst, abs(got[k] - want[k]) / max(tol[k], 1e-300))
        assert abs(got[k] - want[k]) <= tol[k], (k, got[k], want[k], tol[k])
    print("worst error / bound %.3g" % worst)
    return got, want


@pytest.mark.parametrize("shape", [(3, 4, 5), (5, 7, 17)])
def test_ivex_est_matches_the_restatement(shape):
    G, D, S = shape
    model, st = generated_stats(5, G, D, S, 60 * S)
    got, want = check_est(model, st, gaussian_min_count=100.0)
    assert got["gauss_skipped"] == 0 and got["eig_floored"] == 0


@pytest.mark.parametrize("shape", [(3, 4, 5), (5, 7, 17)])
def test_a_gaussian_below_the_minimum_count_is_left_alone(shape):
    G, D, S = shape
    model, st = generated_stats(6, G, D, S, 60 * S, low_count=1)
    got = P.ivex_est(st, model["w_vec"], model["M"], model["sigma_inv"], model["prior_offset"], diagonalize=False)
    assert got["gauss_skipped"] == 1 and got["gauss_updated"] == G - 1
    assert np.array_equal(got["sigma_inv"][1], model["sigma_inv"][1])
    # its projection only goes through the prior transform: M_g V^-1, V of the result
    np.testing.assert_allclose(got["M"][1] @ got["V"], model["M"][1], rtol=0, atol=64 * S * U53 * np.linalg.cond(got["V"]) * np.abs(model["M"][1]).max())
    check_est(model, st)


@pytest.mark.parametrize("shape", [(3, 4, 5), (5, 7, 17)])
def test_eigenvalues_of_the_quadratic_statistics_are_floored(shape):
    G, D, S = shape
    model, st = generated_stats(7, G, D, S, 12 * G, rank_deficient=True)
    got, want = check_est(model, st, gaussian_min_count=10.0)
    assert got["eig_floored"] > 0


@pytest.mark.parametrize("shape", [(3, 4, 5), (5, 7, 17)])
def test_a_variance_is_floored(shape):
    G, D, S = shape
    model, st = generated_stats(8, G, D, S, 60 * S)
    # one Gaussian whose residual covariance is small beside the others': half of S_0 - M_0 R_0 M_0' is taken away
    st["S"][0] = 0.5 * st["S"][0] + 0.5 * R.pack(model["M"][0] @ R.unpack(st["R"][0], S) @ model["M"][0].T)
    got, want = check_est(model, st, variance_floor_factor=0.9)
    assert got["var_floored"] > 0


@pytest.mark.parametrize("shape", [(3, 4, 5), (5, 7, 17)])
@pytest.mark.parametrize("diagonalize", [True, False])
def test_the_prior_transform_whitens_the_ivectors(shape, diagonalize):
    G, D, S = shape
    model, st = generated_stats(9, G, D, S, 60 * S)
    got = P.ivex_est(st, model["w_vec"], model["M"], model["sigma_inv"], model["prior_offset"], diagonalize=diagonalize)
    n = st["num_ivectors"]
    mu = st["ivector_sum"] / n
    C = R.unpack(st["ivector_scatter"], S) / n - np.outer(mu, mu)
    V = got["V"]
    tol = 8 * np.linalg.cond(C) * S * U53
    e0 = np.eye(S)[0]
    assert np.abs(V @ mu - got["prior_offset"] * e0).max() <= tol * np.linalg.norm(V, 2) * np.linalg.norm(mu)
    assert np.abs(V @ C @ V.T - np.eye(S)).max() <= tol * np.linalg.norm(V, 2) ** 2 * np.linalg.norm(C, 2)
    if diagonalize:   # the averaged quadratic term is diagonal in dimensions 1 .., descending
        A = sum(model["w_vec"][g] * got["M"][g].T @ R.unpack(got["sigma_inv"][g], D) @ got["M"][g] for g in range(G))[1:, 1:]
        d = np.diag(A)
        # M V^-1 carries a relative error S u of |M| |V^-1|, cond(V) beside |M V^-1|; it enters A twice, and the eigenvectors' own
        # residual is 8 S u |A|
        tol_d = (4 * np.linalg.cond(V) + 8) * S * U53 * d.max()
        assert np.all(np.diff(d) <= tol_d) and np.abs(A - np.diag(d)).max() <= tol_d


def test_ivex_est_with_threads_gives_the_same_bits():
    model, st = generated_stats(5, 5, 7, 17, 300)
    a = P.ivex_est(st, model["w_vec"], model["M"], model["sigma_inv"], model["prior_offset"], num_threads=1)
    b = P.ivex_est(st, model["w_vec"], model["M"], model["sigma_inv"], model["prior_offset"], num_threads=3)
    assert a["M"].tobytes() == b["M"].tobytes() and a["sigma_inv"].tobytes() == b["sigma_inv"].tobytes() and a["prior_offset"] == b["prior_offset"]


def test_ivector_extractor_est_the_binary_matches_the_library(tmp_path):
    model, st = generated_stats(5, 3, 4, 5, 300)
    ie, acc, out = (str(tmp_path / n) for n in ("0.ie", "0.acc", "1.ie"))
    P.ivex_write(ie, model["w_vec"], model["M"], model["sigma_inv"], model["prior_offset"])
    P.ivex_stats_write(acc, st)
    r = run(["ivector-extractor-est", "--num-threads=2", "--variance-floor-factor=0.05", "--gaussian-min-count=50", ie, acc, out])
    assert r.returncode == 0, r.stderr
    assert b"variances floored in" in r.stderr and b"Overall objective-function improvement per frame was" in r.stderr
    got = P.ivex_read(out)
    want = P.ivex_est(st, model["w_vec"], model["M"], model["sigma_inv"], model["prior_offset"], variance_floor_factor=0.05, gaussian_min_count=50.0)
    assert got["M"].tobytes() == want["M"].tobytes() and got["sigma_inv"].tobytes() == want["sigma_inv"].tobytes()
    assert got["prior_offset"] == want["prior_offset"]


def test_shapes_that_do_not_agree_and_limits_are_errors_that_name_them():
    model, st = generated_stats(5, 3, 4, 5, 20)
    with pytest.raises(P.XvError, match="not the model's"):
        P.ivex_est(st, model["w_vec"][:2], model["M"][:2], model["sigma_inv"][:2], 1.0)
    w, b, ic = ubm()
    with pytest.raises(P.XvError, match="1024"):
        P.ivex_init(w, b, ic, 1025)
    wide = np.zeros((1, 97 * 98 // 2), np.float32)
    wide[0, [i * (i + 1) // 2 + i for i in range(97)]] = 1.0
    with pytest.raises(P.XvError, match="97 is above .* limit of 96"):
        P.ivex_init(np.ones(1, np.float32), np.zeros((1, 97), np.float32), wide, 4)
    with pytest.raises(P.XvError, match="97 is above .* limit of 96"):
        P.ivex_stats_write("/dev/null", T.zero_stats(1, 97, 2))
    empty = T.zero_stats(3, 4, 5)
    with pytest.raises(P.XvError, match="no i-vector"):
        P.ivex_est(empty, model["w_vec"], model["M"], model["sigma_inv"], 1.0)


def test_acc_stats_needs_a_gpu(tmp_path):
    model = R.random_model(1, 3, 4, 5)
    ie = str(tmp_path / "0.ie")
    P.ivex_write(ie, model["w_vec"], model["M"], model["sigma_inv"], model["prior_offset"])
    r = run(["ivector-extractor-acc-stats", ie, "ark:/dev/null", "ark:/dev/null", str(tmp_path / "x.acc")])
    assert r.returncode == 255 and b"no HIP device available" in r.stderr
