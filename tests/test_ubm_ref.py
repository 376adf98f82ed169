"""The numpy restatement of the GMM-UBM stage (tests/ubm_ref.py) against closed forms."""
import numpy as np

import ubm_ref as R


def test_window_two_scales_are_the_regression_weights_and_their_self_convolution():
    s = R.delta_scales(2, 2)
    assert s[0].tolist() == [1.0]
    first = (np.array([-2, -1, 0, 1, 2], np.float32) * np.float32(1.0 / 10.0)).astype(np.float32)
    assert np.array_equal(s[1], first)
    assert s[2].shape == (9,)
    np.testing.assert_allclose(s[2], np.convolve(first.astype(np.float64), first.astype(np.float64)), rtol=0, atol=2e-8)


def test_deltas_of_a_ramp_are_constant_away_from_the_edges():
    T, W = 40, 3
    x = (np.arange(T, dtype=np.float32)[:, None] * np.array([1.0, -0.5, 4.0], np.float32)[None]).astype(np.float32)
    out = R.add_deltas(x, order=2, window=W)
    assert out.shape == (T, 9) and out.dtype == np.float32
    assert np.array_equal(out[:, :3], x)
    np.testing.assert_allclose(out[W:T - W, 3:6], np.broadcast_to([1.0, -0.5, 4.0], (T - 2 * W, 3)), rtol=1e-6)
    np.testing.assert_allclose(out[2 * W:T - 2 * W, 6:9], 0.0, atol=1e-5)
    assert not np.allclose(out[0, 3:6], [1.0, -0.5, 4.0])   # the edge repeats the first frame
    assert R.add_deltas(x, order=1, window=2, truncate=2).shape == (T, 4)


def test_the_diagonal_score_is_the_gaussian_log_density():
    rng = np.random.default_rng(1)
    G, D, T = 5, 4, 7
    w = rng.uniform(0.1, 1.0, G)
    mu, var = rng.normal(size=(G, D)), rng.uniform(0.5, 2.0, (G, D))
    x = rng.normal(size=(T, D))
    gc = R.diag_gconsts(w, mu / var, 1.0 / var)
    got = R.diag_loglikes(x, gc, mu / var, 1.0 / var)
    want = np.array([[np.log(w[g]) + sum(-0.5 * np.log(2 * np.pi * var[g, d]) - 0.5 * (x[t, d] - mu[g, d]) ** 2 / var[g, d] for d in range(D))
                      for g in range(G)] for t in range(T)])
    np.testing.assert_allclose(got, want, rtol=1e-12, atol=1e-12)
    sel = R.gselect(got, 3)
    assert all(sorted(got[t], reverse=True)[:3] == got[t, sel[t]].tolist() for t in range(T))


def test_a_full_model_with_diagonal_covariances_scores_like_its_diagonal_image():
    rng = np.random.default_rng(2)
    G, D, T = 4, 5, 9
    w = rng.uniform(0.1, 1.0, G)
    mu, var = rng.normal(size=(G, D)), rng.uniform(0.5, 2.0, (G, D))
    ic = np.stack([R.pack(np.diag(1.0 / var[g])) for g in range(G)])
    b = mu / var
    gc_d, mi, iv = R.fgmm_to_gmm(w, b, ic)
    np.testing.assert_allclose(mi, b, rtol=1e-12)
    np.testing.assert_allclose(iv, 1.0 / var, rtol=1e-12)
    gc_f = R.full_gconsts(w, b, ic)
    np.testing.assert_allclose(gc_f, gc_d, rtol=1e-12)
    x = rng.normal(size=(T, D))
    sel = np.tile(np.arange(G, dtype=np.int32), (T, 1))
    np.testing.assert_allclose(R.full_loglikes(x, gc_f, b, ic, sel), R.diag_loglikes(x, gc_d, mi, iv), rtol=1e-11, atol=1e-11)


def test_posteriors_sum_to_one_and_follow_the_min_post_rule():
    ll = np.log(np.array([[0.5, 0.3, 0.15, 0.05], [0.4, 0.3, 0.2, 0.1], [0.97, 0.01, 0.01, 0.01]]))
    p, logsum = R.posteriors(ll + 7.0)
    np.testing.assert_allclose(p.sum(1), 1.0, rtol=1e-14)
    np.testing.assert_allclose(logsum, 7.0, rtol=1e-14)
    p, _ = R.posteriors(ll, min_post=0.12)
    np.testing.assert_allclose(p[0], np.array([0.5, 0.3, 0.15, 0.0]) / 0.95, rtol=1e-12)
    np.testing.assert_allclose(p[1], np.array([0.4, 0.3, 0.2, 0.0]) / 0.9, rtol=1e-12)
    np.testing.assert_allclose(p[2], [1.0, 0.0, 0.0, 0.0], rtol=1e-12)
    # everything pruned: the arg-max takes it all
    p, _ = R.posteriors(ll[1:2], min_post=0.6)
    assert p.tolist() == [[1.0, 0.0, 0.0, 0.0]]


def test_a_frame_whose_largest_score_is_not_finite_has_no_posterior():
    """csrc/ubm.h: such a frame has zero entries, every slot posterior is 0 and the log-sum is the largest value as computed;
    every other row, one that mixes -inf with finite scores included, is what it is without the bad rows."""
    inf = np.inf
    good = np.log(np.array([[0.5, 0.3, 0.15, 0.05], [0.4, 0.3, 0.2, 0.1], [0.97, 0.01, 0.01, 0.01]])) + 7.0
    mixed = np.array([[-inf, 2.0, -inf, 1.0]])
    ll = np.concatenate([good[:1], np.full((1, 4), -inf), good[1:2], [[1.0, np.nan, 2.0, 3.0]], mixed, np.full((1, 4), np.nan), good[2:]])
    bad = [1, 3, 5]
    rest = np.delete(ll, bad, axis=0)
    for min_post in (0.0, 0.12, 0.6):
        with np.errstate(all="raise"):   # the rule is stated, not an accident of inf - inf
            p, logsum = R.posteriors(ll, min_post)
            p_rest, logsum_rest = R.posteriors(rest, min_post)
        assert p.shape == ll.shape and not np.isnan(p).any()
        assert not p[bad].any()
        assert np.isneginf(logsum[1]) and np.isnan(logsum[3]) and np.isnan(logsum[5])
        assert np.array_equal(np.delete(p, bad, axis=0), p_rest) and np.array_equal(np.delete(logsum, bad), logsum_rest)
        np.testing.assert_allclose(p_rest.sum(1), 1.0, rtol=1e-14)
    # the -inf slots of a mixed row are at 0 and the log-sum is that of the finite ones
    p, logsum = R.posteriors(mixed)
    e = np.exp(-1.0)
    np.testing.assert_allclose(p[0], [0.0, 1.0 / (1.0 + e), 0.0, e / (1.0 + e)], rtol=1e-14)
    assert p[0, 0] == 0.0 and p[0, 2] == 0.0
    np.testing.assert_allclose(logsum, 2.0 + np.log1p(e), rtol=1e-14)
    # a batch without a bad row takes the old path: the same values as before the rule
    p, logsum = R.posteriors(good, 0.12)
    np.testing.assert_allclose(p[0], np.array([0.5, 0.3, 0.15, 0.0]) / 0.95, rtol=1e-12)
    np.testing.assert_allclose(logsum, 7.0, rtol=1e-14)


def test_the_files_round_trip_through_the_restatement():
    w, means, b, ic = R.random_full_model(3, 3, 4)
    for binary in (True, False):
        m = R.read_full_gmm(R.full_gmm_bytes(w, b, ic, binary))
        tol = 0 if binary else 1e-7
        np.testing.assert_allclose(m["inv_covars"], ic, rtol=tol)
        np.testing.assert_allclose(m["means_invcovars"], b, rtol=tol)
        d = R.read_diag_gmm(R.diag_gmm_bytes(w, b, np.abs(b) + 1, binary, gconsts=w))
        np.testing.assert_allclose(d["inv_vars"], np.abs(b) + 1, rtol=tol)
        assert "gconsts" in d
        sel = [("a", [[1, 2], [3, 4]]), ("b", [[5, 6]])]
        assert R.read_gselect_table(R.gselect_table_bytes(sel, binary)) == sel
        post = [("a", [[(1, 0.5), (2, 0.5)], []]), ("b", [[(7, 1.0)]])]
        assert R.read_post_table(R.post_table_bytes(post, binary)) == post
