"""CPU self-checks of the numpy restatement of diagonal UBM training (tests/dubm_train_ref.py)."""
import numpy as np

import dubm_train_ref as T
import ubm_ref as R

F = np.float32


def test_generator_is_splitmix_and_streams_are_disjoint():
    # splitmix64's first output for state 0 + golden ratio, shifted to 53 bits
    assert T.mix(1, 0) == 0xE220A8397B1DCDAF >> 11
    assert T.mix(0, 5) != T.mix(0, 6) and T.mix(3, 5) == T.mix(3, 5)
    draws = [T.gauss(7, e) for e in range(4000)]
    assert abs(np.mean(draws)) < 0.06 and abs(np.std(draws) - 1.0) < 0.05
    assert len({T.ENTRY_SAMPLE >> 60, T.ENTRY_INIT >> 60, T.ENTRY_SPLIT >> 60}) == 3


def test_sampling_keeps_the_head_then_replaces_uniformly():
    x = np.arange(5000, dtype=F).reshape(-1, 1)
    kept, read = T.sample_frames(x, 100, 3)
    assert read == 5000 and kept.shape == (100, 1) and len(np.unique(kept)) == 100
    assert T.sample_frames(x[:60], 100, 3)[0].shape == (60, 1)
    assert np.array_equal(kept, T.sample_frames(x, 100, 3)[0]) and not np.array_equal(kept, T.sample_frames(x, 100, 4)[0])
    # a reservoir: about num_frames / T of every part of the stream survives
    assert 25 < (kept >= 2500).sum() < 75


def test_initialisation_draws_distinct_frames_and_the_global_variance():
    rng = np.random.default_rng(0)
    x = rng.normal(2.0, 3.0, size=(400, 5)).astype(F)
    w, mi, iv, frames = T.init_from_frames(x, 16, 9)
    assert len(set(frames)) == 16 and np.allclose(w.sum(), 1.0)
    assert np.allclose(1.0 / iv[0], x.astype(np.float64).var(0), rtol=1e-5)
    assert np.allclose(mi / iv, x[frames], rtol=1e-5, atol=1e-6)


def test_chain_scores_are_exact_on_integers_and_within_the_bound_otherwise():
    rng = np.random.default_rng(1)
    G, D = 9, 17
    gc = (rng.integers(-8, 9, G) + np.arange(G) * 2.0 ** -12).astype(F)
    mi, iv = rng.integers(-3, 4, (G, D)).astype(F), (2.0 ** rng.integers(0, 3, (G, D))).astype(F)
    x = rng.integers(-4, 5, (50, D)).astype(F)
    assert np.array_equal(T.chain_scores(x, gc, mi, iv).astype(np.float64), R.diag_loglikes(x, gc, mi, iv))
    x = rng.normal(0, 2, (50, D)).astype(F)
    mi, iv = rng.normal(0, 1, (G, D)).astype(F), rng.uniform(0.5, 2, (G, D)).astype(F)
    err = np.abs(T.chain_scores(x, gc, mi, iv) - R.diag_loglikes(x, gc, mi, iv))
    assert np.all(err <= T.score_bound(x, gc, mi, iv)) and err.max() > 0


def test_sparse_and_dense_statistics_agree_and_the_flags_gate():
    rng = np.random.default_rng(2)
    x = rng.normal(size=(40, 3)).astype(F)
    post = rng.uniform(size=(40, 4)).astype(F)
    post[:, 2] = 0
    t, g = np.nonzero(np.ones_like(post))
    a = T.acc_stats(x, t, g, post.reshape(-1), 4)
    b = T.dense_stats(x, post)
    for u, v in zip(a, b):
        assert np.allclose(u, v, rtol=1e-12, atol=1e-12)
    assert not a[0][2] and T.abs_terms(x, t, g, post.reshape(-1), 4)[3].tolist() == [40, 40, 0, 40]
    occ, mean, var = T.acc_stats(x, t, g, post.reshape(-1), 4, T.parse_flags("m"))
    assert mean.any() and not var.any()
    bo, bm, bv = T.weighted_error_bound(x, post.astype(np.float64), np.zeros(40))
    assert bo.shape == (4,) and bm.shape == bv.shape == (4, 3) and bo[2] == 0 and np.all(bo[[0, 1, 3]] > 0)


def test_m_step_recovers_the_sample_moments_and_handles_low_counts():
    rng = np.random.default_rng(3)
    D = 4
    parts = [rng.normal(m, s, size=(n, D)).astype(F) for m, s, n in ((0, 1, 300), (5, 2, 200), (-4, 0.5, 5))]
    x = np.concatenate(parts)
    g = np.repeat([0, 1, 2], [300, 200, 5])
    occ, mean, var = T.acc_stats(x, np.arange(len(x)), g, np.ones(len(x), F), 3)
    w0, mi0, iv0 = np.full(3, 1 / 3, F), np.zeros((3, D), F), np.ones((3, D), F)
    out = T.dgmm_est(w0, mi0, iv0, occ, mean, var)
    assert out["removed"] == [2] and len(out["weights"]) == 2 and abs(out["weights"].sum() - 1) < 1e-6
    assert np.allclose(out["means_invvars"][1] / out["inv_vars"][1], parts[1].mean(0), rtol=1e-4)
    assert np.allclose(1 / out["inv_vars"][1], parts[1].astype(np.float64).var(0), rtol=1e-4)
    assert out["objf_after"] > out["objf_before"] and out["log"][0][1].startswith("Too little data - removing Gaussian")
    kept = T.dgmm_est(w0, mi0, iv0, occ, mean, var, remove_low_count_gaussians=False)
    assert kept["removed"] == [] and "remove-low-count-gaussians == false: i = 2" in kept["log"][0][1]
    assert np.array_equal(kept["inv_vars"][2], iv0[2])
    floored = T.dgmm_est(w0, mi0, iv0, occ, mean, var, min_variance=1.0)
    assert floored["floored"][1] >= 1 and np.all(floored["inv_vars"] <= 1.0)
    only_w = T.dgmm_est(w0, mi0, iv0, occ, mean, var, update_flags="w")
    assert np.array_equal(only_w["means_invvars"], mi0[:2]) and np.array_equal(only_w["inv_vars"], iv0[:2])


def test_split_halves_the_largest_weight_and_moves_the_means_apart():
    w, mi, iv = np.array([0.5, 0.3, 0.2], F), np.arange(6, dtype=F).reshape(3, 2), np.full((3, 2), 4.0, F)
    w2, mi2, iv2, of = T.split(w, mi, iv, 5, 0.01, 0)
    assert of == [0, 1] and w2.tolist() == [0.25, 0.15000000596046448, 0.20000000298023224, 0.25, 0.15000000596046448]
    assert np.allclose(mi2[0] + mi2[3], 2 * mi[0], atol=1e-6) and not np.array_equal(mi2[0], mi2[3])
    assert np.allclose(np.abs(mi2[3] - mi[0]), 0.01 * 2.0 * np.abs([T.gauss(0, T.ENTRY_SPLIT + 3 * 2 + d) for d in range(2)]), atol=1e-6)
    assert not np.array_equal(T.split(w, mi, iv, 5, 0.01, 1)[1], mi2) and np.array_equal(iv2[3], iv[0])


def test_the_file_round_trips_in_both_modes():
    rng = np.random.default_rng(4)
    occ, mean, var = rng.uniform(1, 9, 3), rng.normal(size=(3, 2)), rng.uniform(1, 2, (3, 2))
    for flags in (7, 5, 4):
        for binary in (True, False):
            got = T.read_accs(T.accs_bytes(occ, mean, var, flags, binary))
            assert got["flags"] == flags and np.array_equal(got["occ"], occ.astype(F)) and np.array_equal(got["mean"], mean.astype(F))
            assert np.array_equal(got["var"], var.astype(F) if flags & 2 else np.zeros((3, 2), F))
