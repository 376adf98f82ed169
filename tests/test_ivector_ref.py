"""The numpy restatement of i-vector extraction (tests/ivector_ref.py) against closed forms, and the inputs of the GPU tests
(tests/ivector_cases.py) against the preconditions those tests assert; no device, no library."""
import numpy as np
import pytest

import ivector_cases as C
import ivector_ref as R


def test_packed_index_is_row_major_over_the_lower_triangle():
    S = 7
    sym = np.arange(S * S, dtype=np.float64).reshape(S, S)
    sym = np.tril(sym) + np.tril(sym, -1).T
    p = R.pack(sym)
    assert len(p) == S * (S + 1) // 2
    for r in range(S):
        for c in range(r + 1):
            assert p[R.packed_index(r, c)] == sym[r, c]
    assert R.packed_index(0, 0) == 0 and R.packed_index(1, 0) == 1 and R.packed_index(1, 1) == 2 and R.packed_index(2, 0) == 3
    assert np.array_equal(R.unpack(p, S), sym)


@pytest.mark.parametrize("D", [1, 3, 8])
def test_one_gaussian_with_identity_model_has_a_closed_form(D):
    """Sigma^-1 = I and M = I: l = X + p e_0 and Q = (gamma + 1) I, so the i-vector is (X + p e_0) / (gamma + 1) - p e_0."""
    rng = np.random.default_rng(D)
    p = 2.5
    M = np.eye(D)[None]
    sig = R.pack(np.eye(D))[None]
    x = rng.normal(size=(11, D)).astype(np.float32)
    post = [(np.array([0]), np.array([w], np.float32)) for w in rng.uniform(0.1, 1.0, 11)]
    out = R.extract(x, post, M, sig, p)
    gamma = sum(float(w[0]) for _, w in post)
    X = sum(float(w[0]) * x[t].astype(np.float64) for t, (_, w) in enumerate(post))
    e0 = np.zeros(D)
    e0[0] = p
    want = (X + e0) / (gamma + 1.0) - e0
    assert np.allclose(out["x"] - e0, want, rtol=1e-13, atol=1e-13)
    assert np.array_equal(out["ivector"], (out["x"] - e0).astype(np.float32))
    assert abs(out["gamma"][0] - gamma) < 1e-12 and np.allclose(out["quadratic"], (gamma + 1.0) * np.eye(D))


@pytest.mark.parametrize("seed", range(5))
def test_the_objective_change_is_never_negative(seed):
    """x maximises F, so F(x) - F(anything) >= 0; it is (x - p e_0)' Q (x - p e_0) / 2."""
    G, D, S = 6, 5, 9
    m = R.random_model(seed, G, D, S)
    x, post = R.integer_utterance(seed, 40, G, D)
    out = R.extract(x, post, m["M"], m["sigma_inv"], m["prior_offset"])
    assert out["auxf_change"] >= 0.0
    d = out["x"].copy()
    d[0] -= m["prior_offset"]
    assert abs(out["auxf_change"] - 0.5 * d @ out["quadratic"] @ d) <= 1e-9 * (1.0 + abs(out["auxf_change"]))


def test_acoustic_weight_and_max_count_rules():
    post = [(np.array([0, 1]), np.array([0.5, 0.25], np.float32)), (np.array([2]), np.array([1.0], np.float32)), (np.array([], int), np.array([], np.float32))]
    # the defaults change nothing
    same, scale, clipped = R.scale_posteriors(post)
    assert scale == np.float32(1.0) and not clipped
    assert all(np.array_equal(a[1], b[1]) for a, b in zip(same, post))
    # acoustic weight alone: every posterior times float32(0.3), rounded in float32
    got, scale, clipped = R.scale_posteriors(post, acoustic_weight=0.3)
    assert scale == np.float32(0.3) and not clipped
    assert got[0][1].dtype == np.float32 and np.array_equal(got[0][1], np.array([0.5, 0.25], np.float32) * np.float32(0.3))
    # tot = 0.5 * 1.75 = 0.875 > 0.7: the scale is 0.5 * 0.7 / 0.875 = 0.4 and the scaled total is max_count
    got, scale, clipped = R.scale_posteriors(post, acoustic_weight=0.5, max_count=0.7)
    assert clipped and scale == np.float32(0.5 * 0.7 / 0.875)
    assert abs(sum(float(w.sum()) for _, w in got) - 0.7) < 1e-6
    # a max_count that does not bite leaves the acoustic weight
    _, scale, clipped = R.scale_posteriors(post, acoustic_weight=0.5, max_count=0.875)
    assert not clipped and scale == np.float32(0.5)


def test_model_bytes_have_the_documented_layout():
    m = R.integer_model(1, 2, 2, 3)
    data = R.ie_bytes(binary=True, **m)
    assert data.startswith(b"\0B<IvectorExtractor> <w> DM \x04\x00\x00\x00\x00\x04\x00\x00\x00\x00<w_vec> DV \x04\x02\x00\x00\x00")
    assert data.endswith(b"<IvectorOffset> \x08" + np.float64(m["prior_offset"]).tobytes() + b"</IvectorExtractor> ")
    assert data.count(b"DM ") == 3 and data.count(b"DP ") == 2
    text = R.ie_bytes(binary=False, **m)
    assert text.startswith(b"<IvectorExtractor> <w>  [ ]\n<w_vec>  [ 0.5 0.5 ]\n<M> 2  [\n")


# ------------------------------------------------------------------------------------------------------------------- test models
def test_the_default_scale_of_a_random_model_is_the_models_of_before():
    a, b = R.random_model(3, 4, 5, 6), R.random_model(3, 4, 5, 6, m_scale=0.3)
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    assert np.array_equal(a["M"][0, 0, :3], np.random.default_rng(3).normal(0.0, 0.3, (4, 5, 6))[0, 0, :3])
    half = R.random_model(3, 4, 5, 6, m_scale=0.15)
    assert np.array_equal(2.0 * half["M"], a["M"]) and np.array_equal(half["sigma_inv"], a["sigma_inv"])
    assert all(C.m_scale_for(S) == 0.3 for S in range(1, 2 * C.NB + 4)) and C.m_scale_for(C.MAX_S) < 0.3 * 0.25


def test_zero_leading_columns_make_the_leading_block_of_q_the_identity():
    G, D, S, s0 = 3, 4, 9, 5
    m = R.integer_model(2, G, D, S)
    z = R.zero_leading_columns(m, s0)
    assert m["M"][:, :, :s0].any() and not z["M"][:, :, :s0].any() and np.array_equal(z["M"][:, :, s0:], m["M"][:, :, s0:])
    x, post = R.integer_utterance(3, 20, G, D)
    out = R.extract(x, post, z["M"], z["sigma_inv"], z["prior_offset"])
    Q = out["quadratic"]
    assert np.array_equal(Q[:s0, :s0], np.eye(s0)) and not Q[:s0, s0:].any() and not Q[s0:, :s0].any()
    assert out["linear"][0] == z["prior_offset"] and not out["linear"][1:s0].any()


# ------------------------------------------------------------------------------------------------------------------- the GPU tests' inputs
# What follows runs no device code: it is the CPU half of tests/test_gpu_ivector.py and tests/test_gpu_ivector_train.py.  Every
# shape those files add beyond S = 67 is built here exactly as they build it (tests/ivector_cases.py), and the preconditions
# they assert on their inputs are asserted on the restatement alone, so that a run on the device cannot fail on one.
ROOM = 1.5   # what the scaled random models leave between eps_of(Q) and the precondition's 1e-6


def _new(cases, before):
    return [c for c in cases if c not in before]


def test_the_shape_lists_sit_on_the_kernels_edges():
    """the values the lists have with the constants of today, so that a reader sees them and a moved constant shows here"""
    assert (C.THREADS, C.NB, C.SOLVE_RT, C.MAX_S, C.MAX_B, C.MAX_D, C.POST_THREADS, C.TRAIN_THREADS, C.RT) == (256, 32, 64, 1024, 64, 96, 1024, 256, 16)
    assert C.SOLVE_EDGES == [95, 96, 256, 257, 258, 287, 288, 400, 513, 514, 600, 769, 770, 1023, 1024]
    assert [s[2] for s in C.POSTERIOR_CASES[3:]] == [63, 64, 65, 66, 128, 129, 400, 1023, 1024]
    assert [b for *_, b in C.BATCH_CASES] == [48, 49, 64, 65, 130] and [d for _, d, *_ in C.DIM_CASES] == [64, 65, 95, 96]
    assert C.STATS_CASES == [(7, 9, 11), (5, 7, 20), (5, 7, 21), (5, 7, 70)] and C.SPLIT_SHAPE == (5, 7, 129) and C.SPLIT_UTTS == 66
    assert (C.LATE_S0, C.LATE_S) == (65, 101) and [c[2] for c in C.LARGE_S_TERM_CASES] == [257, 1024]
    assert [C.small_sums_elements(5, S) for S in (20, 21, 70)] == [236, 258, 2561]


@pytest.mark.parametrize("G,D,S", _new(C.SOLVE_CASES, C.SOLVE_CASES[:4]))
def test_the_solve_cases_meet_the_gpu_tests_precondition(G, D, S):
    m = C.solve_model(G, D, S)
    sim_U = R.derived(m["M"], m["sigma_inv"])
    for x, post in C.solve_utterances(G, D, S, C.solve_utts_count(S)):
        r = R.extract(x, post, m["M"], m["sigma_inv"], m["prior_offset"], sim_U=sim_U)
        eps = C.eps_of(r["quadratic"])
        print("S = %d: eps %.3g, |x| %.3g, median |x_i| %.3g" % (S, eps, np.linalg.norm(r["x"]), np.median(np.abs(r["x"]))))
        assert eps * ROOM < 1e-6
        assert np.linalg.norm(r["x"]) > 0.5   # the solution stays O(1): the bounds of check_solve still bite


@pytest.mark.parametrize("G,D,S,T,B", C.BATCH_CASES + C.DIM_CASES)
def test_the_integer_cases_meet_the_gpu_tests_preconditions(G, D, S, T, B):
    m = R.integer_model(C.integer_seed(G, D, S), G, D, S)
    sim, U = R.derived(m["M"], m["sigma_inv"])
    worst = 0.0
    for x, post in C.case_utterances(G, D, S, T, B):
        r = R.extract(x, post, m["M"], m["sigma_inv"], m["prior_offset"], sim_U=(sim, U))
        assert C.exact_preconditions(m, sim, U, x, post, r["gamma"])
        worst = max(worst, C.eps_of(r["quadratic"]))
    print("worst eps %.3g" % worst)
    assert worst < 1e-6


@pytest.mark.parametrize("G,D,S,T,B", C.LARGE_S_TERM_CASES)
def test_the_large_integer_cases_are_exact_in_float64(G, D, S, T, B):
    assert T <= 40
    m = R.integer_model(C.integer_seed(G, D, S), G, D, S)
    sim, U = R.derived(m["M"], m["sigma_inv"])
    assert U.shape == (G, S * (S + 1) // 2)
    for x, post in C.case_utterances(G, D, S, T, B):
        gamma = R.stats(x, post, G)[0]
        assert C.exact_preconditions(m, sim, U, x, post, gamma)


def test_the_long_utterances_close_a_group_by_frames_and_are_exact_in_float64():
    G, D, S = C.FRAMES_SHAPE
    L = C.FRAMES_LENGTHS
    assert len(L) <= C.MAX_B and L[0] + L[1] <= C.BATCH_FRAMES < L[0] + L[1] + L[2] and L[3] > C.BATCH_FRAMES
    m = R.integer_model(C.integer_seed(G, D, S), G, D, S)
    sim, U = R.derived(m["M"], m["sigma_inv"])
    utts = C.frames_utterances()
    assert [len(x) for x, _ in utts] == L and sum(len(p) for _, p in utts) < 2 ** 31
    for x, post in utts:
        gamma = R.stats(x, post, G)[0]
        assert gamma.all() and C.exact_preconditions(m, sim, U, x, post, gamma)


def test_the_late_bad_pivot_is_late_and_its_neighbours_meet_the_precondition():
    G, D = 2, 3
    for S, s0 in ((C.NB + 5, 0), (C.LATE_S, C.LATE_S0)):
        m = C.not_pd_model(G, D, S, s0)
        sim_U = R.derived(m["M"], m["sigma_inv"])
        good0, bad, good1 = C.not_pd_utterances(D)
        Q = R.extract(*bad, m["M"], m["sigma_inv"], m["prior_offset"], sim_U=sim_U)["quadratic"]
        assert np.array_equal(Q[:s0, :s0], np.eye(s0)) and np.linalg.eigvalsh(Q).min() < 0
        first = C.first_bad_pivot(Q)
        print("S = %d, s0 = %d: the first bad pivot is %d, panel %d" % (S, s0, first, first // C.NB))
        assert s0 <= first < S
        if s0:
            assert first // C.NB >= 2
        for utt in (good0, good1):
            assert C.eps_of(R.extract(*utt, m["M"], m["sigma_inv"], m["prior_offset"], sim_U=sim_U)["quadratic"]) < 1e-6


@pytest.mark.parametrize("G,D,S", _new(C.POSTERIOR_CASES, C.POSTERIOR_CASES[:3]))
def test_the_posterior_cases_meet_the_gpu_tests_precondition(G, D, S):
    m = C.posterior_model(G, D, S)
    sim_U = R.derived(m["M"], m["sigma_inv"])
    utts = C.random_utts(S, C.posterior_utts_count(S), G, D)
    assert len(utts) == (4 if S <= 400 else 2)
    for x, post in utts:
        eps = C.eps_of(R.extract(x, post, m["M"], m["sigma_inv"], m["prior_offset"], sim_U=sim_U)["quadratic"])
        print("S = %d: eps %.3g" % (S, eps))
        assert eps * (ROOM if S > 2 * C.NB + 3 else 1.0) < 1e-6
