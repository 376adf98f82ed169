"""The numpy restatement of i-vector extraction (tests/ivector_ref.py) against closed forms; no device, no library."""
import numpy as np
import pytest

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
