"""The two statements of sliding-window CMN the GPU tests rely on pin each other, without a GPU: the closed form of
tests/cmn_sliding_ref.py, the branch sequence of oracle/frontend.py, and windows computed by hand that are neither."""
import numpy as np
import pytest

import helpers as H  # noqa: F401  (puts the repository root on sys.path)
import cmn_sliding_ref as R
from oracle import frontend as fe

# the option space of tests/test_gpu_cmn_sliding.py's sweep; the lengths are those of both prefix layouts (32 and 16 segments)
WINDOWS = (1, 2, 3, 7, 8, 299, 300, 301, 600, 10000)
MIN_WINDOWS = (0, 1, 50, 100, 101, 700)
LENGTHS = (1, 2, 15, 16, 17, 31, 32, 33, 65, 99, 100, 101, 299, 300, 301, 650)


def option_points():
    for W in WINDOWS:
        yield W, True, 100
        for M in MIN_WINDOWS:
            yield W, False, M


@pytest.fixture(scope="module")
def utts():
    return {T: R.dyadic_features(4000 + T, T, 3) for T in LENGTHS}


def test_closed_form_equals_the_branch_sequence_byte_for_byte(utts):
    """On dyadic inputs both are exact up to the same three roundings (division, subtraction, cast), whatever the order of their
    sums: any difference is a difference in the WINDOW."""
    for x in utts.values():
        R.assert_exactness_precondition(x)
    for W, center, M in option_points():
        for T, x in utts.items():
            a = R.sliding_cmn(x, W, center, M)
            b = fe.sliding_cmn(x, W, center, M)
            assert a.dtype == b.dtype == np.float32 and a.tobytes() == b.tobytes(), (W, M, center, T)
    # centred: the minimum window is not used
    for T, x in utts.items():
        assert R.sliding_cmn(x, 300, True, 1).tobytes() == R.sliding_cmn(x, 300, True, 700).tobytes()
        assert fe.sliding_cmn(x, 300, True, 1).tobytes() == fe.sliding_cmn(x, 300, True, 700).tobytes()


def test_window_properties_over_the_sweep():
    for W, center, M in option_points():
        for T in LENGTHS:
            s, e = R.bounds(T, W, center, M)
            t = np.arange(T)
            assert s.shape == e.shape == (T,)
            assert (0 <= s).all() and (s < e).all() and (e <= T).all(), (W, M, center, T)
            if center:
                assert (e - s == min(W, T)).all(), (W, T)
                if T >= W:
                    assert (s <= t).all() and (t < e).all(), (W, T)
                # away from the edges the window starts W // 2 frames back
                mid = (t - W // 2 >= 0) & (t - W // 2 + W <= T)
                assert (s[mid] == t[mid] - W // 2).all()
            else:
                # derived in cmn_sliding_ref.py's docstring
                want = np.minimum(T, np.maximum(np.minimum(t, W) + 1, M - np.maximum(t - W, 0)))
                assert (e - s == want).all(), (W, M, T)
                assert (s <= t).all() and (t < e).all()          # the frame itself is always inside: the window ends at t + 1 or later
                late = (t >= W) & (t + 1 >= M)
                assert (e[late] - s[late] == W + 1).all()       # W + 1 frames once t >= W


LITERAL = [
    # (T, W, M, centred, windows worked out by hand)
    (5, 3, 100, True, [(0, 3), (0, 3), (1, 4), (2, 5), (2, 5)]),
    (6, 4, 100, True, [(0, 4), (0, 4), (0, 4), (1, 5), (2, 6), (2, 6)]),              # even window: W / 2 back
    (7, 5, 100, True, [(0, 5), (0, 5), (0, 5), (1, 6), (2, 7), (2, 7), (2, 7)]),      # odd window: 5 / 2 = 2 back, not 3
    (3, 8, 100, True, [(0, 3)] * 3),                                                  # window above T: the whole utterance
    (4, 2, 3, False, [(0, 3), (0, 3), (0, 3), (1, 4)]),
    (6, 2, 0, False, [(0, 1), (0, 2), (0, 3), (1, 4), (2, 5), (3, 6)]),               # no minimum: W + 1 frames once t >= W
    (5, 1, 4, False, [(0, 4), (0, 4), (1, 4), (2, 4), (3, 5)]),                       # the minimum extends the END only
    (4, 1, 6, False, [(0, 4)] * 4),                                                   # minimum above T: clipped, start pulled to 0
    (1, 300, 100, False, [(0, 1)]), (1, 300, 100, True, [(0, 1)]),
]


@pytest.mark.parametrize("T,W,M,center,want", LITERAL)
def test_hand_computed_windows_anchor_both_statements(T, W, M, center, want):
    s, e = R.bounds(T, W, center, M)
    assert list(zip(s.tolist(), e.tolist())) == want
    # and through the arithmetic of both: column 0 counts the frames from 1, so the mean over [s, e) is (s + 1 + e) / 2
    x = np.stack([np.arange(1, T + 1), 64.0 - 3 * np.arange(T)], axis=1).astype(np.float32)
    mean0 = np.array([(a + 1 + b) / 2.0 for a, b in want])
    mean1 = np.array([64.0 - 3 * (a + b - 1) / 2.0 for a, b in want])
    out = (x.astype(np.float64) - np.stack([mean0, mean1], axis=1)).astype(np.float32)
    assert np.array_equal(R.sliding_cmn(x, W, center, M), out)
    assert np.array_equal(fe.sliding_cmn(x, W, center, M), out)


def test_literal_output():
    """T = 5, W = 3, centred, x = 1..5: the means are 2 2 3 4 4."""
    x = np.arange(1, 6, dtype=np.float32)[:, None]
    assert R.sliding_cmn(x, 3, True).ravel().tolist() == [-1.0, 0.0, 0.0, 0.0, 1.0]
    assert R.sliding_cmn(x, 0, True).tobytes() == x.tobytes()                         # no window: the input
    assert R.sliding_cmn(np.zeros((0, 4), np.float32), 3, True).shape == (0, 4)


def test_the_exact_sums_do_not_depend_on_the_path():
    """The int64 path and the unlimited one (Python fractions) give the same bytes where both apply, and the unlimited one is
    what runs when a column does not fit 2^53 grid units: a value of 2^60 next to one of 2^-20."""
    rng = np.random.default_rng(5)
    x = (rng.standard_normal((40, 3)) + 1000.0).astype(np.float32)
    for W, center, M in ((7, True, 100), (5, False, 3), (600, False, 100)):
        s, e = R.bounds(40, W, center, M)
        fast = R.sliding_cmn(x, W, center, M, rounded=False)
        slow = x.astype(np.float64) - R._means_by_fractions(x, s, e)
        assert fast.tobytes() == slow.tobytes()
    # a column of 2^58 grid units: int64 sums that no double holds, divided as integers
    z = rng.standard_normal((40, 3)).astype(np.float32)
    z[5, 1], z[17, 1] = 2.0 ** 20, 1.5 * 2.0 ** -15
    k, q = R.grid(z)
    assert k is not None and 2.0 ** 52 < np.abs(k).astype(np.float64).sum(axis=0).max() < 2.0 ** 61
    assert np.array_equal(np.ldexp(k.astype(np.float64), q)[:, 0], z[:, 0].astype(np.float64))
    s, e = R.bounds(40, 7, True)
    assert R.sliding_cmn(z, 7, True, rounded=False).tobytes() == (z.astype(np.float64) - R._means_by_fractions(z, s, e)).tobytes()
    y = np.array([[2.0 ** 60], [2.0 ** -20], [-(2.0 ** 60)], [3.0]], np.float32)
    k, _ = R.grid(y)
    assert k is None
    # window [0, 4) for every frame: the sum is 3 + 2^-20 exactly (a double prefix sum would have lost both small terms)
    got = R.sliding_cmn(y, 8, True, rounded=False)
    assert got[3, 0] == 3.0 - (3.0 + 2.0 ** -20) / 4.0


def test_the_engine_case_tells_the_options_apart():
    """The precondition of tests/test_gpu_cmn_sliding.py's engine test, with the oracle alone: on its utterances the x-vectors of
    the wrong options (minimum window 100 in place of 50 or 0, centred in place of not) are at least 10 parity bars from the right
    ones.  (The assertions are in engine_case.)"""
    import test_gpu_cmn_sliding as G
    utts, vads, right = G.engine_case()
    assert sorted(right) == [0, 50] and all(150 <= x.shape[0] <= 400 for _, x in utts)


def test_select_keeps_the_rows_with_a_nonzero_decision():
    f = np.arange(12, dtype=np.float32).reshape(6, 2)
    assert np.array_equal(R.select(f, [1, 0, 0, 2, -1, 0]), f[[0, 3, 4]])
    assert R.select(f, np.zeros(6)).shape == (0, 2)
    assert np.array_equal(R.select(f, np.ones(6)), f)
