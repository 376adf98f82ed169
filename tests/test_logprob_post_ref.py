"""The numpy restatement of logprob-to-post (tests/logprob_post_ref.py) against rows worked by hand, and the wiring of its uniform."""
import numpy as np

import dither_ref
import logprob_post_ref as LP

F = np.float32
NINF = F(-np.inf)


def lg(*p):
    return np.log(np.array(p, np.float64)).astype(F)


def test_hand_worked_rows_without_random_pruning():
    # min_post = 0.01: 0.5 and 0.03 stay with their own value, 0.004 and 0.0007 go, -inf goes; the second row comes out empty
    x = np.stack([np.concatenate([lg(0.004, 0.5, 0.0007), [NINF], lg(0.03)]), np.concatenate([lg(0.004, 0.0007, 0.0007), [NINF, NINF]])])
    post, nans = LP.logprob_to_post(x, "utt", 0.01, False)
    assert nans == 0 and len(post) == 2
    assert post[0][0].tolist() == [1, 4] and post[0][0].dtype == np.int32 and post[0][1].dtype == F
    assert post[0][1].tolist() == [np.exp(np.float64(x[0, 1])).astype(F), np.exp(np.float64(x[0, 4])).astype(F)]
    assert abs(float(post[0][1][0]) - 0.5) < 1e-7 and abs(float(post[0][1][1]) - 0.03) < 1e-8
    assert post[1][0].tolist() == [] and post[1][1].tolist() == []


def test_min_post_zero_keeps_everything_and_minus_infinity_gives_zero():
    x = np.stack([np.concatenate([lg(0.2), [NINF], lg(0.0007)])])
    for prune in (True, False):
        for mp in (0.0, -1.0):
            post, nans = LP.logprob_to_post(x, "utt", mp, prune)
            assert nans == 0 and post[0][0].tolist() == [0, 1, 2]
            assert post[0][1][1] == 0.0 and abs(float(post[0][1][0]) - 0.2) < 1e-7 and abs(float(post[0][1][2]) - 0.0007) < 1e-9


def test_nan_is_dropped_and_counted_whatever_min_post_is():
    x = np.array([[np.nan, np.log(0.5), np.nan]], F)
    for mp in (0.0, 0.01):
        post, nans = LP.logprob_to_post(x, "utt", mp, True)
        assert nans == 2 and post[0][0].tolist() == [1]


def test_random_pruning_follows_the_dither_generators_first_uniform():
    """p / min_post = 0.4 or 0.07 against u of (key, row, column): kept with min_post's bits exactly where u <= the ratio; columns
    stay ascending; a second key draws other numbers; the row index counts within the utterance"""
    rows, cols = 6, 40
    x = np.tile(lg(0.004, 0.0007, 0.5, 0.2), (rows, cols // 4))
    u = dither_ref.uniforms("spk-a", rows, cols)[0]
    post, _ = LP.logprob_to_post(x, "spk-a", 0.01, True)
    ratio = (np.exp(x.astype(np.float64)).astype(F) / F(0.01)).astype(F)
    for r in range(rows):
        want = [j for j in range(cols) if j % 4 >= 2 or ratio[r, j] >= u[r, j]]
        assert post[r][0].tolist() == want and want == sorted(want)
        for j, w in zip(*post[r]):
            assert w.view(np.uint32) == (F(0.01).view(np.uint32) if j % 4 < 2 else np.exp(np.float64(x[r, j])).astype(F).view(np.uint32))
    kept_small = sum(int((i % 4 < 2).sum()) for i, _ in post)
    assert 0 < kept_small < rows * cols // 2
    other, _ = LP.logprob_to_post(x, "spk-b", 0.01, True)
    assert any(a[0].tolist() != b[0].tolist() for a, b in zip(post, other))
    # rows 2 .. 6 read as an utterance of their own are rows 0 .. 4 of that utterance: other draws; read with row0 = 2 they are the same
    again, _ = LP.logprob_to_post(x[2:], "spk-a", 0.01, True, row0=2)
    assert all(a[0].tolist() == b[0].tolist() for a, b in zip(post[2:], again))
    alone, _ = LP.logprob_to_post(x[2:], "spk-a", 0.01, True)
    assert any(a[0].tolist() != b[0].tolist() for a, b in zip(post[2:], alone))


def test_half_of_the_entries_at_half_of_min_post_are_kept():
    """2^16 entries with p = min_post / 2: each is kept with probability 1/2 (u is uniform on the multiples of 2^-24 in (0, 1]), so
    the kept share lies within five binomial standard deviations, 5 * sqrt(n / 4) = 640 entries, of n / 2.  The number is
    deterministic; it shows that u is wired to all three of key, row and column."""
    rows, cols = 256, 256
    n = rows * cols
    x = np.full((rows, cols), np.log(0.005), F)
    post, _ = LP.logprob_to_post(x, "binomial", 0.01, True)
    kept = sum(len(i) for i, _ in post)
    print("kept %d of %d" % (kept, n))
    assert abs(kept - n / 2) <= 5 * np.sqrt(n * 0.25)
    per_row = np.array([len(i) for i, _ in post])
    per_col = np.bincount(np.concatenate([i for i, _ in post]), minlength=cols)
    # no row and no column is all or nothing: 256 draws each, 128 expected, 5 sigma = 40
    assert np.all(np.abs(per_row - cols / 2) <= 40) and np.all(np.abs(per_col - rows / 2) <= 40)
    assert all(np.all(w.view(np.uint32) == F(0.01).view(np.uint32)) for _, w in post)
