"""Self-checks of the numpy restatement of per-speaker CMVN (tests/cmvn_ref.py): no library, no GPU."""
import numpy as np
import pytest

import cmvn_ref as R


def test_statistics_of_a_tiny_matrix():
    x = np.array([[1, 2], [3, 4], [5, 9]], dtype=np.float32)
    st = R.stats(x)
    assert st.tolist() == [[9.0, 15.0, 3.0], [35.0, 101.0, 0.0]]


def test_mean_normalisation_known_answer():
    st = np.array([[9.0, 15.0, 3.0], [35.0, 101.0, 0.0]])
    n = R.cmvn_norm(st)
    assert n.dtype == np.float32 and n.tolist() == [[-3.0, -5.0], [1.0, 1.0]]
    y = R.apply(np.array([[1, 2], [3, 4], [5, 9]], np.float32), n)
    assert y.tolist() == [[-2.0, -3.0], [0.0, -1.0], [2.0, 4.0]]


def test_variance_normalisation_known_answer():
    # column 0: mean 3, variance 35 / 3 - 9 = 8 / 3
    st = np.array([[9.0, 0.0, 3.0], [35.0, 12.0, 0.0]])
    n = R.cmvn_norm(st, norm_vars=True)
    var = 35.0 / 3.0 - 9.0
    assert n[1, 0] == np.float32(1.0 / np.sqrt(var)) and n[0, 0] == np.float32(-(3.0 * (1.0 / np.sqrt(var))))
    assert n[1, 1] == np.float32(0.5) and n[0, 1] == 0.0   # mean 0, variance 4
    y = R.apply(np.array([[1, 2], [3, -2], [5, 2]], np.float32), n)
    np.testing.assert_allclose(y.mean(axis=0)[0], 0.0, atol=1e-6)
    np.testing.assert_allclose((y.astype(np.float64) ** 2).mean(axis=0), [1.0, 1.0], rtol=1e-6)


def test_the_product_and_the_sum_are_rounded_separately():
    x = np.array([[np.float32(1.0) + np.float32(2.0 ** -23)]], np.float32)
    n = np.array([[-1.0], [np.float32(1.0) + np.float32(2.0 ** -23)]], np.float32)
    # (1 + e)^2 = 1 + 2 e + e^2 rounds to 1 + 2 e in float32; a fused multiply-add would keep the e^2
    assert R.apply(x, n)[0, 0] == np.float32(2.0 ** -22)


def test_a_constant_column_is_floored():
    st = R.stats(np.full((7, 1), 2.5, np.float32))
    n, floored = R.cmvn_norm(st, norm_vars=True, return_floored=True)
    assert floored == 1
    assert n[1, 0] == np.float32(1.0 / np.sqrt(1.0e-20)) and n[0, 0] == np.float32(-(2.5 * (1.0 / np.sqrt(1.0e-20))))
    assert R.cmvn_norm(st, norm_vars=False, return_floored=True)[1] == 0


def test_skip_dims_leave_the_column_alone():
    rng = np.random.default_rng(0)
    x = rng.normal(3, 2, size=(50, 4)).astype(np.float32)
    for nv in (False, True):
        n = R.cmvn_norm(R.stats(x), norm_vars=nv, skip_dims=(1, 3))
        assert n[1, 1] == 1.0 and n[0, 1] == 0.0 and n[1, 3] == 1.0 and n[0, 3] == 0.0
        y = R.apply(x, n)
        assert np.array_equal(y[:, [1, 3]], x[:, [1, 3]])
        assert not np.array_equal(y[:, 0], x[:, 0])


@pytest.mark.parametrize("norm_vars", [False, True])
def test_reverse_inverts_forward(norm_vars):
    rng = np.random.default_rng(1)
    x = rng.normal(-4, 3, size=(200, 5)).astype(np.float32)
    st = R.stats(x)
    y = R.apply(x, R.cmvn_norm(st, norm_vars=norm_vars))
    back = R.apply(y, R.cmvn_norm(st, norm_vars=norm_vars, reverse=True))
    # two float32 affine maps: a few ulps of the largest magnitude involved (|x| and the mean are below 16)
    assert np.abs(back.astype(np.float64) - x).max() <= 8 * 16 * 2.0 ** -24


def test_no_normalisation_is_the_identity():
    x = np.arange(12, dtype=np.float32).reshape(4, 3)
    n = R.cmvn_norm(R.stats(x), norm_means=False)
    assert n.tolist() == [[0.0] * 3, [1.0] * 3] and np.array_equal(R.apply(x, n), x)


def test_refusals():
    st = np.array([[9.0, 15.0, 3.0], [35.0, 101.0, 0.0]])
    with pytest.raises(R.CmvnError, match="cannot normalize the variance but not the mean"):
        R.cmvn_norm(st, norm_means=False, norm_vars=True)
    with pytest.raises(R.CmvnError, match="Insufficient stats"):
        R.cmvn_norm(np.array([[0.0, 0.0, 0.5], [0.0, 0.0, 0.0]]))
    with pytest.raises(R.CmvnError):
        R.cmvn_norm(st, skip_dims=(2,))
    with pytest.raises(R.CmvnError):
        R.cmvn_norm(np.zeros((3, 3)))


def test_bound_covers_a_plain_recursive_sum():
    rng = np.random.default_rng(2)
    x = rng.normal(50, 1, size=(700, 3)).astype(np.float32)
    exact, bound = R.stats(x), R.stats_bound(x)
    got = np.zeros_like(exact)
    for r in range(x.shape[0]):
        got[0, :3] += x[r].astype(np.float64)
        got[1, :3] += x[r].astype(np.float64) ** 2
    got[0, 3] = 700
    assert np.all(np.abs(got - exact) <= bound)
