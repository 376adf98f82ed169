"""GPU tests of the three kernels of nnet-am-compute (csrc/nnet2_kernels.hip), one launch each through xv_nnet2_kernel_*: the spliced
affine bit for bit on small integers (every product and partial sum exact in fp32), at the edges of the row tile, the K tail, the
N tail and the halo; the row kernel and the head against float64 under the rule of nnet2_ref.tolerance.

Measured on an MI355X (profiles/nnet2_parity.md): the row kernel's largest error is 0.27 of its bound, the head's 0.29."""
import numpy as np
import pytest

import helpers as H
import nnet2_ref as R

pytestmark = pytest.mark.gpu

ROWS = (1, 16, 17, 127, 128, 129, 257)
KS = (8, 32, 40, 350)
CONTEXTS = ([0], [-2, -1, 0, 1, 2], [-1, 2], [-7, 2], [-3, 3])
NS = (1, 10, 127, 128, 130, 350)


def _affine_cases():
    out = []
    for i in range(30):
        rows, k, ctx, n = ROWS[i % 7], KS[i % 4], CONTEXTS[i % 5], NS[i % 6]
        if k * len(ctx) > 700:   # every partial sum stays far below 2^24 (700 * 64)
            ctx = CONTEXTS[2]
        out.append((rows, k, ctx, n))
    return out


AFFINE_CASES = _affine_cases()


def test_the_cases_hold_every_edge():
    assert {c[0] for c in AFFINE_CASES} == set(ROWS) and {c[1] for c in AFFINE_CASES} == set(KS) and {c[3] for c in AFFINE_CASES} == set(NS)
    assert {tuple(c[2]) for c in AFFINE_CASES} == {tuple(c) for c in CONTEXTS} and all(c[1] * len(c[2]) <= 700 for c in AFFINE_CASES)


def _exact(x, ctx, w, b):
    """integer arithmetic: rows outside x are zero"""
    rows, k = x.shape
    halo = max(abs(c) for c in ctx)
    xp = np.zeros((rows + 2 * halo, k), np.int64)
    xp[halo:halo + rows] = x
    out = np.tile(b.astype(np.int64), (rows, 1))
    for i, c in enumerate(ctx):
        out += xp[halo + c:halo + c + rows] @ w[:, i * k:(i + 1) * k].astype(np.int64).T
    return out


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("rows,k,ctx,n", AFFINE_CASES, ids=["r%d-k%d-c%s-n%d" % (r, k, "_".join(map(str, c)), n) for r, k, c, n in AFFINE_CASES])
def test_the_spliced_affine_is_exact_on_small_integers(rows, k, ctx, n):
    P = H.pkg()
    rng = np.random.default_rng(rows * 1000 + k + n)
    x = rng.integers(-8, 9, size=(rows, k))
    w = rng.integers(-8, 9, size=(n, k * len(ctx)))
    b = rng.integers(-8, 9, size=n)
    w[0, 0], x[0, 0], x[-1, -1] = 8, -8, 8   # the ends of the range are there
    got = P.nnet2.kernel_affine(x, ctx, w, b)
    want = _exact(x, ctx, w, b)
    assert np.abs(want).max() < 2 ** 24
    assert np.array_equal(_bits(got), _bits(want))


def test_two_utterances_whose_paddings_abut():
    """[13 copies | utterance a | 9 copies][13 copies | utterance b | 9 copies] as the stage packs them: exact everywhere, and the
    rows of a are the rows a gives when it is packed alone."""
    P = H.pkg()
    rng = np.random.default_rng(2)
    ctx, k, n = [-7, 2], 40, 130
    a, b = rng.integers(-8, 9, size=(20, k)), rng.integers(-8, 9, size=(70, k))
    w, bias = rng.integers(-8, 9, size=(n, 2 * k)), rng.integers(-8, 9, size=n)
    pa, pb = R.pad(a, 13, 9), R.pad(b, 13, 9)
    both = np.concatenate([pa, pb])
    got = P.nnet2.kernel_affine(both, ctx, w, bias)
    assert np.array_equal(_bits(got), _bits(_exact(both, ctx, w, bias)))
    alone = P.nnet2.kernel_affine(pa, ctx, w, bias)
    assert np.array_equal(_bits(got[7:len(pa) - 2]), _bits(alone[7:len(pa) - 2]))   # the rows whose context lies inside a's own rows


# ------------------------------------------------------------------------------------------------------------------ the row kernel
ROW_CASES = [("pnorm", 60, 6), ("pnorm", 3500, 350), ("pnorm", 64, 64), ("pnorm", 455, 65), ("relu", 6, 6), ("relu", 65, 65), ("relu", 350, 350),
             ("none", 64, 64), ("none", 350, 350)]


def _row_ref(x, nonlin, out_dim, norm, dtype):
    x = x.astype(dtype)
    y = R.pnorm(x, out_dim) if nonlin == "pnorm" else np.maximum(x, dtype(0)) if nonlin == "relu" else x
    return R.normalize(y) if norm else y


@pytest.mark.parametrize("normalize", [False, True])
@pytest.mark.parametrize("nonlin,in_dim,out_dim", ROW_CASES)
def test_the_row_kernel_against_float64(nonlin, in_dim, out_dim, normalize):
    P = H.pkg()
    rng = np.random.default_rng(in_dim + out_dim)
    x = rng.normal(size=(9, in_dim)).astype(np.float32)
    x[3] *= 30.0
    x[4] = 0.0                                   # the normalizer's floor: 0 * 2^33
    if normalize:
        x[5] *= 2.0 ** -30                       # small rows are brought to unit mean square
    got = P.nnet2.kernel_row(x, out_dim, nonlin, normalize)
    ref64, ref32 = _row_ref(x, nonlin, out_dim, normalize, np.float64), _row_ref(x, nonlin, out_dim, normalize, np.float32)
    tol = R.tolerance(ref64, ref32)
    err = np.abs(got - ref64)
    print("row kernel %s %d -> %d normalize=%d: largest error / bound %.3g, fp32 restatement %.3g" % (
        nonlin, in_dim, out_dim, normalize, (err / np.maximum(tol, 1e-300)).max(), np.abs(ref32 - ref64).max()))
    assert got.shape == ref64.shape and np.all(err <= tol)
    assert np.all(got[4] == 0.0)
    hi, lo = P.nnet2.kernel_row(x, out_dim, nonlin, normalize, planes=True)
    assert hi.shape[1] % 32 == 0 and not hi[:, out_dim:].any() and not lo[:, out_dim:].any()   # the K padding is zero


# ------------------------------------------------------------------------------------------------------------------------ the head
def _head_ref(x, sizes, priors, log, dtype):
    p = R.softmax(x.astype(dtype))
    if sizes is not None:
        p = R.sum_group(p, sizes)
    if priors is not None:
        p = p * (dtype(1) / priors.astype(dtype))
    return np.log(np.maximum(p, dtype(R.FLOOR))) if log else p


@pytest.mark.parametrize("use_priors", [False, True])
@pytest.mark.parametrize("log", [False, True])
@pytest.mark.parametrize("n,groups,rows", [(37, 17, 5), (1100, 300, 5), (10500, 5000, 4), (65, None, 3)])
def test_the_head_against_float64(n, groups, rows, log, use_priors):
    P = H.pkg()
    rng = np.random.default_rng(n)
    x = (rng.normal(size=(rows, n)) * 3.0).astype(np.float32)
    sizes = None if groups is None else R.random_sizes(rng, n, groups)
    n_out = n if groups is None else groups
    if sizes is not None:
        sizes[:2] = sizes[:2].sum() - 1, 1       # group 1 is one column
        x[:, sizes[0]] = x.max(axis=1) - 100.0   # ... 100 below the maximum: the softmax floor, alone in its group
    else:
        x[:, 1] = x.max(axis=1) - 100.0
    priors = None
    if use_priors:
        priors = rng.uniform(0.01, 1.0, size=n_out).astype(np.float32)
        priors[1] = 4.0                          # 1e-20 / 4: the floor of the logarithm
    got = P.nnet2.kernel_head(x, sizes, priors, log)
    ref64, ref32 = _head_ref(x, sizes, priors, log, np.float64), _head_ref(x, sizes, priors, log, np.float32)
    want_floor = np.log(1e-20) if log else (1e-20 / 4.0 if use_priors else 1e-20)
    assert np.allclose(ref64[:, 1], want_floor, rtol=1e-6)   # the floors are hit on purpose
    tol = R.tolerance(ref64, ref32)
    err = np.abs(got - ref64)
    print("head %d -> %s log=%d priors=%d: largest error / bound %.3g, fp32 restatement %.3g" % (
        n, groups, log, use_priors, (err / tol).max(), np.abs(ref32 - ref64).max()))
    assert got.shape == ref64.shape and np.all(err <= tol)
    assert np.all(np.abs(got[:, 1] - ref64[:, 1]) <= 2.0 ** -22 * np.abs(ref64[:, 1]))


def test_a_row_of_the_head_does_not_depend_on_its_neighbours():
    P = H.pkg()
    rng = np.random.default_rng(3)
    x = (rng.normal(size=(6, 1100)) * 3.0).astype(np.float32)
    sizes = R.random_sizes(rng, 1100, 300)
    full = P.nnet2.kernel_head(x, sizes, None, True)
    assert np.array_equal(_bits(P.nnet2.kernel_head(x[4:5], sizes, None, True)), _bits(full[4:5]))
    assert np.array_equal(_bits(P.nnet2.kernel_head(x[::-1], sizes, None, True)), _bits(full[::-1]))
