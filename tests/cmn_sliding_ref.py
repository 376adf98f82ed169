"""TEST INFRASTRUCTURE - an independent restatement of apply-cmvn-sliding --norm-vars=false and select-voiced-frames.

Not derived from the kernels (csrc/kernels.hip cmn_prefix_kernel / cmn_select_kernel) nor from oracle/frontend.py, which walks
the same branch sequence as the kernel.  Two things are stated here, each in its own way:

THE WINDOW, as a closed form per frame.  T frames, window W, minimum window M, `//` floor division; frame t's mean is taken over
the frames [s, e):

    centred:      n = min(W, T),  s = clamp(t - W // 2, 0, T - n),  e = s + n
    not centred:  e = max(t + 1, M),  s = max(t - W, 0);  if e > T: s = max(s - (e - T), 0), e = T

In the not-centred case M acts on every frame (not only where the window was shifted), and the window holds W + 1 frames once
t >= W.  Its length in one expression (derived from the two lines above: before the clip the window is e0 - s0 with
e0 = max(t + 1, M), s0 = max(t - W, 0); clipping to T moves both ends by e0 - T unless s reaches 0, where the length is T):

    e - s = min(T, max(min(t, W) + 1, M - max(t - W, 0)))

THE ARITHMETIC, exactly.  Every fp32 value is an integer multiple of 2^q for the smallest exponent q in the matrix, so the window
sum is an integer: int64 where a whole column fits (and an exact double too where it stays below 2^53 grid units), Python
integers and fractions where it does not.  Then mean = sum / n, out = float32(float64(x) - mean): one rounding per operation.

tests/test_cmn_sliding_ref.py pins this file, oracle/frontend.py and hand-computed windows against each other.
"""
import fractions

import numpy as np


def bounds(T, W, center, M=100):
    """(s, e): int64 arrays of length T, frame t's window is [s[t], e[t])."""
    t = np.arange(T, dtype=np.int64)
    if center:
        n = min(W, T)
        s = np.clip(t - W // 2, 0, T - n)
        return s, s + n
    e = np.maximum(t + 1, M)
    s = np.maximum(t - W, 0)
    over = np.maximum(e - T, 0)
    return np.maximum(s - over, 0), np.minimum(e, T)


def grid(x):
    """(k, q): the fp32 matrix x as integers on its own grid, x == k * 2^q exactly; k is an int64 array, or None when a value
    needs more than 62 bits on that grid (then use the slow path)."""
    x = np.asarray(x, dtype=np.float32)
    assert np.isfinite(x).all()
    m, ex = np.frexp(x.astype(np.float64))            # x = m * 2^ex, 0.5 <= |m| < 1, m has 24 significant bits
    nz = x != 0
    if not nz.any():
        return np.zeros(x.shape, np.int64), 0
    q = int(ex[nz].min()) - 24
    if int(ex[nz].max()) - q > 62:
        return None, q
    hi = (m * 2.0 ** 24).astype(np.int64)             # the 24-bit significand as an integer, shifted as an integer:
    return hi << np.where(nz, ex - 24 - q, 0).astype(np.int64), q      # a double would hold 53 of the 62 bits only


def sliding_cmn(x, W, center, M=100, rounded=True):
    """float32(float64(x) - (exact window sum) / n) for an fp32 matrix x [T, D]; rounded=False: the float64 before the cast."""
    x = np.asarray(x, dtype=np.float32)
    T, D = x.shape
    if T == 0:
        return np.zeros((0, D), np.float32 if rounded else np.float64)
    if W <= 0:
        return x.copy() if rounded else x.astype(np.float64)
    s, e = bounds(T, W, center, M)
    n = (e - s).astype(np.float64)[:, None]
    k, q = grid(x)
    size = float(np.abs(k).astype(np.float64).sum(axis=0).max()) if k is not None else np.inf
    if size < 2.0 ** 61:
        c = np.zeros((T + 1, D), np.int64)
        np.cumsum(k, axis=0, out=c[1:])
        total = c[e] - c[s]
        if size < 2.0 ** 52:                           # the sum is an exact double: the division rounds ONCE
            mean = np.ldexp(total.astype(np.float64), q) / n
        else:                                          # an exact int64 that no double holds: divide it as an integer, rounding once
            lens = np.broadcast_to((e - s)[:, None], total.shape)
            quot = [float(fractions.Fraction(int(a), int(b))) for a, b in zip(total.ravel(), lens.ravel())]
            mean = np.ldexp(np.array(quot, np.float64).reshape(total.shape), q)
        # (the scaling by 2^q is exact: a power of two, and fp32's range is far inside float64's)
    else:
        mean = _means_by_fractions(x, s, e)
    v = x.astype(np.float64) - mean
    return v.astype(np.float32) if rounded else v


def _means_by_fractions(x, s, e):
    """The same means without any size limit: Python integers, one correctly rounded division per element."""
    T, D = x.shape
    ints = [[fractions.Fraction(float(v)) for v in row] for row in x]       # a double holds an fp32 value exactly
    c = [[fractions.Fraction(0)] * D]
    for row in ints:
        c.append([a + b for a, b in zip(c[-1], row)])
    mean = np.empty((T, D), np.float64)
    for t in range(T):
        n = int(e[t] - s[t])
        for d in range(D):
            mean[t, d] = float((c[e[t]][d] - c[s[t]][d]) / n)              # Fraction -> float rounds to nearest even, once
    return mean


def select(feats, vad):
    """select-voiced-frames: the rows whose decision is non-zero (possibly none)."""
    feats = np.asarray(feats)
    vad = np.asarray(vad)
    assert vad.shape[0] == feats.shape[0]
    return feats[vad != 0]


def dyadic_features(seed, T, D, shift=6, kmax=1 << 12):
    """x = k * 2^-shift with integer |k| <= kmax, plus a constant per-column offset on the same grid (|offset k| <= kmax), so
    that the mean matters: |x| <= 2 kmax 2^-shift, exact in fp32 for kmax <= 2^22."""
    rng = np.random.default_rng(seed)
    k = rng.integers(-kmax, kmax + 1, size=(T, D)) + rng.integers(-kmax, kmax + 1, size=(1, D))
    return (k.astype(np.float64) * 2.0 ** -shift).astype(np.float32)


def assert_exactness_precondition(x, shift=6):
    """What makes bit equality the criterion for the device's fp64 prefix sums: every value on the grid 2^-shift, and the sum of
    the |values| of a column below 2^53 grid units - then every partial sum, in ANY order, is an exact double."""
    k = np.asarray(x, np.float64) * 2.0 ** shift
    assert np.array_equal(k, np.rint(k)), "features off the 2^-%d grid" % shift
    if k.size:
        assert np.abs(k).sum(axis=0).max() < 2.0 ** 53
