"""Per-speaker cepstral mean and variance normalisation in numpy: the restatement the library (csrc/cmvn.h) is compared with.

Restated from Kaldi's transform/cmvn.cc of early 2018 (AccCmvnStats, ApplyCmvn, ApplyCmvnReverse, FakeStatsForSomeDims):
  statistics of a rows x cols matrix: float64 [2][cols + 1]; row 0 = column sums and the frame count, row 1 = sums of squares and 0
  norm of a statistics matrix: float32 [2][cols]; row 0 = offset, row 1 = scale, all arithmetic in float64
  application: out = x * scale + offset in float32, the product and the sum each rounded on their own
"""
import math
import struct

import numpy as np

VAR_FLOOR = 1.0e-20


class CmvnError(ValueError):
    pass


def stats(x):
    """Exactly rounded statistics (math.fsum of the float64 terms; the square of a float32 is exact in float64)."""
    x = np.asarray(x, dtype=np.float32).astype(np.float64)
    rows, cols = x.shape
    st = np.zeros((2, cols + 1), dtype=np.float64)
    for d in range(cols):
        st[0, d] = math.fsum(x[:, d])
        st[1, d] = math.fsum(x[:, d] * x[:, d])
    st[0, cols] = rows
    return st


def stats_bound(x):
    """|computed - exact| <= n * 2^-53 * sum |term| per entry of stats(x), for ANY order of an fp64 summation of n terms:
    each of the n - 1 additions commits a relative error of at most u = 2^-53 on a partial sum whose magnitude is at most
    sum |term| * (1 + u)^(n - 1), so the total is below (n - 1) u (1 + u)^(n - 1) sum |term| < n u sum |term| for n u << 1
    (Higham, Accuracy and Stability of Numerical Algorithms, sec. 4.2).  The terms themselves are exact."""
    x = np.asarray(x, dtype=np.float32).astype(np.float64)
    rows, cols = x.shape
    b = np.zeros((2, cols + 1), dtype=np.float64)
    for d in range(cols):
        b[0, d] = rows * 2.0 ** -53 * math.fsum(np.abs(x[:, d]))
        b[1, d] = rows * 2.0 ** -53 * math.fsum(x[:, d] * x[:, d])
    return b


def cmvn_norm(st, norm_means=True, norm_vars=False, reverse=False, skip_dims=(), return_floored=False):
    st = np.array(st, dtype=np.float64)
    if st.ndim != 2 or st.shape[0] != 2 or st.shape[1] < 2:
        raise CmvnError("the statistics are a [2][cols + 1] matrix")
    if norm_vars and not norm_means:
        raise CmvnError("You cannot normalize the variance but not the mean.")
    cols = st.shape[1] - 1
    count = st[0, cols]
    if not count >= 1.0:
        raise CmvnError("Insufficient stats for cepstral mean and variance normalization: count = %g" % count)
    for d in skip_dims:
        if not 0 <= d < cols:
            raise CmvnError("skip-dims: dimension %d is out of range" % d)
        st[0, d] = 0.0
        st[1, d] = count
    norm = np.zeros((2, cols), dtype=np.float32)
    floored = 0
    for d in range(cols):
        if not norm_means:
            norm[0, d], norm[1, d] = 0.0, 1.0
            continue
        mean = np.float64(st[0, d]) / np.float64(count)
        scale = np.float64(1.0)
        offset = mean if reverse else -mean
        if norm_vars:
            var = np.float64(st[1, d]) / np.float64(count) - mean * mean
            if var < VAR_FLOOR:
                var = np.float64(VAR_FLOOR)
                floored += 1
            if reverse:
                scale = np.sqrt(var)
            else:
                scale = np.float64(1.0) / np.sqrt(var)
                offset = -(mean * scale)
        norm[0, d] = np.float32(offset)
        norm[1, d] = np.float32(scale)
    return (norm, floored) if return_floored else norm


def apply(x, norm):
    x = np.asarray(x, dtype=np.float32)
    norm = np.asarray(norm, dtype=np.float32)
    prod = (x * norm[1][None, :]).astype(np.float32)      # rounded to float32 ...
    return (prod + norm[0][None, :]).astype(np.float32)   # ... before the sum is formed and rounded


def read_double_matrices(path):
    """{key: float64 matrix} of a binary archive of "DM" objects (what compute-cmvn-stats writes), bits kept."""
    out = {}
    data = open(path, "rb").read()
    pos = 0
    while pos < len(data):
        sp = data.index(b" ", pos)
        key = data[pos:sp].decode()
        assert data[sp + 1:sp + 6] == b"\x00BDM ", (key, data[sp + 1:sp + 6])
        assert data[sp + 6] == 4 and data[sp + 11] == 4
        rows, = struct.unpack_from("<i", data, sp + 7)
        cols, = struct.unpack_from("<i", data, sp + 12)
        start = sp + 16
        out[key] = np.frombuffer(data, dtype="<f8", count=rows * cols, offset=start).reshape(rows, cols).copy()
        pos = start + rows * cols * 8
    return out


def read_double_matrix_file(path):
    data = open(path, "rb").read()
    assert data[:5] == b"\x00BDM " and data[5] == 4 and data[10] == 4
    rows, = struct.unpack_from("<i", data, 6)
    cols, = struct.unpack_from("<i", data, 11)
    return np.frombuffer(data, dtype="<f8", count=rows * cols, offset=15).reshape(rows, cols).copy()
