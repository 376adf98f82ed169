"""Restatement of Kaldi's CompressedMatrix (early 2018) in numpy, fp32 THROUGHOUT: what copy-feats --compress=true writes.

Every operation below is one IEEE single-precision rounding (numpy float32 arithmetic, no fused multiply-add), which is what
the device kernels do too (csrc/compress_kernels.hip, built with contraction off and correctly rounded division): the objects
are compared for equality, not within a tolerance.  oracle/kaldi_io.py's write_compressed_matrix is a fixture writer that
computes in float64 and takes (3 * rows) // 4 for the upper quartile; this file is the semantics (csrc/compress.h).

Object layout (everything after the "CM " / "CM2 " / "CM3 " token):
  float32 min, float32 range, int32 rows, int32 cols,
  CM : uint16 percentiles[cols][4], uint8 data[cols][rows]   (column-major bytes)
  CM2: uint16 data[rows][cols]
  CM3: uint8 data[rows][cols]
"""
import struct

import numpy as np

F = np.float32
INV65535 = F(1.52590218966964e-05)

METHODS = {1: "auto", 2: "CM", 3: "CM2", 5: "CM3"}


def format_of(rows, method):
    if method not in METHODS:
        raise ValueError("compression method %d is not built (1, 2, 3 and 5 are)" % method)
    if method == 1:
        return "CM" if rows > 8 else "CM2"
    return METHODS[method]


def compressed_size(rows, cols, method=1):
    """(bytes after the token, format)"""
    fmt = format_of(rows, method)
    if rows == 0 or cols == 0:
        return 16, "CM"
    if fmt == "CM":
        return 16 + cols * 8 + rows * cols, fmt
    return 16 + rows * cols * (2 if fmt == "CM2" else 1), fmt


def global_header(m):
    """(min, range) as float32"""
    mn, mx = F(m.min()), F(m.max())
    if mn == 0:
        mn = F(0.0)                      # a zero minimum is written as +0, whichever zero the search met
    if mx == mn:
        mx = F(mn + F(F(1.0) + np.abs(mn)))
    return mn, F(mx - mn)


def to_code(x, mn, rng, top):
    """int((x - min) / range * top + 0.499), the fraction clamped to [0, 1]"""
    with np.errstate(all="ignore"):
        f = (np.asarray(x, F) - mn) / rng
        f = np.fmin(np.fmax(f, F(0.0)), F(1.0))
        return (f * F(top) + F(0.499)).astype(np.int64)


def column_header(sorted_col, mn, rng):
    """the four uint16 words of one column, forced strictly increasing"""
    s = sorted_col
    n = len(s)
    if n >= 5:
        q = n // 4
        u = to_code(np.array([s[0], s[q], s[3 * q], s[n - 1]], F), mn, rng, 65535.0)
        p0 = min(int(u[0]), 65532)
        p25 = min(max(int(u[1]), p0 + 1), 65533)
        p75 = min(max(int(u[2]), p25 + 1), 65534)
        p100 = max(int(u[3]), p75 + 1)
    else:
        u = to_code(np.asarray(s, F), mn, rng, 65535.0)
        p0 = min(int(u[0]), 65532)
        p25 = min(max(int(u[1]), p0 + 1), 65533) if n > 1 else p0 + 1
        p75 = min(max(int(u[2]), p25 + 1), 65534) if n > 2 else p25 + 1
        p100 = max(int(u[3]), p75 + 1) if n > 3 else p75 + 1
    return [p0, p25, p75, p100]


def decode_percentiles(words, mn, rng):
    """min + range * 1.52590218966964e-05f * u, left to right, as the reader does"""
    return [F(mn + F(F(rng * INV65535) * F(w))) for w in words]


def _segment(v, lo, hi, scale, base):
    """base + clamp(int((v - lo) / (hi - lo) * scale + 0.5), 0, scale); the clamp is applied before the conversion, which is the
    same for every argument an int can hold and defined for the others: an infinite argument is the last code, and 0 / 0 (the
    decoded percentiles of a column coincide when range / 65535 underflows) the first, as fmaxf / fminf give it"""
    with np.errstate(all="ignore"):
        t = (v - lo) / F(hi - lo) * F(scale) + F(0.5)
        t = np.fmin(np.fmax(t, F(0.0)), F(scale))
    return base + t.astype(np.int64)


def column_bytes(col, p):
    col = np.asarray(col, F)
    p0, p25, p75, p100 = p
    b = np.where(col < p25, _segment(col, p0, p25, 64.0, 0),
                 np.where(col < p75, _segment(col, p25, p75, 128.0, 64), _segment(col, p75, p100, 63.0, 192)))
    return b.astype(np.uint8)


def compress(m, method=1):
    """(format, object bytes) of one matrix; format "FM" and None for a matrix that is not compressed (a non-finite value, or
    a range that is not finite)."""
    m = np.asarray(m, F)
    if m.ndim != 2:
        raise ValueError("a matrix, please")
    rows, cols = m.shape
    fmt = format_of(rows, method)
    if rows == 0 or cols == 0:
        return "CM", struct.pack("<ffii", 0.0, 0.0, 0, 0)
    with np.errstate(all="ignore"):
        if not np.all(np.isfinite(m)):
            return "FM", None
        mn, rng = global_header(m)
        if not np.isfinite(rng):
            return "FM", None
    head = struct.pack("<ffii", mn, rng, rows, cols)
    if fmt == "CM2":
        return fmt, head + to_code(m, mn, rng, 65535.0).astype("<u2").tobytes()
    if fmt == "CM3":
        return fmt, head + to_code(m, mn, rng, 255.0).astype(np.uint8).tobytes()
    words = np.zeros((cols, 4), "<u2")
    data = np.zeros((cols, rows), np.uint8)
    for c in range(cols):
        w = column_header(np.sort(m[:, c]), mn, rng)
        words[c] = w
        data[c] = column_bytes(m[:, c], decode_percentiles(w, mn, rng))
    return fmt, head + words.tobytes() + data.tobytes()


def write_object(f, fmt, obj):
    """what TableWriter::WriteCompressed puts behind the key: "\\0B", the token, a space, the object"""
    f.write(b"\x00B" + fmt.encode() + b" " + obj)
