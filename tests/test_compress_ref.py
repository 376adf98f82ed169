"""tests/compress_ref.py (the fp32 restatement of Kaldi's CompressedMatrix) against the independent reader and the fixture
writer of oracle/kaldi_io.py.  The fixture writer computes in float64 and takes (3 * rows) // 4 for the upper quartile, so the
comparisons with it use data whose codes do not depend on the width of the arithmetic: integers on the code grid itself
(min 0, max 65535 or 255: (x - min) / range * top is x to within 2^-7, far from the .501 where a code changes)."""
import io
import struct

import numpy as np
import pytest

import compress_ref as C
import helpers as H  # noqa: F401  (puts the repository root on sys.path)
from oracle import kaldi_io as kio


def grid(seed, rows, cols, top):
    rng = np.random.default_rng(seed)
    m = rng.integers(0, top + 1, size=(rows, cols)).astype(np.float32)
    m[0, 0], m[-1, -1] = 0.0, float(top)
    return m


def read_back(fmt, obj):
    buf = io.BytesIO()
    buf.write(b"k ")
    C.write_object(buf, fmt, obj)
    buf.seek(0)
    (key, m), = list(kio.read_ark(buf, "matrix"))
    assert key == "k"
    return m


def step_bound(m, fmt, obj):
    """What the format itself promises for every element, from the header: half a code step of the value's segment plus one
    step of the 16-bit percentile grid (range / 65535: the ends of a column's outer segments are rounded onto it), and 4 ulp
    of slack for the fp32 operations of encoder and decoder."""
    mn, rng, rows, cols = struct.unpack("<ffii", obj[:16])
    slack = 4 * np.spacing(np.float32(max(abs(mn), abs(mn + rng))))
    if fmt == "CM2":
        return np.full(m.shape, 0.5 * rng / 65535 + rng / 65535 + slack)
    if fmt == "CM3":
        return np.full(m.shape, 0.5 * rng / 255 + rng / 65535 + slack)
    words = np.frombuffer(obj[16:16 + cols * 8], "<u2").reshape(cols, 4).astype(np.float64)
    p = mn + rng * words / 65535.0
    bound = np.empty(m.shape)
    for c in range(cols):
        v = m[:, c]
        seg = np.where(v < p[c, 1], (p[c, 1] - p[c, 0]) / 64, np.where(v < p[c, 2], (p[c, 2] - p[c, 1]) / 128, (p[c, 3] - p[c, 2]) / 63))
        bound[:, c] = 0.5 * seg + rng / 65535 + slack
    return bound


@pytest.mark.parametrize("method,fmt", [(2, "CM"), (3, "CM2"), (5, "CM3"), (1, "CM")])
def test_objects_are_read_back_within_the_formats_own_bound(method, fmt):
    rng = np.random.default_rng(5)
    m = (rng.standard_normal((57, 23)) * np.linspace(0.1, 30, 23)).astype(np.float32)
    m[:, 4] = 1.25                                    # a constant column inside a varying matrix
    got_fmt, obj = C.compress(m, method)
    assert got_fmt == fmt and len(obj) == C.compressed_size(57, 23, method)[0]
    back = read_back(fmt, obj)
    assert back.shape == m.shape
    err = np.abs(back.astype(np.float64) - m)
    bound = step_bound(m, fmt, obj)
    assert (err <= bound).all(), float((err / bound).max())


def test_automatic_method_flips_between_eight_and_nine_rows():
    m = np.random.default_rng(1).standard_normal((9, 5)).astype(np.float32)
    assert C.compress(m[:8], 1)[0] == "CM2" and C.compress(m, 1)[0] == "CM"
    for bad in (0, 4, 6, 7, 8):
        with pytest.raises(ValueError):
            C.compress(m, bad)


@pytest.mark.parametrize("method,fmt,top", [(3, "CM2", 65535), (5, "CM3", 255)])
def test_cm2_and_cm3_bytes_equal_the_fixture_writer(method, fmt, top):
    m = grid(2, 37, 23, top)
    buf = io.BytesIO()
    kio.write_compressed_matrix(buf, m, fmt)
    assert buf.getvalue() == fmt.encode() + b" " + C.compress(m, method)[1]


@pytest.mark.parametrize("rows", [8, 12, 64, 1000])
def test_cm_column_headers_equal_the_fixture_writers_when_rows_divide_by_four(rows):
    m = grid(rows, rows, 23, 65535)
    buf = io.BytesIO()
    kio.write_compressed_matrix(buf, m, "CM")
    theirs = buf.getvalue()[3:]
    ours = C.compress(m, 2)[1]
    assert ours[:16 + 23 * 8] == theirs[:16 + 23 * 8]


def test_the_upper_quartile_is_s_3q_not_s_3rows_over_4():
    """rows = 10: q = 2, 3 q = 6, while (3 * rows) // 4 = 7; the column is 0, 1000, 2000 ... so that the two differ."""
    m = np.zeros((10, 2), np.float32)
    m[:, 0] = np.arange(10) * 1000.0
    m[:, 1] = 65535.0 * (np.arange(10) % 2)           # spans the grid: min 0, range 65535
    perm = np.random.default_rng(3).permutation(10)
    obj = C.compress(m[perm], 2)[1]
    words = np.frombuffer(obj[16:32], "<u2").reshape(2, 4)
    assert words[0].tolist() == [0, 2000, 6000, 9000]


def test_short_columns_degenerate_ranges_and_empty_objects():
    # rows < 5, method 2: s[0..3] where they exist, the word before plus one where they do not
    m = np.array([[0.0], [65535.0], [30000.0]], np.float32)
    words = np.frombuffer(C.compress(m, 2)[1][16:24], "<u2")
    assert words.tolist() == [0, 30000, 65534, 65535]              # p75 = min(u16(s[2]), 65534), p100 = p75 + 1: there is no s[3]
    one = np.array([[7.0, 7.0]], np.float32)
    mn, rng, rows, cols = struct.unpack("<ffii", C.compress(one, 2)[1][:16])
    assert (mn, rng, rows, cols) == (7.0, 8.0, 1, 2)            # max == min: range = 1 + |min|
    assert np.frombuffer(C.compress(one, 2)[1][16:24], "<u2").tolist() == [0, 1, 2, 3]
    mn, rng, _, _ = struct.unpack("<ffii", C.compress(np.full((9, 3), -3.5, np.float32), 1)[1][:16])
    assert (mn, rng) == (-3.5, 4.5)
    for shape in ((0, 23), (5, 0), (0, 0)):
        assert C.compress(np.zeros(shape, np.float32), 1) == ("CM", b"\0" * 16)
        assert C.compressed_size(shape[0], shape[1], 3) == (16, "CM")
    for bad in (np.nan, np.inf, -np.inf):
        m = np.ones((9, 3), np.float32)
        m[4, 1] = bad
        assert C.compress(m, 1) == ("FM", None)
