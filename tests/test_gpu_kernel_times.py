"""GPU tests of the timed paths: every entry point that returns a kernel time (xv_*_kernel_time, and the device_ms outputs of the
PLDA entry points) is called once at the smallest shape that still runs each of its kernels.  A time must be finite and above
zero - the shared event timer (csrc/device.h) records around the launches and reads back - and where the call returns results
too, they are the bits of the untimed call.  No upper bound is asserted on any time."""
import ctypes
import math

import numpy as np
import pytest

import helpers as H
import ivector_ref as IR

pytestmark = pytest.mark.gpu
P = H.pkg()


def _valid(ms):
    return math.isfinite(ms) and ms > 0.0


def test_mfcc():
    """xv_mfcc_compute_i16 takes no device_ms, so the timed launches are those of xv_mfcc_kernel_time, which returns no features:
    the features of the untimed entry point are compared before and after it."""
    rng = np.random.default_rng(1)
    waves = [rng.integers(-20000, 20000, n).astype(np.int16) for n in (400, 1000)]
    conf = dict(sample_frequency=8000.0, frame_length=25.0, low_freq=20.0, high_freq=3700.0, dither=0.0)
    before = P.mfcc(waves, **conf)
    assert [f.shape for f in before] == [(3, 13), (11, 13)]
    L = P.lib()
    o = P.mfcc_options(**conf)
    samples = np.concatenate(waves)
    off = np.array([0, 400, 1400], np.int64)
    ms = ctypes.c_float(0)
    P._check(L.xv_mfcc_kernel_time(0, ctypes.byref(o), samples.ctypes.data, off.ctypes.data, 2, 2, ctypes.byref(ms)))
    print("mfcc %.4f ms" % ms.value)
    assert _valid(ms.value)
    after = P.mfcc(waves, **conf)
    for a, b in zip(before, after):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_reverberation():
    rng = np.random.default_rng(2)
    wave = rng.normal(0.0, 3000.0, 2000).astype(np.float32)
    rir = (rng.normal(0.0, 1.0, 300) * np.exp(-np.arange(300) / 60.0) * 8000.0).astype(np.float32)
    noise = rng.normal(0.0, 1000.0, 500).astype(np.float32)
    args = dict(rirs=[rir], additive=[[(noise, 10.0, 0.0)]])
    ms = P.reverberate([wave], kernel_time_reps=1, **args)
    print("reverberation %.4f ms" % ms)
    assert _valid(ms)


def test_compression():
    """9 rows under method 1 are a CM object (the selection kernel runs), 3 rows a CM2 one"""
    rng = np.random.default_rng(3)
    mats = [rng.normal(0.0, 5.0, (9, 5)).astype(np.float32), rng.normal(0.0, 5.0, (3, 5)).astype(np.float32)]
    assert [P.compressed_size(m.shape[0], 5, 1)[1] for m in mats] == ["CM", "CM2"]
    ms = P.compress(mats, method=1, kernel_time_reps=1)
    print("compression %.4f ms" % ms)
    assert _valid(ms)


def test_cmvn():
    rng = np.random.default_rng(4)
    mats = [rng.normal(0.0, 5.0, (7, 5)).astype(np.float32), rng.normal(0.0, 5.0, (1, 5)).astype(np.float32)]
    stats_ms, apply_ms = P.cmvn_stats(mats, kernel_time_reps=1)
    print("cmvn statistics %.4f ms, apply %.4f ms" % (stats_ms, apply_ms))
    assert _valid(stats_ms) and _valid(apply_ms)


def test_ubm():
    G, D = 4, 6   # 2 columns with their deltas
    rng = np.random.default_rng(5)
    eye = np.eye(D)[np.tril_indices(D)].astype(np.float32)
    diag = P.Ubm.diag(np.zeros(G, np.float32), rng.integers(-3, 4, (G, D)).astype(np.float32), np.ones((G, D), np.float32))
    full = P.Ubm.full(np.zeros(G, np.float32), rng.integers(-2, 3, (G, D)).astype(np.float32), np.tile(eye, (G, 1)))
    feats = [rng.integers(-4, 5, (t, D)).astype(np.float32) for t in (15, 25)]
    ms = P.ubm_kernel_time(diag, full, feats, n=2, reps=1)
    print("ubm", ms)
    assert sorted(ms) == ["deltas", "full", "gselect", "softmax", "sort"]
    assert all(_valid(v) for v in ms.values()), ms


def test_ivector():
    G, D, S = 4, 5, 8
    ie = P.IvectorExtractor(**IR.integer_model(6, G, D, S))
    utts = [IR.integer_utterance(7 + u, t, G, D) for u, t in enumerate((12, 30))]
    ms = ie.kernel_time([x for x, _ in utts], [p for _, p in utts], reps=1)
    print("i-vector", ms)
    assert sorted(ms) == ["derive", "linear", "quadratic", "solve", "stats"]
    assert all(_valid(v) for v in ms.values()), ms


# ------------------------------------------------------------------------------------------------------------------- PLDA
def _twice(fn, args, outputs):
    """fn(*args, device_ms) with device_ms NULL and then with a float: (the outputs' bytes of each call, the time)"""
    got = []
    ms = ctypes.c_float(0)
    for device_ms in (None, ctypes.byref(ms)):
        for o in outputs:
            o.fill(0)
        P._check(fn(*args, device_ms))
        got.append([o.tobytes() for o in outputs])
    return got[0], got[1], ms.value


def test_plda():
    dim, n = 8, 6
    rng = np.random.default_rng(8)
    x = rng.normal(0.0, 1.0, (n, dim)).astype(np.float32)
    segments = [[0, 1, 2, 3], [4, 5]]
    L = P.lib()
    # the package's own calls set the argument types (and are the timed calls of the Python interface)
    s_tot, sums, s_bet, ms_py = P.scatter_stats(x, segments, return_ms=True)
    assert _valid(ms_py)
    off, idx = P._segments(segments)
    outs = [np.empty((dim, dim)), np.empty((2, dim)), np.empty((dim, dim))]
    a, b, ms = _twice(L.xv_scatter_stats, (0, x.ctypes.data, n, dim, off.ctypes.data, idx.ctypes.data, 2, outs[0].ctypes.data,
                                           outs[1].ctypes.data, outs[2].ctypes.data), outs)
    print("scatter statistics %.4f ms" % ms)
    assert _valid(ms) and a == b == [s_tot.tobytes(), sums.tobytes(), s_bet.tobytes()]

    t = rng.normal(0.0, 1.0, (dim, dim))
    offset, psi, num = rng.normal(0.0, 1.0, dim), rng.uniform(0.5, 2.0, dim), np.array([1.0, 2.0, 1.0, 3.0, 1.0, 1.0])
    y, scale, ms_py = P.plda_transform(x, t, offset, psi, num=num, return_ms=True)
    assert _valid(ms_py)
    outs = [np.empty((n, dim), np.float32), np.empty(n)]
    a, b, ms = _twice(L.xv_plda_transform, (0, x.ctypes.data, n, dim, t.ctypes.data, offset.ctypes.data, psi.ctypes.data, num.ctypes.data,
                                            1, 0, outs[0].ctypes.data, outs[1].ctypes.data), outs)
    print("transform %.4f ms" % ms)
    assert _valid(ms) and a == b == [y.tobytes(), scale.tobytes()]

    trials = np.array([[0, 0], [1, 5], [3, 2], [2, 2], [1, 0]], np.int32)
    scores, ms_py = P.plda_score(y[:4], num[:4], y, psi, trials, return_ms=True)
    assert _valid(ms_py)
    u = np.ascontiguousarray(y[:4])
    nu = np.ascontiguousarray(num[:4])
    outs = [np.empty(len(trials))]
    a, b, ms = _twice(L.xv_plda_score, (0, u.ctypes.data, nu.ctypes.data, 4, y.ctypes.data, n, dim, psi.ctypes.data, trials.ctypes.data,
                                        len(trials), outs[0].ctypes.data), outs)
    print("scoring %.4f ms" % ms)
    assert _valid(ms) and a == b == [scores.tobytes()]
