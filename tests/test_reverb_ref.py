"""The two CPU restatements of wav-reverberate (tests/reverb_ref.py) against each other and against cases computable by hand."""
import numpy as np

import reverb_ref as R

RATE = 8000.0


def test_fft64_agrees_with_direct_convolution():
    for seed, n, L in ((1, 1, 1), (2, 39, 63), (3, 8000, 64), (4, 8000, 4000), (5, 48000, 2049)):
        x = R.speechlike(seed, n).astype(np.float64)
        h = R.decaying_rir(seed, L).astype(np.float64) / 32768.0
        a, b = R.conv_direct64(x, h), R.conv_fft64(x, h)
        assert a.shape == b.shape == (n + L - 1,)
        assert np.abs(a - b).max() <= 1e-9 * max(1.0, np.abs(a).max())


def test_orientation_case_direct_against_fft():
    x = R.speechlike(11, 60 * 8000).astype(np.float64)
    h = R.decaying_rir(11, 4000).astype(np.float64) / 32768.0
    d = np.abs(R.conv_direct64(x, h) - R.conv_fft64(x, h)).max()
    print("60 s through 4000 taps: max|direct - fft64| = %.3e" % d)
    assert d <= 2e-11 * 32768


def test_ref32_stays_close_to_ref64_and_is_float32():
    x = R.speechlike(12, 16000)
    h = R.decaying_rir(12, 4000)
    noise = R.speechlike(13, 9000)
    kw = dict(rir=h, additive=[(noise, 10.0, 0.25)])
    a = R.reverberate(x, RATE, dtype=np.float64, **kw)
    b = R.reverberate(x, RATE, dtype=np.float32, **kw)
    assert b.dtype == np.float32 and a.dtype == np.float64 and a.shape == b.shape == (16000,)
    err = np.abs(a - b).max()
    assert 0 < err < 1e-5 * np.abs(a).max()


def test_unit_impulse_returns_the_input():
    x = R.speechlike(14, 5000)
    for k in (0, 7, 300):
        h = np.zeros(k + 1)
        h[k] = 32768.0                                    # 1.0 after the scaling; the power over the k samples longer
                                                          # signal is lower, so normalisation would scale by sqrt((n + k) / n)
        for dt in (np.float64, np.float32):
            y = R.reverberate(x, RATE, rir=h, normalize_output=False, dtype=dt)                     # shifted back by the peak
            assert y.shape == (5000,) and np.abs(y - x).max() < (1e-9 if dt == np.float64 else 2e-2)
            z = R.reverberate(x, RATE, rir=h, shift_output=False, normalize_output=False, dtype=dt)  # the whole tail, delayed by k
            assert z.shape == (5000 + k,)
            assert np.abs(z[k:] - x).max() < (1e-9 if dt == np.float64 else 2e-2) and np.abs(z[:k]).max(initial=0.0) < 2e-2


def test_duration_shorter_and_longer_than_the_input():
    x = R.speechlike(15, 4000)
    y = R.reverberate(x, RATE, duration=0.25)
    assert y.shape == (2000,) and np.array_equal(y, x[:2000].astype(np.float64))
    z = R.reverberate(x, RATE, duration=1.25)
    assert z.shape == (10000,)
    assert np.array_equal(z[:4000], x) and np.array_equal(z[4000:8000], x) and np.array_equal(z[8000:], x[:2000])
    h = R.decaying_rir(15, 100)
    w = R.reverberate(x, RATE, rir=h, duration=1.25, normalize_output=False)     # repeats the extended signal, unshifted
    full = R.conv_direct64(x.astype(np.float64), h / 32768.0)
    assert np.allclose(w[:4099], full) and np.allclose(w[4099:8198], full)


def test_snr_of_zero_db_against_a_signal_of_known_power():
    n = 8000
    x = np.full(n, 1000.0) * np.where(np.arange(n) % 2, 1, -1)      # power 1e6
    noise = np.full(n, 10.0) * np.where(np.arange(n) % 4 < 2, 1, -1)  # power 100
    y = R.reverberate(x, RATE, additive=[(noise, 0.0, 0.0)], normalize_output=False)
    added = y - x
    assert abs(np.dot(added, added) / n - 1e6) < 1e-3              # scaled to the signal's power
    y20 = R.reverberate(x, RATE, additive=[(noise, 20.0, 0.0)], normalize_output=False)
    assert abs(np.dot(y20 - x, y20 - x) / n - 1e4) < 1e-5


def test_start_times_at_and_beyond_the_end():
    x = R.speechlike(16, 8000)
    noise = R.speechlike(17, 4000)
    a = R.reverberate(x, RATE, additive=[(noise, 5.0, 1.0)], normalize_output=False)     # exactly at the end: nothing added
    b = R.reverberate(x, RATE, additive=[(noise, 5.0, 2.5)], normalize_output=False)
    assert np.array_equal(a, x) and np.array_equal(b, x)
    c = R.reverberate(x, RATE, additive=[(noise, 5.0, 0.75)], normalize_output=False)    # cut where the signal ends
    assert np.array_equal(c[:6000], x[:6000]) and not np.array_equal(c[6000:], x[6000:])


def test_normalisation_keeps_the_power():
    x = R.speechlike(18, 12000)
    h = R.decaying_rir(18, 900)
    noise = R.speechlike(19, 12000)
    for dt, tol in ((np.float64, 1e-12), (np.float32, 1e-5)):
        y = R.reverberate(x, RATE, rir=h, additive=[(noise, 3.0, 0.0)], shift_output=False, dtype=dt).astype(np.float64)
        p_in = np.dot(x.astype(np.float64), x.astype(np.float64)) / len(x)
        assert abs(np.dot(y, y) / len(y) - p_in) <= tol * p_in
    v = R.reverberate(x, RATE, volume=0.5)
    assert np.array_equal(v, 0.5 * x)


def test_quantize_truncates_toward_zero_and_saturates():
    q, c = R.quantize(np.array([0.9, -0.9, 1.5, -1.5, 32767.9, 32768.0, -32768.9, -32769.0, 1e9]))
    assert q.tolist() == [0, 0, 1, -1, 32767, 32767, -32768, -32768, 32767] and c == 3
