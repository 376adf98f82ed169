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


# ------------------------------------------------------------------------------------------------------------------
# The additions for tests/test_gpu_reverb_edges.py, and what its cases (tests/reverb_edges.py) have to fulfil: exact
# arithmetic where the GPU test compares bytes, and that the mistake a case is there to catch moves the fp64 reference
# far beyond the bar the GPU is held to.
import warnings  # noqa: E402

import reverb_edges as E  # noqa: E402


def test_fft4096_32_is_the_transform():
    rng = np.random.default_rng(20)
    re, im = rng.standard_normal((3, R.PART_N)).astype(np.float32), rng.standard_normal((3, R.PART_N)).astype(np.float32)
    a, b = R.fft4096_32(re, im)
    assert a.dtype == b.dtype == np.float32
    want = np.fft.fft(re.astype(np.float64) + 1j * im.astype(np.float64), axis=1)
    assert np.abs(a + 1j * b - want).max() <= 1e-6 * np.abs(want).max()


def test_partitioned32_agrees_with_direct_convolution():
    for seed, n, L in ((21, 1, 1), (22, 39, 65), (23, 1, E.H + 1), (24, 2 * E.H + 7, E.H), (25, 3 * E.H - 1, 3 * E.H + 5)):
        x = R.speechlike(seed, n)
        h = R.flat_rir(seed, L, min(L - 1, 20)).astype(np.float64) / 32768.0
        a, b = R.conv_direct64(x, h), R.conv_partitioned32(x, h)
        assert b.dtype == np.float32 and a.shape == b.shape == (n + L - 1,)
        assert np.abs(a - b).max() <= 2e-6 * np.abs(a).max()


def test_flat_rir_has_no_decay_and_its_peak_where_asked():
    h = R.flat_rir(26, 8 * E.H + 1, 20)
    assert h.dtype == np.int16 and int(np.argmax(h)) == 20 and h[20] == 20000 and np.abs(np.delete(h, 20)).max() <= 12000
    e = [float(np.square(h[p * E.H:(p + 1) * E.H].astype(np.float64)).mean()) for p in range(1, 8)]
    assert max(e) < 1.2 * min(e)


def test_the_constants_are_the_ones_the_cases_were_laid_out_for():
    assert E.DMAX < E.H < E.DC < E.C and E.DC % E.H == 0 and E.C % E.DC == 0 and R.PART_N == 2 * E.H


def test_quantize_at_the_thresholds_without_a_warning():
    v = np.array([t[0] for t in E.THRESHOLDS], np.float32)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        q, c = R.quantize(v)
    assert q.dtype == np.int16 and q.tolist() == [t[1] for t in E.THRESHOLDS]
    assert c == sum(t[2] for t in E.THRESHOLDS) == 5
    for val, want, clipped in E.THRESHOLDS:                      # one by one: the count is of exactly these
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            assert R.quantize(np.array([val])) == (np.array([want], np.int16), int(clipped))
    for x, q, count in E.threshold_rotations() + E.count_utterances():
        got, c = R.quantize(x)
        assert np.array_equal(got, q) and c == count
    assert sorted(u[2] for u in E.count_utterances()) == [0, 1, 4, 6]


def test_section1_sums_are_exact():
    """Integer taps and samples: every sum is an integer over 32768 below 2^12, exact in fp64 in any order and in fp32."""
    names = dict(E.direct_filters())
    assert E.peak_of(names["L=%d tie 5, 40" % E.DMAX]) == 5 and E.peak_of(names["L=%d all negative" % E.DMAX]) == 7
    assert names["L=%d all negative" % E.DMAX].max() == -1
    assert len(E.section1_cases()) == 8 * 6
    for c in E.section1_cases():
        exact = np.convolve(c.x.astype(np.int64), c.rir.astype(np.int64))
        full = R.conv_direct64(c.x, c.rir.astype(np.float64) / 32768.0)
        assert np.array_equal(full * 32768.0, exact) and np.abs(exact).max() < 2 ** 12, c.name
        assert np.array_equal(full.astype(np.float32).astype(np.float64), full)
        for shift in (False, True):
            want = R.reverberate(c.x, 8000.0, rir=c.rir, shift_output=shift, volume=1.0)
            assert np.array_equal(E.direct_expect(c, shift).astype(np.float64), want), c.name
    ext = sorted({len(c.x) + len(c.rir) - 1 for c in E.section1_cases() if len(c.rir) == E.DMAX})
    assert ext == [E.DMAX, E.DMAX + 1, E.DC - 1, E.DC, E.DC + 1, 2 * E.DC + 1]


def _share_beyond(a, b, bar):
    return float((np.abs(a - b) > bar).mean())


def test_section2_a_slice_one_tap_off_moves_half_of_the_samples_beyond_the_bar():
    assert R.early_slice(E.section2_cases(400.0)[12].rir, 400.0) == (30, 30, 50)        # strictly inside the filter
    worst = (1.0, None)
    for rate in (8000.0, 400.0):
        for idx, c in enumerate(E.section2_cases(rate)):
            r64, bar = E.section2_ref(rate, idx)
            assert len(c.additive[0][0]) == len(r64) + 7
            moves = E.slice_moves(c.rir, rate)
            assert moves
            for mv in moves:
                m64 = R.reverberate(c.x, rate, rir=c.rir, additive=c.additive, early_taps=mv, **E.SECTION2_OPTS)
                share = _share_beyond(m64, r64, bar)
                worst = min(worst, (share, (c.name, mv)))
                assert share >= 0.5, (c.name, mv, share)
    print("section 2: smallest share of samples a one-tap move of the slice puts beyond the bar: %.3f at %s" % worst)


def test_section3_a_lost_partition_or_last_tap_moves_the_reference_a_thousand_bars():
    """Asserted on the whole convolution (shift_output=false); the shifted output is a slice of the same samples, of which
    a short signal's does not reach the later partitions at all."""
    worst = (np.inf, None)
    cases = E.section3_cases()
    assert len(cases) == 10 * 5 and all(np.abs(c.x).max() > 0 for c in cases)
    for idx, c in enumerate(cases):
        for shift in (False, True):
            r64, e32, e32p, bar = E.section3_ref(idx, shift)
            assert e32p <= bar and e32 <= bar and bar > 0
            print("section 3 %s, shift %d: e32 %.3e  e32p %.3e  e32p/e32 %.2f" % (c.name, shift, e32, e32p, e32p / max(e32, 1e-300)))
        r64, _, _, bar = E.section3_ref(idx, False)
        L = len(c.rir)
        cuts = [(p * E.H, min(L, (p + 1) * E.H)) for p in range(E.partitions(L))] + [(L - 1, L)]
        for a, b in cuts:
            h = c.rir.copy()
            h[a:b] = 0
            moved = float(np.abs(R.reverberate(c.x, 8000.0, rir=h, shift_output=False, volume=1.0) - r64).max())
            worst = min(worst, (moved / bar, (c.name, a, b)))
            assert moved >= 1000 * bar, (c.name, a, b, moved, bar)
    print("section 3: smallest (zeroed partition or last tap) / bar: %.0f at %s" % worst)


def test_section4_slices_are_the_ones_the_rates_were_chosen_for():
    h = E.section4_cases(8000.0)[4].rir
    assert E.peak_of(h) == E.H + 52
    got = [(R.early_slice(h, r)[2] - R.early_slice(h, r)[1], E.early_partitions(h, r)) for r in E.SECTION4_RATES]
    assert got == [(408, 1), (E.H, 1), (E.H + 1, 2), (2448, 2)]
    assert R.early_slice(h, 48000.0) == (E.H + 52, E.H + 4, E.H + 52 + 2400)      # starts inside the second partition
    assert sum(E.early_partitions(c.rir, r) == 2 for r in E.SECTION4_RATES for c in E.section4_cases(r)) >= 8


def test_section4_a_slice_one_tap_off_or_cut_at_a_partition_moves_the_reference_four_bars():
    worst, worst_cut = (np.inf, None), (np.inf, None)
    for rate in E.SECTION4_RATES:
        for idx, c in enumerate(E.section4_cases(rate)):
            r64, e32, e32p, bar = E.section4_ref(rate, idx)
            assert e32p <= bar and len(c.additive[0][0]) == len(r64) + 1
            print("section 4 %s: e32 %.3e  e32p %.3e" % (c.name, e32, e32p))
            _, e0, e1 = R.early_slice(c.rir, rate)
            moves = [(mv, False) for mv in E.slice_moves(c.rir, rate)]
            if E.early_partitions(c.rir, rate) == 2:
                moves.append(((e0, e0 + E.H), True))
            for mv, cut in moves:
                m64 = R.reverberate(c.x, rate, rir=c.rir, additive=c.additive, early_taps=mv, **E.SECTION4_OPTS)
                moved = float(np.abs(m64 - r64).max())
                if cut:
                    worst_cut = min(worst_cut, (moved / bar, (c.name, mv)))
                else:
                    worst = min(worst, (moved / bar, (c.name, mv)))
                assert moved >= 4 * bar, (c.name, mv, moved, bar)
    print("section 4: smallest one-tap move / bar: %.1f at %s; smallest cut to one partition / bar: %.1f at %s" % (worst + worst_cut))


def test_section5_reference_is_all_integers_and_ref32_equals_ref64():
    assert np.dot(E.sign3(E.C + 1, 4), E.sign3(E.C + 1, 4)) == 16 * (E.C + 1)
    for idx, c in enumerate(E.section5_cases()):
        r64 = E.section5_ref(idx, False)
        assert np.array_equal(r64, np.round(r64)) and np.abs(r64).max() <= 16, c.name
        for noise, snr, start in c.additive:
            assert float(np.float32(start)) * E.RATE5 == int(start * E.RATE5) and set(np.abs(noise)) <= {1.0, 2.0}
        r32 = R.reverberate(c.x, E.RATE5, additive=c.additive, volume=1.0, dtype=np.float32)
        assert np.array_equal(r32.astype(np.float64), r64), c.name
        if any(int(s * E.RATE5) < len(c.x) for _, _, s in c.additive):
            assert not np.array_equal(r64, c.x), c.name
    # what a chunk counted one sample short does to the normalised output, against the 2^-22 it is held to
    n = 2 * E.C + 1
    assert abs(np.sqrt(1.0 - 1.0 / n) - 1.0) > 32 * E.ULP4


def test_section6_trim_and_repeat_expectations_are_exact():
    x = E.int_signal(6100, E.TRIM_N)
    for shift in (False, True):
        for out_len in E.trim_out_lens():
            y = E.trim_expect(x, E.trim_rir(), shift, out_len)
            assert np.array_equal(y.astype(np.float64) * 32768.0, np.round(y.astype(np.float64) * 32768.0))
    ext = E.TRIM_N + E.DMAX - 1
    full = R.conv_direct64(x, E.trim_rir().astype(np.float64) / 32768.0)
    assert np.array_equal(E.trim_expect(x, E.trim_rir(), True, E.TRIM_N), full[20:20 + E.TRIM_N].astype(np.float32))
    assert np.array_equal(E.trim_expect(x, E.trim_rir(), True, E.TRIM_N + 1), full[:E.TRIM_N + 1].astype(np.float32))     # no shift
    assert np.array_equal(E.trim_expect(x, E.trim_rir(), False, ext + 1)[-1:], full[:1].astype(np.float32))             # wraps
