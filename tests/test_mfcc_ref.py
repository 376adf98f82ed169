"""CPU checks of tests/mfcc_ref.py (the yardstick of tests/test_gpu_mfcc.py) that do not reuse its code: hand-worked frame
counts and first samples, the FFT against a direct DFT, orthonormal DCT rows, a tone in the right mel filter, Parseval, and a
hand-worked VAD sequence."""
import numpy as np
import pytest

import mfcc_ref as R


def test_dct_rows_are_orthonormal():
    for nb, nc in ((23, 23), (23, 13), (40, 20)):
        m = R.dct_matrix(R.options(num_mel_bins=nb, num_ceps=nc))
        np.testing.assert_allclose(m @ m.T, np.eye(nc), atol=1e-12)
    m32 = R.dct_matrix(R.options(), np.float32)
    assert m32.dtype == np.float32
    np.testing.assert_allclose(m32 @ m32.T, np.eye(13), atol=1e-6)


@pytest.mark.parametrize("P", [2, 8, 256, 512])
def test_fft_equals_a_direct_dft(P):
    rng = np.random.default_rng(P)
    x = rng.standard_normal((3, P))
    k = np.arange(P)
    dft = x @ np.exp(-2j * np.pi * np.outer(k, k) / P)     # X[k] = sum_n x[n] exp(-2 pi i n k / P)
    re, im = R.fft_radix2(x, np.zeros_like(x))
    np.testing.assert_allclose(re + 1j * im, dft, atol=1e-9 * P)
    re32, im32 = R.fft_radix2(x, np.zeros_like(x), np.float32)
    assert re32.dtype == np.float32 and im32.dtype == np.float32
    np.testing.assert_allclose(re32 + 1j * im32, dft, atol=3e-6 * P)
    assert np.abs(re32 - re).max() > 0       # it really computed in fp32


def test_frame_counts_and_first_samples_hand_worked():
    # 8 kHz, 25 ms / 10 ms: L = 200, S = 80, P = 256
    snip = R.options(**R.CONF_MFCC_SNIP_EDGE)
    assert R.geometry(snip) == (200, 80, 256)
    assert R.geometry(R.options()) == (400, 160, 512)
    for n, f in ((0, 0), (1, 0), (199, 0), (200, 1), (279, 1), (280, 2), (8000, 98)):
        assert R.num_frames(n, snip) == f, n
    assert [R.first_sample(t, snip) for t in range(3)] == [0, 80, 160]
    idx = R.frame_indices(280, snip)
    assert idx.shape == (2, 200) and idx[0, 0] == 0 and idx[1, 0] == 80 and idx[1, -1] == 279
    # snip-edges=false: (n + 40) // 80 frames, frame t starts at 80 t + 40 - 100
    ns = R.options(**R.CONF_MFCC)
    for n, f in ((0, 0), (1, 0), (39, 0), (40, 1), (119, 1), (120, 2), (200, 3), (8000, 100)):
        assert R.num_frames(n, ns) == f, n
    assert [R.first_sample(t, ns) for t in range(3)] == [-60, 20, 100]
    idx = R.frame_indices(200, ns)
    assert idx.shape == (3, 200)
    # reflection at the start: samples -60 .. -1 read 59 .. 0
    assert list(idx[0, :62]) == list(range(59, -1, -1)) + [0, 1]
    # reflection at the end: frame 2 starts at 100; positions 200 .. 299 read 199 .. 100
    assert list(idx[2, 98:103]) == [198, 199, 199, 198, 197] and idx[2, -1] == 100
    # a waveform far shorter than the window reflects more than once and stays inside
    idx = R.frame_indices(40, ns)
    assert idx.shape == (1, 200) and idx.min() == 0 and idx.max() == 39
    assert list(idx[0, 58:64]) == [1, 0, 0, 1, 2, 3] and list(idx[0, 98:103]) == [38, 39, 39, 38, 37]


def test_pure_tone_lands_in_the_mel_filter_that_contains_it():
    o = R.options(**R.CONF_MFCC, dither=0.0)
    L, S, P = R.geometry(o)
    bank = R.mel_bank(o)
    assert bank.shape == (23, 129) and bank.min() >= 0 and bank.max() <= 1 and not bank[:, -1].any()
    mel = lambda f: 1127.0 * np.log(1.0 + f / 700.0)
    edges = mel(20.0) + (mel(3700.0) - mel(20.0)) / 24 * np.arange(25)
    for freq in (250.0, 1000.0, 2500.0, 3500.0):
        t = np.arange(4000)
        x = 10000.0 * np.sin(2 * np.pi * freq * t / 8000.0)
        w, _ = R.windowed_frames(x, R.options(**R.CONF_MFCC, dither=0.0, preemphasis_coefficient=0.0))
        pad = np.zeros((w.shape[0], P))
        pad[:, :L] = w
        power = np.abs(np.fft.rfft(pad, axis=1)) ** 2
        best = int(np.argmax(power[10] @ bank.T))
        centre = edges[best + 1]
        assert abs(mel(freq) - centre) <= (edges[1] - edges[0]), (freq, best)   # within one filter spacing of its centre
        assert edges[best] < mel(freq) < edges[best + 2]


def test_parseval_on_the_windowed_frame():
    rng = np.random.default_rng(5)
    o = R.options(dither=0.0)
    L, S, P = R.geometry(o)
    x = rng.standard_normal(4000) * 3000
    w, _ = R.windowed_frames(x, o)
    pad = np.zeros((w.shape[0], P))
    pad[:, :L] = w
    re, im = R.fft_radix2(pad, np.zeros_like(pad))
    full = (re * re + im * im).sum(axis=1)           # all P bins
    np.testing.assert_allclose(full / P, (w * w).sum(axis=1), rtol=1e-10)


def test_silence_row_closed_form():
    o = R.options(**R.CONF_MFCC, dither=0.0)
    row = R.mfcc(np.zeros(2000), o)
    np.testing.assert_allclose(row, np.tile(R.silence_row(o), (row.shape[0], 1)), atol=1e-9)
    # all log mel energies equal: only the first DCT row sees them
    le = np.log(float(np.finfo(np.float32).eps))
    assert abs(row[0, 0] - le) < 1e-12 and np.abs(row[0, 1:]).max() < 1e-9
    o2 = R.options(**R.CONF_MFCC, dither=0.0, use_energy=False)
    assert abs(R.mfcc(np.zeros(2000), o2)[0, 0] - np.sqrt(23.0) * le) < 1e-9


def test_vad_hand_worked_sequence():
    # thr = 5.5 + 0.5 * mean; c0 below: mean = 3.2 -> thr = 7.1; above-threshold frames: 2, 3, 7
    c0 = np.array([1.0, 2.0, 9.0, 8.0, 1.0, 1.0, 1.0, 8.0, 1.0, 0.0])
    assert c0.mean() == 3.2
    v = dict(R.CONF_VAD, vad_proportion_threshold=0.5)
    thr = 5.5 + 0.5 * 3.2
    assert R.vad_threshold(c0, v) == thr
    # ctx = 2: windows clipped at the ends: den = 3, 4, 5, ..., 5, 4, 3
    # t=0: {0,0,1} 1/3 no; t=1: {0,0,1,1} 2/4 yes; t=2: {0,0,1,1,0} 2/5 no; t=3: {0,1,1,0,0} no; t=4: {1,1,0,0,0} no;
    # t=5: {1,0,0,0,1} no; t=6: {0,0,0,1,0} no; t=7: {0,0,1,0,0} no; t=8: {0,1,0,0} 1/4 no; t=9: {1,0,0} 1/3 no
    hand = [0, 1, 0, 0, 0, 0, 0, 0, 0, 0]
    got = R.vad(np.stack([c0, np.zeros(10)], axis=1), v)
    assert list(got) == hand
    # the reference's proportion 0.12: any above-threshold frame within 2 frames makes a frame voiced
    got = R.vad(np.stack([c0, np.zeros(10)], axis=1), R.CONF_VAD)
    assert list(got) == [1, 1, 1, 1, 1, 1, 1, 1, 1, 1]
    c1 = np.array([9.0, 0, 0, 0, 0, 0, 0, 0, 0, 0])    # thr = 5.95: only frame 0 above -> frames 0..2 voiced
    assert list(R.vad(c1[:, None], R.CONF_VAD)) == [1, 1, 1, 0, 0, 0, 0, 0, 0, 0]
    assert list(R.vad(np.array([[3.0]]), R.CONF_VAD)) == [0]       # one frame: thr = 7 > 3
    assert list(R.vad(np.array([[20.0]]), R.CONF_VAD)) == [1]      # thr = 15.5 < 20
