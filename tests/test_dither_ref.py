"""CPU checks of tests/dither_ref.py, the restatement of the MFCC kernel's dither generator that tests/test_gpu_mfcc_options.py
holds the kernel to: its key hash against the library's host function, the moments of its draws, and its use as the `noise`
of tests/mfcc_ref.py."""
import numpy as np

import dither_ref as D
import helpers as H
import mfcc_ref as R

KEYS = ["", "a", "utt1", "spkA-utt1", "spk2-pipe", "sw02001-A_000098-001156", "k" * 300, "été-1"]


def test_key_hash_is_the_librarys():
    P = H.pkg()
    assert D.fnv1a("") == 0xcbf29ce484222325                   # the offset basis
    assert D.fnv1a("a") == 0xaf63dc4c8601ec8c                  # FNV-1a's published test vector
    for k in KEYS:
        assert D.fnv1a(k) == P.utt_seed(k), k
    assert len({D.fnv1a(k) for k in KEYS}) == len(KEYS)


def test_mix64_and_the_uniforms():
    # fmix64 is a bijection with fixed point 0; its first values, worked by hand with Python integers
    def fmix(x):
        m = (1 << 64) - 1
        x ^= x >> 33
        x = (x * 0xff51afd7ed558ccd) & m
        x ^= x >> 33
        x = (x * 0xc4ceb9fe1a85ec53) & m
        return x ^ (x >> 33)
    xs = [0, 1, 2, 0x9e3779b97f4a7c15, (1 << 64) - 1, 1 << 63]
    assert [int(v) for v in D.mix64(np.array(xs, np.uint64))] == [fmix(x) for x in xs]
    assert fmix(0) == 0
    # one counter by hand: frame 3, sample 5 of key "utt1"
    g, m = 0x9e3779b97f4a7c15, (1 << 64) - 1
    r = fmix((fmix(D.fnv1a("utt1") ^ g) + ((3 << 32) | 5) * g) & m)
    u1, u2 = D.uniforms("utt1", 4, 6)
    assert u1[3, 5] == ((r >> 40) + 1) / 2.0 ** 24 and u2[3, 5] == ((r >> 8) & 0xffffff) / 2.0 ** 24
    u1, u2 = D.uniforms("range", 300, 400)
    assert u1.min() > 0 and u1.max() <= 1 and u2.min() >= 0 and u2.max() < 1
    assert (u1.astype(np.float32) == u1).all() and (u2.astype(np.float32) == u2).all()    # exact in fp32


def _lag1(z, axis):
    a = np.take(z, range(z.shape[axis] - 1), axis)
    b = np.take(z, range(1, z.shape[axis]), axis)
    return float((a * b).mean()), a.size


def test_draws_are_standard_normal_and_uncorrelated():
    """For N iid N(0,1) draws the sample mean has standard error 1/sqrt(N), the mean of z^2 sqrt(2/N) (var z^2 = 2), and
    the mean of z_i z_j over M independent pairs 1/sqrt(M) (var of a product of two independent N(0,1) = 1)."""
    for key, F, L in (("spkA-utt1", 1500, 200), ("", 700, 400), ("zero", 64, 4096)):
        z = D.draws(key, F, L)
        assert z.shape == (F, L) and z.dtype == np.float64 and np.isfinite(z).all()
        N = z.size
        mean, var = float(z.mean()), float((z * z).mean())
        across_samples, m1 = _lag1(z, 1)
        across_frames, m2 = _lag1(z, 0)
        print("draws %r [%d, %d]: mean %.5f (se %.5f)  E z^2 %.5f (se %.5f)  lag-1 over samples %.5f (se %.5f)  over frames %.5f (se %.5f)"
              % (key, F, L, mean, N ** -0.5, var, (2.0 / N) ** 0.5, across_samples, m1 ** -0.5, across_frames, m2 ** -0.5))
        assert abs(mean) < 6 * N ** -0.5
        assert abs(var - 1.0) < 6 * (2.0 / N) ** 0.5
        assert abs(across_samples) < 6 * m1 ** -0.5
        assert abs(across_frames) < 6 * m2 ** -0.5
        # per row and per column too: a generator that is right only on average over the matrix would show here
        assert np.abs(z.mean(axis=1)).max() < 6 * L ** -0.5 and np.abs(z.mean(axis=0)).max() < 6 * F ** -0.5
    a, b = D.draws("spkA-utt1", 5, 7), D.draws("spkA-utt2", 5, 7)
    assert (a != b).all()                                       # the key is part of the draw
    assert (D.draws("spkA-utt1", 9, 11)[:5, :7] == a).all()     # a draw depends on (key, frame, sample) alone
    assert (a.T != D.draws("spkA-utt1", 7, 5)).any()            # and not symmetrically on frame and sample


def test_draws_feed_the_mfcc_restatement():
    rng = np.random.default_rng(3)
    x = np.round(rng.standard_normal(3000) * 800).astype(np.int16)
    for conf in (R.CONF_MFCC, R.CONF_MFCC_SNIP_EDGE):
        o = R.options(**conf, dither=1.0)
        L, _, _ = R.geometry(o)
        F = R.num_frames(len(x), o)
        noise = D.draws("utt", F, L)
        plain = R.mfcc(x, R.options(**conf, dither=0.0), np.float64)
        for dtype in (np.float64, np.float32):
            got = R.mfcc(x, o, dtype, noise=noise)
            assert got.dtype == dtype and got.shape == (F, o["num_ceps"]) and np.isfinite(got).all()
            # dither 1 on a signal of size 800 moves the features a little, and does move them
            d = np.abs(got - plain).max()
            assert 0 < d < 1.0, d
        # the all-zero waveform: the frame energy is the draws' own
        z = R.mfcc(np.zeros(len(x), np.int16), o, np.float64, noise=noise)
        w = noise - noise.mean(axis=1, keepdims=True)
        assert np.allclose(z[:, 0], np.log((w * w).sum(axis=1)), rtol=0, atol=1e-12)
