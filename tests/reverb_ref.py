"""CPU restatement of wav-reverberate for one output channel (csrc/reverb.h lists the six points), twice:

ref64  reverberate(..., dtype=np.float64): direct convolution (np.convolve) in fp64; for the long cases, where that takes
       minutes, one whole-signal fp64 FFT (conv_fft64), which tests/test_reverb_ref.py shows to agree with the direct form.
ref32  reverberate(..., dtype=np.float32): the block-FFT formulation of the upstream tool (overlap-add, FFT size the power of
       two at or above four filter lengths) with every intermediate - spectra, products, power sums, scale factors -
       rounded to fp32: what a float build gives.
ref32p reverberate(..., dtype=np.float32, partitioned=True): the kernels' own formulation in fp32 (conv_partitioned32):
       uniformly partitioned overlap-save with 4096-point transforms, whose error - unlike ref32's, which transforms at
       least four filter lengths at once - says something about a scheme of short transforms (tests/test_gpu_reverb_edges.py).

Semantics are upstream Kaldi's as recalled (featbin/wav-reverberate.cc, feat/signal.cc); parity with Kaldi itself is unpinned.
Also the generators of the test signals (speech-like bursts over a noise floor, decaying impulse responses)."""
import numpy as np

DIRECT_LIMIT = 2.0e9        # multiply-adds up to which ref64 convolves directly


def early_slice(rir, rate):
    """(peak, e0, e1): first maximum of the signed values; the slice [peak - 0.001 rate, peak + 0.05 rate) inside the RIR."""
    peak = int(np.argmax(rir))
    e0 = max(0, peak - int(0.001 * rate))
    e1 = min(len(rir), peak + int(0.05 * rate))
    if e1 <= e0:
        e1 = e0 + 1
    return peak, e0, e1


def conv_direct64(x, h):
    return np.convolve(np.asarray(x, np.float64), np.asarray(h, np.float64))


def conv_fft64(x, h):
    n = len(x) + len(h) - 1
    size = 1 << int(np.ceil(np.log2(max(2, n))))
    return np.fft.irfft(np.fft.rfft(np.asarray(x, np.float64), size) * np.fft.rfft(np.asarray(h, np.float64), size), size)[:n]


def conv64(x, h):
    return conv_direct64(x, h) if float(len(x)) * len(h) <= DIRECT_LIMIT else conv_fft64(x, h)


def conv_block32(x, h):
    """Overlap-add block convolution, everything complex64 / float32."""
    x = np.asarray(x, np.float32)
    h = np.asarray(h, np.float32)
    n, L = len(x), len(h)
    fft_len = 1
    while fft_len < 4 * L:
        fft_len *= 2
    block = fft_len - L + 1
    nb = (n + block - 1) // block
    H = np.fft.rfft(h, fft_len)
    assert H.dtype == np.complex64, "this numpy computes float32 FFTs in double"
    padded = np.zeros(nb * block, np.float32)
    padded[:n] = x
    out = np.zeros(nb * block + L - 1, np.float32)
    step = max(1, (1 << 22) // fft_len)          # blocks per pass (bounds the memory of the long cases)
    for b0 in range(0, nb, step):
        b1 = min(nb, b0 + step)
        seg = padded[b0 * block:b1 * block].reshape(b1 - b0, block)
        Y = np.fft.rfft(seg, fft_len, axis=1)
        Y *= H[None, :]
        y = np.fft.irfft(Y, fft_len, axis=1)
        assert y.dtype == np.float32
        out[b0 * block:b1 * block] += y[:, :block].reshape(-1)      # each sample receives one head ...
        if L > 1:
            for i in range(b0, b1):                                   # ... and at most one tail (L - 1 < block)
                out[(i + 1) * block:(i + 1) * block + L - 1] += y[i - b0, block:block + L - 1]
    return out[:n + L - 1]


PART_N = 4096               # transform size of conv_partitioned32; hop and partition are half of it
PART_LOG2N = 12


def _twiddles32():
    j = np.arange(PART_N // 2)
    a = 2.0 * np.pi * j / PART_N
    return np.cos(a).astype(np.float32), (-np.sin(a)).astype(np.float32)      # rounded from double, as csrc/reverb.cc builds them


_BITREV = np.array([int(format(i, "0%db" % PART_LOG2N)[::-1], 2) for i in range(PART_N)])


def fft4096_32(re, im):
    """Forward transform of the rows of (re, im), float32 planes of 4096 columns: radix-2, decimation in time, every product
    and sum rounded to float32.  Returns new planes."""
    re = np.ascontiguousarray(np.asarray(re, np.float32)[:, _BITREV])
    im = np.ascontiguousarray(np.asarray(im, np.float32)[:, _BITREV])
    wr_all, wi_all = _twiddles32()
    rows = re.shape[0]
    for s in range(PART_LOG2N):
        half = 1 << s
        wr = wr_all[::PART_N // 2 >> s][:half]
        wi = wi_all[::PART_N // 2 >> s][:half]
        r = re.reshape(rows, -1, 2, half)
        i = im.reshape(rows, -1, 2, half)
        xr, xi = r[:, :, 1, :], i[:, :, 1, :]
        tr = wr * xr - wi * xi
        ti = wr * xi + wi * xr
        ur, ui = r[:, :, 0, :].copy(), i[:, :, 0, :].copy()
        r[:, :, 0, :] = ur + tr
        i[:, :, 0, :] = ui + ti
        r[:, :, 1, :] = ur - tr
        i[:, :, 1, :] = ui - ti
        assert tr.dtype == np.float32
    return re, im


def conv_partitioned32(x, h):
    """The kernels' formulation (csrc/reverb_kernels.h) in fp32: block b is the spectrum of x[(b - 1) H, (b + 1) H), output
    block b the second half of the inverse transform of the sum over min(P, b + 1) partitions p of X[b - p] H[p]."""
    x = np.asarray(x, np.float32)
    h = np.asarray(h, np.float32)
    n, L = len(x), len(h)
    N, H = PART_N, PART_N // 2
    ext = n + L - 1
    nb = (ext + H - 1) // H
    P = (L + H - 1) // H
    xp = np.zeros((nb + 1) * H, np.float32)
    xp[H:H + n] = x                                    # xp[H + s] = x[s]: block b starts at xp[b H]
    xb = np.stack([xp[b * H:b * H + N] for b in range(nb)])
    hp = np.zeros((P, N), np.float32)
    for p in range(P):
        seg = h[p * H:(p + 1) * H]
        hp[p, :len(seg)] = seg
    Xr, Xi = fft4096_32(xb, np.zeros_like(xb))
    Hr, Hi = fft4096_32(hp, np.zeros_like(hp))
    ar = np.zeros((nb, N), np.float32)
    ai = np.zeros((nb, N), np.float32)
    for p in range(P):                                 # block b takes partition p when b >= p
        xr, xi = Xr[:nb - p], Xi[:nb - p]
        ar[p:] += xr * Hr[p] - xi * Hi[p]
        ai[p:] += xr * Hi[p] + xi * Hr[p]
    yr, _ = fft4096_32(ar, -ai)                        # the inverse: conj(FFT(conj Z)) / N
    y = yr[:, H:] * np.float32(1.0 / N)
    assert y.dtype == np.float32
    return y.reshape(-1)[:ext]


def power(x, dtype):
    x = np.asarray(x, dtype)
    return dtype(np.dot(x, x)) / dtype(len(x))


def output_length(n, rir_len, rate, shift_output=True, duration=0.0):
    if duration > 0:
        return int(float(np.float32(rate)) * float(np.float32(duration)))
    if shift_output or rir_len <= 0:
        return n
    return n + rir_len - 1


def reverberate(x, rate, rir=None, additive=(), shift_output=True, normalize_output=True, duration=0.0, volume=0.0,
                dtype=np.float64, partitioned=False, early_taps=None):
    """x: samples in the 16-bit range; rir: as read from its file (scaled by 1/32768 here); additive: (noise, snr dB, start s).
    Returns the output before quantisation, in dtype.  partitioned: the fp32 leg convolves as the kernels do (ref32p).
    early_taps: another slice (e0, e1) than early_slice's, for tests that ask what a wrong slice would change."""
    conv = conv64 if dtype == np.float64 else conv_partitioned32 if partitioned else conv_block32
    x = np.asarray(x, dtype)
    n = len(x)
    power_before = power(x, dtype)
    sig = x.copy()
    shift = 0
    early = power_before
    rir_len = 0
    if rir is not None:
        h = np.asarray(rir, dtype) * dtype(1.0 / 32768.0)
        rir_len = len(h)
        peak, e0, e1 = early_slice(h, rate)
        if early_taps is not None:
            e0, e1 = early_taps
        ext = n + rir_len - 1
        xe = np.concatenate([x, np.zeros(rir_len - 1, dtype)])
        y_early = np.asarray(conv(xe, h[e0:e1])[:ext], dtype)
        early = dtype(np.dot(y_early, y_early)) / dtype(ext)
        sig = np.asarray(conv(x, h), dtype)
        assert len(sig) == ext
        shift = peak if shift_output else 0
    for noise, snr, start in additive:
        nz = np.asarray(noise, dtype)
        npow = power(nz, dtype)
        scale = dtype(np.sqrt(dtype(10.0 ** (-float(np.float32(snr)) / 10.0)) * early / npow))
        off = int(float(np.float32(start)) * float(np.float32(rate)))
        if off < len(sig):
            m = min(len(nz), len(sig) - off)
            sig[off:off + m] += (nz[:m] * scale).astype(dtype)
    power_after = power(sig, dtype)
    if volume > 0:
        sig = sig * dtype(np.float32(volume))
    elif normalize_output:
        sig = sig * dtype(np.sqrt(power_before / power_after))
    out_len = output_length(n, rir_len, rate, shift_output, duration)
    if out_len <= n:
        return np.asarray(sig[shift:shift + out_len], dtype)
    reps = out_len // len(sig) + 1
    return np.asarray(np.tile(sig, reps)[:out_len], dtype)


def quantize(y):
    """(int16 samples, clipped count): truncated toward zero, saturated - what the wave writer does.  NaN gives 0 and is
    not counted as clipped (rv_finish_kernel); the infinities saturate and are counted."""
    y = np.asarray(y, np.float64)
    t = np.trunc(np.where(np.isnan(y), 0.0, y))
    clipped = int(((t > 32767) | (t < -32768)).sum())
    return np.clip(t, -32768, 32767).astype(np.int16), clipped


# ---------------------------------------------------------------------------------------------- test signals
def speechlike(seed, n, rate=8000.0):
    """int16 signal: bursts of band-limited noise plus tones over a noise floor (never a stretch of exact zeros)."""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / rate
    x = rng.standard_normal(n) * 30.0
    pos = 0
    while pos < n:
        burst = int(rng.integers(int(0.05 * rate), int(0.6 * rate)))
        pause = int(rng.integers(int(0.02 * rate), int(0.4 * rate)))
        end = min(n, pos + burst)
        m = end - pos
        if m > 8:
            k = int(rng.integers(2, 12))
            noise = np.convolve(rng.standard_normal(m), np.ones(k) / k, mode="same")
            f1 = rng.uniform(100, 0.2 * rate)
            seg = 3000.0 * noise + 2500.0 * np.sin(2 * np.pi * f1 * t[pos:end])
            x[pos:end] += seg * np.hanning(m) * rng.uniform(0.3, 1.5)
        pos = end + pause
    return np.clip(np.round(x), -32768, 32767).astype(np.int16)


def flat_rir(seed, length, peak):
    """int16 impulse response without decay: every partition carries the same energy, the maximum stands at `peak`."""
    rng = np.random.default_rng(seed)
    h = np.clip(np.round(rng.standard_normal(length) * 3000.0), -12000, 12000)
    h[peak] = 20000.0
    return h.astype(np.int16)


def decaying_rir(seed, length, rate=8000.0, t60=0.4):
    """int16 impulse response: a direct path at a small delay, then exponentially decaying noise."""
    rng = np.random.default_rng(seed)
    i = np.arange(length)
    h = rng.standard_normal(length) * 4000.0 * np.exp(-6.9 * i / (t60 * rate))
    peak = min(length - 1, 20)
    h[:peak] *= 0.05
    h[peak] = 20000.0
    return np.clip(np.round(h), -32768, 32767).astype(np.int16)
