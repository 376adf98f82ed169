"""numpy restatement of Kaldi's MFCC (compute-mfcc-feats) and energy VAD (compute-vad), written for the tests
[UPSTREAM semantics, recalled: feat/feature-window.cc, feat/mel-computations.cc, feat/feature-mfcc.cc,
ivector/voice-activity-detection.cc]; parity with Kaldi itself is unpinned, as everywhere in this tree.

Every function takes a `dtype`.  float64 is the truth.  float32 runs the same formulas with every intermediate - the
tables included - rounded to fp32, through its own radix-2 FFT (np.fft may compute in double): it stands for what a
float build such as Kaldi's gives, and its distance from float64 is the yardstick the GPU kernel is held to.

Options are a dict named like the command-line options with underscores; options(**kw) fills in Kaldi's defaults."""
import numpy as np

DEFAULTS = dict(sample_frequency=16000.0, frame_length=25.0, frame_shift=10.0, dither=1.0, preemphasis_coefficient=0.97,
                remove_dc_offset=True, window_type="povey", blackman_coeff=0.42, round_to_power_of_two=True, snip_edges=True,
                num_mel_bins=23, low_freq=20.0, high_freq=0.0, num_ceps=13, cepstral_lifter=22.0, use_energy=True,
                raw_energy=True, energy_floor=0.0)
VAD_DEFAULTS = dict(vad_energy_threshold=5.0, vad_energy_mean_scale=0.5, vad_frames_context=0, vad_proportion_threshold=0.6)

# the reference's conf/mfcc.conf (egs/sre/v2), v3's conf/mfcc_snip_edge.conf and conf/vad.conf, restated
CONF_MFCC = dict(sample_frequency=8000.0, frame_length=25.0, low_freq=20.0, high_freq=3700.0, num_ceps=23, snip_edges=False)
CONF_MFCC_SNIP_EDGE = dict(sample_frequency=8000.0, frame_length=25.0, low_freq=20.0, high_freq=3700.0, num_ceps=23)
CONF_VAD = dict(vad_energy_threshold=5.5, vad_energy_mean_scale=0.5, vad_proportion_threshold=0.12, vad_frames_context=2)


def options(**kw):
    o = dict(DEFAULTS)
    for k, v in kw.items():
        if k not in o:
            raise KeyError(k)
        o[k] = v
    return o


def geometry(o):
    """(L, S, P): window length, shift in samples, FFT size."""
    L = int(o["sample_frequency"] * 0.001 * o["frame_length"])
    S = int(o["sample_frequency"] * 0.001 * o["frame_shift"])
    P = 1
    while P < L:
        P *= 2
    return L, S, P


def num_frames(n, o):
    L, S, _ = geometry(o)
    if o["snip_edges"]:
        return 0 if n < L else 1 + (n - L) // S
    return (n + S // 2) // S


def first_sample(t, o):
    L, S, _ = geometry(o)
    return t * S if o["snip_edges"] else t * S + S // 2 - L // 2


def frame_indices(n, o):
    """[F, L] indices into the waveform, reflected at the ends without snip-edges."""
    L, _, _ = geometry(o)
    F = num_frames(n, o)
    idx = np.array([first_sample(t, o) for t in range(F)], dtype=np.int64).reshape(F, 1) + np.arange(L, dtype=np.int64)
    if not o["snip_edges"]:
        while True:
            bad = (idx < 0) | (idx >= n)
            if not bad.any():
                break
            idx = np.where(idx < 0, -idx - 1, idx)
            idx = np.where(idx >= n, 2 * n - 1 - idx, idx)
    return idx


def window(o, dtype=np.float64):
    L, _, _ = geometry(o)
    i = np.arange(L, dtype=dtype)
    a = dtype(2.0 * np.pi) / dtype(L - 1)
    kind = o["window_type"]
    if kind == "povey":
        return np.power(dtype(0.5) - dtype(0.5) * np.cos(a * i), dtype(0.85)).astype(dtype)
    if kind == "hamming":
        return (dtype(0.54) - dtype(0.46) * np.cos(a * i)).astype(dtype)
    if kind == "hanning":
        return (dtype(0.5) - dtype(0.5) * np.cos(a * i)).astype(dtype)
    if kind == "rectangular":
        return np.ones(L, dtype)
    if kind == "blackman":
        c = dtype(o["blackman_coeff"])
        return (c - dtype(0.5) * np.cos(a * i) + (dtype(0.5) - c) * np.cos(dtype(2) * a * i)).astype(dtype)
    raise ValueError(kind)


def mel_scale(f, dtype=np.float64):
    return (dtype(1127.0) * np.log(dtype(1.0) + np.asarray(f, dtype) / dtype(700.0))).astype(dtype)


def mel_bank(o, dtype=np.float64):
    """Dense [num_mel_bins, P/2 + 1] triangular filters (FFT bins 0 .. P/2 - 1 can carry weight; the Nyquist bin never does)."""
    _, _, P = geometry(o)
    sf = dtype(o["sample_frequency"])
    nyq = dtype(0.5) * sf
    low = dtype(o["low_freq"])
    high = dtype(o["high_freq"]) if o["high_freq"] > 0 else nyq + dtype(o["high_freq"])
    nb = o["num_mel_bins"]
    mel_low, mel_high = mel_scale(low, dtype), mel_scale(high, dtype)
    delta = (mel_high - mel_low) / dtype(nb + 1)
    mel = mel_scale(sf / dtype(P) * np.arange(P // 2, dtype=dtype), dtype)
    bank = np.zeros((nb, P // 2 + 1), dtype)
    for b in range(nb):
        left = mel_low + dtype(b) * delta
        center = left + delta
        right = center + delta
        inside = (mel > left) & (mel < right)
        up = (mel - left) / (center - left)
        down = (right - mel) / (right - center)
        bank[b, :P // 2] = np.where(inside, np.where(mel <= center, up, down), dtype(0)).astype(dtype)
    return bank


def dct_matrix(o, dtype=np.float64):
    """First num_ceps rows of the orthonormal DCT-II over num_mel_bins points."""
    nb, nc = o["num_mel_bins"], o["num_ceps"]
    n = np.arange(nb, dtype=dtype)
    m = np.empty((nc, nb), dtype)
    m[0] = np.sqrt(dtype(1.0) / dtype(nb))
    for k in range(1, nc):
        m[k] = np.sqrt(dtype(2.0) / dtype(nb)) * np.cos(dtype(np.pi) / dtype(nb) * (n + dtype(0.5)) * dtype(k))
    return m.astype(dtype)


def lifter(o, dtype=np.float64):
    q = dtype(o["cepstral_lifter"])
    i = np.arange(o["num_ceps"], dtype=dtype)
    if q == 0:
        return np.ones(o["num_ceps"], dtype)
    return (dtype(1.0) + dtype(0.5) * q * np.sin(dtype(np.pi) * i / q)).astype(dtype)


def fft_radix2(re, im, dtype=np.float64):
    """Forward DFT along the last axis (a power of two), decimation in time, all arithmetic in dtype."""
    re = np.array(re, dtype)
    im = np.array(im, dtype)
    P = re.shape[-1]
    bits = P.bit_length() - 1
    assert 1 << bits == P
    rev = np.array([int(format(i, "0%db" % bits)[::-1], 2) if bits else 0 for i in range(P)])
    re, im = re[..., rev], im[..., rev]
    lead = re.shape[:-1]
    half = 1
    while half < P:
        ang = dtype(-2.0 * np.pi) * np.arange(half, dtype=dtype) / dtype(2 * half)
        wr, wi = np.cos(ang).astype(dtype), np.sin(ang).astype(dtype)
        r = re.reshape(lead + (P // (2 * half), 2, half))
        i = im.reshape(lead + (P // (2 * half), 2, half))
        ar, ai, br, bi = r[..., 0, :], i[..., 0, :], r[..., 1, :], i[..., 1, :]
        tr = (wr * br - wi * bi).astype(dtype)
        ti = (wr * bi + wi * br).astype(dtype)
        re = np.stack([ar + tr, ar - tr], axis=-2).astype(dtype).reshape(lead + (P,))
        im = np.stack([ai + ti, ai - ti], axis=-2).astype(dtype).reshape(lead + (P,))
        half *= 2
    return re, im


def windowed_frames(x, o, dtype=np.float64, noise=None):
    """Steps 1-6: ([F, L] windowed frames, [F] raw log-energies or None).  noise: [F, L] N(0,1) draws for the dither."""
    x = np.asarray(x, dtype)
    L, _, _ = geometry(o)
    eps = dtype(np.finfo(np.float32).eps)
    idx = frame_indices(len(x), o)
    w = x[idx] if idx.size else np.zeros((0, L), dtype)
    if o["dither"] != 0:
        if noise is None:
            raise ValueError("dither needs the noise draws")
        w = (w + dtype(o["dither"]) * np.asarray(noise, dtype)).astype(dtype)
    if o["remove_dc_offset"]:
        w = (w - (w.sum(axis=1, dtype=dtype) / dtype(L))[:, None]).astype(dtype)
    raw = None
    if o["raw_energy"]:
        raw = np.log(np.maximum((w * w).sum(axis=1, dtype=dtype), eps)).astype(dtype)
    c = dtype(o["preemphasis_coefficient"])
    if c != 0:
        prev = np.concatenate([w[:, :1], w[:, :-1]], axis=1)
        w = (w - c * prev).astype(dtype)
    w = (w * window(o, dtype)).astype(dtype)
    return w, raw


def mfcc(x, o, dtype=np.float64, noise=None):
    """[F, num_ceps] in dtype."""
    L, _, P = geometry(o)
    eps = dtype(np.finfo(np.float32).eps)
    w, raw = windowed_frames(x, o, dtype, noise)
    F = w.shape[0]
    if F == 0:
        return np.zeros((0, o["num_ceps"]), dtype)
    energy = raw if o["raw_energy"] else np.log(np.maximum((w * w).sum(axis=1, dtype=dtype), eps)).astype(dtype)
    if o["energy_floor"] > 0:
        energy = np.maximum(energy, np.log(dtype(o["energy_floor"]))).astype(dtype)
    pad = np.zeros((F, P), dtype)
    pad[:, :L] = w
    re, im = fft_radix2(pad, np.zeros_like(pad), dtype)
    power = (re * re + im * im).astype(dtype)[:, :P // 2 + 1]
    mel = (power @ mel_bank(o, dtype).T).astype(dtype)
    logmel = np.log(np.maximum(mel, eps)).astype(dtype)
    ceps = (logmel @ dct_matrix(o, dtype).T).astype(dtype)
    ceps = (ceps * lifter(o, dtype)).astype(dtype)
    if o["use_energy"]:
        ceps[:, 0] = energy
    return ceps


def silence_row(o, dtype=np.float64):
    """The MFCC row of digital silence with dither=0: every mel energy and the frame energy sit at the floor."""
    eps = dtype(np.finfo(np.float32).eps)
    logmel = np.full(o["num_mel_bins"], np.log(eps), dtype)
    row = (dct_matrix(o, dtype) @ logmel) * lifter(o, dtype)
    if o["use_energy"]:
        e = np.log(eps)
        if o["energy_floor"] > 0:
            e = max(e, np.log(dtype(o["energy_floor"])))
        row[0] = e
    return row.astype(dtype)


def vad_threshold(c0, v, dtype=np.float64):
    c0 = np.asarray(c0, dtype)
    thr = dtype(v["vad_energy_threshold"])
    if v["vad_energy_mean_scale"] != 0 and len(c0):
        thr = thr + dtype(v["vad_energy_mean_scale"]) * (c0.sum(dtype=dtype) / dtype(len(c0)))
    return dtype(thr)


def vad(feats, v, dtype=np.float64):
    """[T] of 1.0 / 0.0: Kaldi's ComputeVadEnergy on one utterance's features (column 0 = log energy)."""
    c0 = np.asarray(feats, dtype)[:, 0]
    T = len(c0)
    thr = vad_threshold(c0, v, dtype)
    ctx = int(v["vad_frames_context"])
    # frame t looks at frames lo .. hi: num of them are above the threshold (exact integer counts through a running sum)
    t = np.arange(T)
    lo, hi = np.maximum(0, t - ctx), np.minimum(T - 1, t + ctx)
    above = np.concatenate([[0], np.cumsum(c0 > thr)])
    num = above[hi + 1] - above[lo]
    den = hi - lo + 1
    return (num.astype(dtype) >= den.astype(dtype) * dtype(v["vad_proportion_threshold"])).astype(np.float32)
