"""The cases of tests/test_gpu_reverb_edges.py: small utterances that put the reverberation kernels at their partition, slice,
chunk and clip edges, with the references each is held against.  tests/test_reverb_ref.py asserts on the CPU what the
cases have to fulfil to mean anything (exact arithmetic where bytes are compared, and that the mistake a case is there
to catch moves the reference far beyond the case's bar); the GPU tests then only compare.

Every length is derived from the kernels' constants, read from csrc/reverb_kernels.h."""
import collections
import functools
import os
import re

import numpy as np

import helpers
import reverb_ref as R

_HDR = open(os.path.join(helpers.ROOT, helpers.PKG_NAME, "csrc", "reverb_kernels.h")).read()


def _const(name):
    return int(re.search(r"\b%s = (\d+);" % name, _HDR).group(1))


H = _const("kRvH")                  # hop and partition of the FFT path
DMAX = _const("kRvDirectMax")       # longest filter of the direct path
DC = _const("kRvDirectChunk")       # outputs per workgroup of the direct path
C = _const("kRvChunk")              # samples per workgroup and fp64 partial of the power, mix and finish kernels

Case = collections.namedtuple("Case", "name x rir additive")
ULP4 = 2.0 ** -22                   # four fp32 units in the last place, relative


def _frozen(a):
    a.setflags(write=False)
    return a


def int_signal(seed, n, dtype=np.int16):
    """Integers in [-8, 8], the first one not zero (an utterance of one sample has to carry energy)."""
    x = np.random.default_rng(seed).integers(-8, 9, n)
    if x[0] == 0:
        x[0] = 3
    return _frozen(x.astype(dtype))


def int_rir(seed, length, peaks=(), top=9):
    """Integer taps in [-8, 8], none of them zero (so that every tap of an early slice counts), `top` at `peaks`."""
    rng = np.random.default_rng(seed)
    h = rng.integers(1, 9, length) * rng.choice([-1, 1], length)
    for p in peaks:
        h[p] = top
    return _frozen(h.astype(np.float32))


def peak_of(rir):
    return int(np.argmax(rir))


# ------------------------------------------------------------------------------------------ 1. direct path, bit for bit
@functools.lru_cache(maxsize=None)
def direct_filters():
    out = [("L=%d" % L, int_rir(1000 + L, L)) for L in (1, 2, DMAX - 1)]
    out += [("L=%d peak %d" % (DMAX, p), int_rir(1100 + p, DMAX, (p,))) for p in (0, 20, DMAX - 1)]
    out.append(("L=%d tie 5, 40" % DMAX, int_rir(1200, DMAX, (5, 40))))
    neg = -np.random.default_rng(1300).integers(2, 9, DMAX)
    neg[[7, 33]] = -1
    out.append(("L=%d all negative" % DMAX, _frozen(neg.astype(np.float32))))
    return out


def direct_lengths(L):
    """n = 1, n = 2 and the n that put ext_len = n + L - 1 around one and two chunks of the direct kernel."""
    return [1, 2] + [e - L + 1 for e in (DC - 1, DC, DC + 1, 2 * DC + 1)]


@functools.lru_cache(maxsize=None)
def section1_cases():
    cases = []
    for i, (name, h) in enumerate(direct_filters()):
        for j, n in enumerate(direct_lengths(len(h))):
            cases.append(Case("%s, n=%d" % (name, n), int_signal(1400 + 10 * i + j, n), h, ()))
    return cases


def direct_expect(c, shift):
    full = R.conv_direct64(c.x, np.asarray(c.rir, np.float64) / 32768.0)
    y = full[peak_of(c.rir):peak_of(c.rir) + len(c.x)] if shift else full
    return y.astype(np.float32)


# ---------------------------------------------------------------------- 2. direct path, early energy against the reference
SECTION2_PEAKS = {8000.0: (0, 20, DMAX - 1), 400.0: (0, 30, 50, DMAX - 1)}
SECTION2_SNRS = (0.0, 6.0)


@functools.lru_cache(maxsize=None)
def section2_cases(rate):
    cases = []
    for i, peak in enumerate(SECTION2_PEAKS[rate]):
        h = int_rir(2000 + int(rate) + i, DMAX, (peak,))
        for j, n in enumerate(direct_lengths(DMAX)):
            x = int_signal(2100 + 10 * i + j, n)
            noise = int_signal(2200 + 10 * i + j, n + DMAX - 1 + 7, np.float32)
            for snr in SECTION2_SNRS:
                cases.append(Case("rate %d, peak %d, n=%d, snr %g" % (rate, peak, n, snr), x, h, ((noise, snr, 0.0),)))
    return cases


SECTION2_OPTS = dict(shift_output=False, volume=1.0)


@functools.lru_cache(maxsize=None)
def section2_ref(rate, idx):
    """(ref64, bar per sample): the bar is 2^-22 (|convolved sample| + |scaled noise sample|)."""
    c = section2_cases(rate)[idx]
    r64 = R.reverberate(c.x, rate, rir=c.rir, additive=c.additive, **SECTION2_OPTS)
    conv = R.conv_direct64(c.x, np.asarray(c.rir, np.float64) / 32768.0)
    return _frozen(r64), _frozen(ULP4 * (np.abs(conv) + np.abs(r64 - conv)))


def slice_moves(rir, rate):
    """The slices one tap off the right one at either end, those that exist."""
    _, e0, e1 = R.early_slice(np.asarray(rir, np.float64), rate)
    return [(a, b) for a, b in ((e0 - 1, e1), (e0 + 1, e1), (e0, e1 - 1), (e0, e1 + 1)) if 0 <= a < b <= len(rir)]


# --------------------------------------------------------------------------- the float bar of the FFT path (3 and 4)
def _float_ref(c, rate, **kw):
    """(ref64, e32, e32p, bar) with bar = max(4 max(e32, e32p), 2^-22 max|ref64|)."""
    kw = dict(kw, rir=c.rir, additive=c.additive)
    r64 = R.reverberate(c.x, rate, dtype=np.float64, **kw)
    e32 = float(np.abs(R.reverberate(c.x, rate, dtype=np.float32, **kw) - r64).max())
    e32p = float(np.abs(R.reverberate(c.x, rate, dtype=np.float32, partitioned=True, **kw) - r64).max())
    return _frozen(r64), e32, e32p, max(4.0 * max(e32, e32p), ULP4 * float(np.abs(r64).max()))


# ---------------------------------------------------------------------------- 3. FFT path, every partition and block edge
@functools.lru_cache(maxsize=None)
def fft_filters():
    """(length, peak): one tap over the direct path, around one and two partitions, eight partitions and one tap more; a
    peak one block in (the shift is then exactly one block) and a peak at the last tap."""
    out = [(L, min(L - 1, 20)) for L in (DMAX + 1, H - 1, H, H + 1, 2 * H, 2 * H + 1, 8 * H, 8 * H + 1)]
    return out + [(2 * H + 1, H), (2 * H + 1, 2 * H)]


def partitions(L):
    return (L + H - 1) // H


def _speech(seed, n):
    """R.speechlike, re-seeded while it is digital silence (its noise floor rounds to 0 now and then at n = 1)."""
    while True:
        x = R.speechlike(seed, n)
        if np.abs(x).max() > 0:
            return _frozen(x)
        seed += 1000


def _flat(seed, L, peak):
    """R.flat_rir, re-seeded while its last tap is too small for its loss to show."""
    while True:
        h = R.flat_rir(seed, L, peak)
        if abs(int(h[-1])) >= 1000:
            return _frozen(h.astype(np.float32))
        seed += 1000


@functools.lru_cache(maxsize=None)
def section3_cases():
    cases = []
    for i, (L, peak) in enumerate(fft_filters()):
        h = _flat(3000 + i, L, peak)
        k = partitions(L) + 2
        for j, n in enumerate([1, 39] + [k * H + d - L + 1 for d in (-1, 0, 1)]):
            cases.append(Case("L=%d peak %d, n=%d" % (L, peak, n), _speech(3100 + 10 * i + j, n), h, ()))
    return cases


@functools.lru_cache(maxsize=None)
def section3_ref(idx, shift):
    return _float_ref(section3_cases()[idx], 8000.0, shift_output=shift, volume=1.0)


# --------------------------------------------------------------------------- 4. FFT path, the early slice across partitions
SECTION4_RATES = (8000.0, 40160.0, 40180.0, 48000.0)
SECTION4_L = 3 * H + 5
SECTION4_PEAKS = (0, 100, H - 1, H, H + 52, SECTION4_L - 1)
SECTION4_OPTS = dict(shift_output=False, volume=1.0)


@functools.lru_cache(maxsize=None)
def section4_cases(rate):
    n = 2 * H + 1
    cases = []
    for i, peak in enumerate(SECTION4_PEAKS):
        h = _frozen(R.flat_rir(4000 + i, SECTION4_L, peak).astype(np.float32))
        x = _frozen(R.speechlike(4100 + i, n))
        noise = _frozen(R.speechlike(4200 + i, n + SECTION4_L).astype(np.float32))
        cases.append(Case("rate %d, peak %d" % (rate, peak), x, h, ((noise, -10.0, 0.0),)))
    return cases


@functools.lru_cache(maxsize=None)
def section4_ref(rate, idx):
    return _float_ref(section4_cases(rate)[idx], rate, **SECTION4_OPTS)


def early_partitions(rir, rate):
    _, e0, e1 = R.early_slice(np.asarray(rir, np.float64), rate)
    return partitions(e1 - e0)


# ------------------------------------------------------------------------------------ 5. mix and power kernels, bit for bit
RATE5 = 8192.0                      # start = k / 8192 is exact in float32 and int(start * rate) = k


def sign3(n, amp, phase=0):
    """+-amp in a sign pattern of period 3: the power is amp^2 at every length."""
    return _frozen((amp * np.array([1, 1, -1])[(np.arange(n) + phase) % 3]))


def _add(m, start, amp):
    return (sign3(m, amp, start).astype(np.float32), 0.0, float(np.float32(start / RATE5)))


@functools.lru_cache(maxsize=None)
def section5_cases():
    cases = []
    for n in (C - 1, C, C + 1, 2 * C + 1):
        x = sign3(n, 4).astype(np.int16)
        lists = []
        for s in (0, 1, C - 1, C, C + 1, n - 1, n, n + 5):
            for m in (1, 2):
                lists.append(("noise of %d at %d" % (m, s), [_add(m, s, 2 if (s + m) % 2 else 1)]))
        lists.append(("ends at the last sample", [_add(37, n - 37, 2)]))
        lists.append(("ends one past the last sample", [_add(37, n - 36, 1)]))
        lists.append(("longer than the signal", [_add(n + 9, 0, 2)]))
        lists.append(("longer than the signal, from 3", [_add(n + 9, 3, 1)]))
        lists.append(("three on the same samples", [_add(50, C - 20, 2), _add(70, C - 30, 1), _add(90, C - 10, 2)]))
        for what, adds in lists:
            cases.append(Case("n=%d, %s" % (n, what), x, None, tuple(adds)))
    return cases


@functools.lru_cache(maxsize=None)
def section5_ref(idx, normalised):
    c = section5_cases()[idx]
    return _frozen(R.reverberate(c.x, RATE5, additive=c.additive, **({} if normalised else dict(volume=1.0))))


# ---------------------------------------------------------------------- 6. finish kernel: thresholds, counts, trim, repeat
def _f32(v):
    return np.float32(v)


# value, the 16-bit sample it becomes, whether it counts as clipped - written out by hand: clipped are exactly the values
# >= 32768.0 and <= -32769.0, the infinities among them; NaN gives 0 and is not clipped; everything else goes toward zero
THRESHOLDS = [
    (_f32(32767.0), 32767, False),
    (_f32(32767.5), 32767, False),
    (np.nextafter(_f32(32768.0), _f32(0.0)), 32767, False),
    (_f32(32768.0), 32767, True),
    (_f32(1e9), 32767, True),
    (_f32(np.inf), 32767, True),
    (_f32(-32768.0), -32768, False),
    (_f32(-32768.5), -32768, False),
    (np.nextafter(_f32(-32769.0), _f32(0.0)), -32768, False),
    (_f32(-32769.0), -32768, True),
    (_f32(-np.inf), -32768, True),
    (_f32(np.nan), 0, False),
    (_f32(-0.0), 0, False),
    (_f32(0.99), 0, False),
    (_f32(-0.99), 0, False),
    (_f32(1.5), 1, False),
    (_f32(-1.5), -1, False),
]
THRESHOLD_LEN = 2 * C + 3
THRESHOLD_POS = (0, C - 1, C, C + 1, THRESHOLD_LEN - 1)
BACKGROUND = (np.float32(100.25), 100)      # every other sample, and what it becomes


def planted(values_at):
    """(float32 utterance, its 16-bit samples, clipped count) with THRESHOLDS[k] at position p for (p, k) in values_at."""
    x = np.full(THRESHOLD_LEN, BACKGROUND[0], np.float32)
    q = np.full(THRESHOLD_LEN, BACKGROUND[1], np.int16)
    count = 0
    for p, k in values_at:
        x[p], q[p] = THRESHOLDS[k][0], THRESHOLDS[k][1]
        count += THRESHOLDS[k][2]
    return _frozen(x), _frozen(q), count


@functools.lru_cache(maxsize=None)
def threshold_rotations():
    """One utterance per rotation: together every value stands once at every position."""
    K = len(THRESHOLDS)
    return [planted([(p, (r + i) % K) for i, p in enumerate(THRESHOLD_POS)]) for r in range(K)]


@functools.lru_cache(maxsize=None)
def count_utterances():
    """Four utterances with different counts; the second has none and sits between two that clip in more than one chunk."""
    hi, lo, inf, big, nan, near = 3, 9, 5, 4, 11, 2          # indices into THRESHOLDS
    a = planted([(0, hi), (C - 1, lo), (C, inf), (2 * C + 2, big)])                     # chunks 0, 1 and 2
    b = planted([(0, near), (C - 1, nan), (C, 1), (C + 1, 7), (2 * C + 2, 8)])          # none
    c = planted([(5, hi), (C + 1, hi), (C + 2, lo), (2 * C, 10), (2 * C + 1, inf), (2 * C + 2, nan), (77, big)])
    d = planted([(C, lo)])
    return [a, b, c, d]


TRIM_N = 301                         # more than one pass of the workgroup's 256 threads


@functools.lru_cache(maxsize=None)
def trim_rir():
    return int_rir(6000, DMAX, (20,))


def trim_out_lens(n=TRIM_N):
    ext = n + DMAX - 1
    return (1, n - 1, n, n + 1, ext, ext + 1, 2 * ext + 3)


def trim_expect(x, rir, shift, out_len):
    y = R.reverberate(x, RATE5, rir=rir, shift_output=shift, duration=out_len / RATE5, volume=1.0)
    assert y.shape == (out_len,)
    return y.astype(np.float32)
