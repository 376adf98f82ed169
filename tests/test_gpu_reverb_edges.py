"""GPU tests of the reverberation kernels at their own edges: the partitions of the FFT path, the early slice, the chunks of
the direct, power, mix and finish kernels, the saturation thresholds and the cap of the spectra groups.  The cases and
their references are tests/reverb_edges.py; tests/test_reverb_ref.py asserts on the CPU that each case can see the
mistake it is there for.  tests/test_gpu_reverb.py compares whole recordings; here every sample of a small case matters.

Everything goes through reverberate().  The utterances of a test that share a rate and an option set go into one ragged
call in shuffled order, beside a direct-path, an FFT-path and a RIR-less neighbour.

Where the kernels' arithmetic is exact (integer data: fp64 sums rounded once, products with powers of two) bytes are
compared.  The float bar of the FFT path, per utterance:
    max|gpu - ref64| <= max(4 max(e32, e32p), 2^-22 max|ref64|)
e32 = max|ref32 - ref64| and e32p = max|ref32p - ref64| over the same samples; ref32p is the kernels' own formulation in
fp32 (reverb_ref.conv_partitioned32), so the factor 4 covers exactly another FFT factorisation and other summation orders;
the floor is four fp32 units in the last place of the utterance's peak.  Figures: profiles/reverb_edges.md."""
import numpy as np
import pytest

import helpers as H
import reverb_edges as E
import reverb_ref as R

pytestmark = pytest.mark.gpu


def _neighbours(dtype):
    return [E.Case("direct-path neighbour", R.speechlike(9001, 500).astype(dtype), R.decaying_rir(9002, 40).astype(np.float32), ()),
            E.Case("FFT-path neighbour", R.speechlike(9003, 3000).astype(dtype), R.flat_rir(9004, E.H + 52, 20).astype(np.float32), ()),
            E.Case("RIR-less neighbour", R.speechlike(9005, 700).astype(dtype), None,
                   ((R.speechlike(9006, 900).astype(np.float32), 5.0, 0.01),))]


def _call(cases, rate, seed, **opts):
    """One ragged call of the cases, shuffled, beside the neighbours; the outputs in the order of `cases`."""
    P = H.pkg()
    every = list(cases) + _neighbours(cases[0].x.dtype)
    order = np.random.default_rng(seed).permutation(len(every))
    assert len({c.x.dtype for c in every}) == 1
    got = P.reverberate([every[i].x for i in order], rirs=[every[i].rir for i in order],
                        additive=[list(every[i].additive) for i in order], rate=rate, **opts)
    out = [None] * len(every)
    for pos, i in enumerate(order):
        out[i] = got[pos]
    return out[:len(cases)]


def _same_bytes(got, want, name):
    assert got.dtype == want.dtype == np.float32 and got.shape == want.shape, (name, got.shape, want.shape)
    assert got.tobytes() == want.tobytes(), (name, np.flatnonzero(got != want)[:8])


# ------------------------------------------------------------------------------------------ 1. direct path, bit for bit
@pytest.mark.parametrize("shift", [False, True])
def test_direct_path_is_the_fp64_sum_rounded_once(shift):
    cases = E.section1_cases()
    as_i16 = _call(cases, 8000.0, 11, shift_output=shift, volume=1.0)
    as_f32 = _call([c._replace(x=c.x.astype(np.float32)) for c in cases], 8000.0, 12, shift_output=shift, volume=1.0)
    for c, a, b in zip(cases, as_i16, as_f32):
        _same_bytes(a, E.direct_expect(c, shift), c.name)
        _same_bytes(b, a, c.name + " as float32")


# ---------------------------------------------------------------------- 2. direct path, early energy against the reference
@pytest.mark.parametrize("rate", [8000.0, 400.0])
def test_direct_path_early_energy_scales_the_noise(rate):
    cases = E.section2_cases(rate)
    got = _call(cases, rate, 21, **E.SECTION2_OPTS)
    bad = []
    for idx, (c, g) in enumerate(zip(cases, got)):
        r64, bar = E.section2_ref(rate, idx)
        assert g.shape == r64.shape, c.name
        over = np.abs(g.astype(np.float64) - r64) / np.maximum(bar, 1e-300)
        print("early, direct: %s  worst error / bar %.3f" % (c.name, over.max()))
        if not (np.abs(g.astype(np.float64) - r64) <= bar).all():
            bad.append((c.name, float(over.max()), float((over > 1).mean())))
    assert not bad, bad


# ------------------------------------------------------------------------------------------------ 3 and 4. the FFT path
def _float_bar(what, cases, got, ref):
    bad = []
    for idx, (c, g) in enumerate(zip(cases, got)):
        r64, e32, e32p, bar = ref(idx)
        assert g.dtype == np.float32 and g.shape == r64.shape and np.isfinite(g).all(), c.name
        err = float(np.abs(g.astype(np.float64) - r64).max())
        print("| %s, %s | %d | %.3e | %.3e | %.3e | %.3e | %.3f |" % (what, c.name, g.size, err, e32, e32p, bar, err / bar))
        if not err <= bar:
            bad.append((c.name, err, bar))
    assert not bad, bad


@pytest.mark.parametrize("shift", [False, True])
def test_fft_path_at_every_partition_and_block_edge(shift):
    cases = E.section3_cases()
    got = _call(cases, 8000.0, 31, shift_output=shift, volume=1.0)
    _float_bar("shift_output=%s" % str(shift).lower(), cases, got, lambda idx: E.section3_ref(idx, shift))


@pytest.mark.parametrize("rate", E.SECTION4_RATES)
def test_fft_path_early_slice_across_partitions(rate):
    cases = E.section4_cases(rate)
    got = _call(cases, rate, 41, **E.SECTION4_OPTS)
    _float_bar("early slice", cases, got, lambda idx: E.section4_ref(rate, idx))


# ------------------------------------------------------------------------------------ 5. mix and power kernels, bit for bit
def test_mix_kernel_adds_every_sample_of_every_noise():
    cases = E.section5_cases()
    got = _call(cases, E.RATE5, 51, volume=1.0)
    for idx, (c, g) in enumerate(zip(cases, got)):
        _same_bytes(g, E.section5_ref(idx, False).astype(np.float32), c.name)


def test_power_kernels_count_every_sample_of_every_chunk():
    cases = E.section5_cases()
    got = _call(cases, E.RATE5, 52)
    worst = 0.0
    for idx, (c, g) in enumerate(zip(cases, got)):
        r64 = E.section5_ref(idx, True)
        assert g.shape == r64.shape, c.name
        err = np.abs(g.astype(np.float64) - r64)
        worst = max(worst, float((err / np.maximum(np.abs(r64), 1e-300)).max()) / E.ULP4)
        assert (err <= E.ULP4 * np.abs(r64)).all(), (c.name, float((err / np.abs(r64).clip(1e-300)).max()))
    print("normalised mix: worst relative error / 2^-22 = %.3f" % worst)


# ---------------------------------------------------------------------- 6. finish kernel: thresholds, counts, trim, repeat
def _finish_call(utts, seed):
    P = H.pkg()
    order = np.random.default_rng(seed).permutation(len(utts)) if seed is not None else np.arange(len(utts))
    got = P.reverberate([utts[i][0] for i in order], rate=E.RATE5, volume=1.0, return_int16=True)
    for pos, i in enumerate(order):
        x, q, count = utts[i]
        f, q16, clipped = got[pos]
        nan = np.isnan(x)
        assert f.dtype == np.float32 and f.shape == x.shape and np.isnan(f[nan]).all(), i
        assert f[~nan].tobytes() == x[~nan].tobytes(), i
        planted = np.flatnonzero(x != E.BACKGROUND[0])
        assert q16.dtype == np.int16 and np.array_equal(q16, q), (i, [(int(p), float(x[p]), int(q16[p]), int(q[p])) for p in planted if q16[p] != q[p]])
        assert clipped == count, (i, clipped, count)


def test_finish_kernel_saturates_exactly_at_the_thresholds():
    _finish_call(E.threshold_rotations(), 61)


def test_finish_kernel_counts_each_utterances_clipped_samples():
    utts = E.count_utterances()
    assert [u[2] for u in utts] == [4, 0, 6, 1]
    _finish_call(utts, None)              # in this order: the one without sits between two that clip in several chunks


@pytest.mark.parametrize("shift", [False, True])
def test_finish_kernel_trims_shifts_and_repeats(shift):
    x = E.int_signal(6100, E.TRIM_N)
    for out_len in E.trim_out_lens():
        got = _call([E.Case("out_len %d" % out_len, x, E.trim_rir(), ())], E.RATE5, 62 + out_len, shift_output=shift,
                    duration=out_len / E.RATE5, volume=1.0)[0]
        _same_bytes(got, E.trim_expect(x, E.trim_rir(), shift, out_len), "n %d, out_len %d" % (E.TRIM_N, out_len))


def test_finish_kernel_reads_across_the_chunk_edge():
    P = H.pkg()
    one = np.array([7], np.int16)                      # one sample, no RIR, repeated: wraps at every sample
    got = P.reverberate([one], rate=E.RATE5, duration=(E.C + 1) / E.RATE5, volume=1.0)[0]
    _same_bytes(got, np.full(E.C + 1, 7, np.float32), "n 1 repeated")
    x = E.int_signal(6200, E.C + 1)
    for shift in (False, True):                        # the shifted read s = o + 20 crosses the edge before o does
        got = _call([E.Case("chunk edge", x, E.trim_rir(), ())], E.RATE5, 63, shift_output=shift, duration=E.C / E.RATE5, volume=1.0)[0]
        _same_bytes(got, E.trim_expect(x, E.trim_rir(), shift, E.C), "n C + 1, out_len C, shift %d" % shift)


# ------------------------------------------------------------------------------------ 7. spectra groups at the cap's edge
def test_spectra_groups_at_the_edge_of_the_cap(monkeypatch):
    P = H.pkg()
    rir_list = [R.flat_rir(7000, E.H + 1, 20).astype(np.float32), E.trim_rir(), R.flat_rir(7001, E.DMAX + 1, 3).astype(np.float32),
                R.flat_rir(7002, 2 * E.H + 9, E.H + 5).astype(np.float32)]
    rirs = [0, 1, None, 2, 3, 0]                       # FFT path, 64-tap direct, none, FFT path, FFT path, the first one's again
    lens = (E.H + 700, 900, 1500, E.H, 2 * E.H, 1)
    waves = [R.speechlike(7100 + i, n) for i, n in enumerate(lens)]
    blocks = [-(-(n + len(rir_list[r]) - 1) // E.H) if r is not None and len(rir_list[r]) > E.DMAX else 0 for n, r in zip(lens, rirs)]
    assert blocks == [3, 0, 0, 2, 5, 2] and max(blocks) <= 5
    two = blocks[0] + blocks[3]
    whole = P.reverberate(waves, rirs=rirs, rate=8000.0, rir_list=rir_list)
    for cap in (1, two - 1, two, two + 1):
        monkeypatch.setenv("XVEC_DEBUG", "reverb_group_blocks=%d" % cap)
        grouped = P.reverberate(waves, rirs=rirs, rate=8000.0, rir_list=rir_list)
        for u, (a, b) in enumerate(zip(whole, grouped)):
            assert a.tobytes() == b.tobytes(), (cap, u)
