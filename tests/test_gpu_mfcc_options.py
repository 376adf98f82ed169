"""GPU sweep of the MFCC and energy-VAD kernels over their option space, dither included: what tests/test_gpu_mfcc.py leaves
at one value (window geometry and FFT size, pre-emphasis, DC removal, the shape of the mel bank and of the DCT, lifter, energy
floor), parity of the dithered features with tests/dither_ref.py's draws, the VAD at Kaldi's defaults, at the edges of its
options and on proportion ties, and the tool flags no other test passes.

The parity criterion is test_gpu_mfcc.py's, unchanged: max|gpu - ref64| <= 4 * max|ref32 - ref64| per option set over all
frames of the set.  A set is only a usable case if its yardstick max|ref32 - ref64| is at least 16 fp32 ulps of its largest
feature (asserted); all sets here were run on the CPU beforehand: yardsticks 6e-5 (lifter 0) to 3e-3 (80 bins), no mel energy
at the log floor.  profiles/mfcc_option_sweep.md holds the measured table and which of these tests notices which one-line
mutation of the kernel."""
import fractions
import functools
import os
import subprocess

import numpy as np
import pytest

import dither_ref as D
import helpers as H
import mfcc_ref as R
from oracle import kaldi_io as kio
from test_gpu_mfcc import BIN, parity_waves, speechlike, write_wav

pytestmark = pytest.mark.gpu

K8 = dict(sample_frequency=8000.0)          # Kaldi's defaults at 8 kHz: snip-edges, 13 ceps, the bank up to Nyquist
OPTION_SETS = {
    "fl20_fs5": dict(R.CONF_MFCC, frame_length=20.0, frame_shift=5.0),                          # L 160, S 40, P 256
    "fl32_8k_L_eq_P": dict(R.CONF_MFCC, frame_length=32.0),                                     # L = P = 256
    "fl10_fs15_P128": dict(K8, frame_length=10.0, frame_shift=15.0),                            # L 80 < S 120, P 128
    "fl10_fs15_P128_no_snip": dict(K8, frame_length=10.0, frame_shift=15.0, snip_edges=False),
    "16k_fl64_L_eq_P": dict(frame_length=64.0),                                                 # L = P = 1024
    "44k1_40bins_20ceps": dict(sample_frequency=44100.0, num_mel_bins=40, num_ceps=20),         # L 1102, S 441, P 2048
    "16k_fl200_P4096": dict(frame_length=200.0, frame_shift=50.0, snip_edges=False),            # L 3200, S 800, P 4096
    "preemph_0": dict(R.CONF_MFCC, preemphasis_coefficient=0.0),
    "preemph_1": dict(R.CONF_MFCC, preemphasis_coefficient=1.0),
    # the first samples of the window only count where the window does not vanish there
    "preemph_1_rectangular": dict(R.CONF_MFCC, preemphasis_coefficient=1.0, window_type="rectangular"),
    "preemph_05_hamming": dict(R.CONF_MFCC_SNIP_EDGE, preemphasis_coefficient=0.5, window_type="hamming"),
    "remove_dc_false": dict(R.CONF_MFCC, remove_dc_offset=False),
    "40bins_40ceps_to_nyquist": dict(K8, num_mel_bins=40, num_ceps=40, snip_edges=False),       # FFT bin P/2 - 1 carries weight
    "16k_80bins_70ceps": dict(num_mel_bins=80, num_ceps=70),                                    # second trip of both loops
    "lifter_0": dict(R.CONF_MFCC, cepstral_lifter=0.0),
    # num-ceps 1 without energy is no usable parity case (c0 alone: yardstick 2e-5 on values of 100, 3 ulps; 1.1e-4 with four
    # coefficients, still under 16 ulps); with 8 it is 2.6e-4, and test_few_ceps_are_the_first_columns_of_eight holds 1, 2 and
    # 3 coefficients to this set
    "ceps_8_no_energy": dict(R.CONF_MFCC, num_ceps=8, use_energy=False),
    "low100_high_minus300": dict(R.CONF_MFCC, low_freq=100.0, high_freq=-300.0),
    "blackman_03": dict(R.CONF_MFCC, window_type="blackman", blackman_coeff=0.3),
    "floor_1e6_raw": dict(R.CONF_MFCC, energy_floor=1e6, raw_energy=True),
    "floor_1e6_windowed": dict(R.CONF_MFCC_SNIP_EDGE, energy_floor=1e6, raw_energy=False),
}

_ROWS = {}


def _write_table():
    path = os.environ.get("XVEC_MFCC_SWEEP_MD")       # set by whoever refreshes the table of profiles/mfcc_option_sweep.md
    if not path or not _ROWS:
        return
    with open(path, "w") as f:
        f.write("| option set | L, S, P | frames | max abs(gpu - ref64) | max abs(ref32 - ref64) | bar (4 x) | inside |\n|---|---|---|---|---|---|---|\n")
        for name, (geo, fr, g, r) in _ROWS.items():
            f.write("| %s | %d, %d, %d | %d | %.3e | %.3e | %.3e | %s |\n" % ((name,) + geo + (fr, g, r, 4 * r, "yes" if g <= 4 * r else "NO")))


@functools.lru_cache(maxsize=2)
def _waves(rate, L, S):
    """parity_waves at this rate plus the lengths around one window and around the first frame without snip-edges."""
    extra = [n for n in (L - 1, L, L + 1, S // 2 - 1, S // 2) if n > 0]
    return parity_waves(rate) + [speechlike(200 + i, n, rate) for i, n in enumerate(extra)]


def _parity(name, kw, waves, got, noise=None):
    """Asserts shapes and the 4x bar over all these utterances; returns (frames, err_gpu, err_32, ref64 list)."""
    o = R.options(**kw)
    err_gpu = err_32 = top = 0.0
    frames = 0
    refs = []
    for i, (w, g) in enumerate(zip(waves, got)):
        nz = None if noise is None else noise[i]
        r64 = R.mfcc(w, o, np.float64, noise=nz)
        r32 = R.mfcc(w, o, np.float32, noise=nz)
        refs.append(r64)
        assert r32.dtype == np.float32 and g.dtype == np.float32
        assert g.shape == r64.shape == (R.num_frames(len(w), o), o["num_ceps"])
        frames += g.shape[0]
        if g.size:
            assert np.isfinite(g).all()
            err_gpu = max(err_gpu, float(np.abs(g.astype(np.float64) - r64).max()))
            err_32 = max(err_32, float(np.abs(r32.astype(np.float64) - r64).max()))
            top = max(top, float(np.abs(r64).max()))
    print("parity %s: L,S,P %s  frames %d  max|gpu-ref64| %.3e  max|ref32-ref64| %.3e  bar %.3e  largest feature %.1f"
          % (name, R.geometry(o), frames, err_gpu, err_32, 4 * err_32, top))
    _ROWS[name] = (R.geometry(o), frames, err_gpu, err_32)
    _write_table()
    assert err_32 >= 16 * float(np.spacing(np.float32(top))), (name, err_32, top)     # a usable yardstick
    assert err_gpu <= 4 * err_32, (name, err_gpu, err_32)
    return frames, err_gpu, err_32, refs


@pytest.mark.parametrize("name", list(OPTION_SETS))
def test_option_parity(name):
    P = H.pkg()
    kw = dict(OPTION_SETS[name], dither=0.0)
    o = R.options(**kw)
    L, S, _ = R.geometry(o)
    waves = _waves(o["sample_frequency"], L, S)
    got = P.mfcc(waves, **kw)
    counts = [g.shape[0] for g in got]
    assert 0 in counts and 1 in counts                                   # the edges of the frame count are in the set
    frames, _, err_32, refs = _parity(name, kw, waves, got)
    assert frames > 1000
    if o["energy_floor"] > 0:
        # a share of the frames, not all, sits exactly at log(energy_floor), in the restatement and in the kernel alike; a
        # frame whose unfloored energy is within the bar of the floor may fall on either side
        floor = np.log(np.float64(o["energy_floor"]))
        plain = R.options(**dict(kw, energy_floor=0.0))
        n_ref = n_gpu = n_all = 0
        for w, g, r64 in zip(waves, got, refs):
            if not g.size:
                continue
            e = R.mfcc(w, plain, np.float64)[:, 0]
            at_ref = r64[:, 0] == floor
            assert (at_ref == (e <= floor)).all()
            at_gpu = g[:, 0] == np.float32(floor)
            assert (g[:, 0] >= np.float32(floor)).all()
            clear = np.abs(e - floor) > 4 * err_32
            assert (at_gpu == at_ref)[clear].all()
            n_ref, n_gpu, n_all = n_ref + int(at_ref.sum()), n_gpu + int(at_gpu.sum()), n_all + len(e)
        print("energy floor %s: %d of %d frames at log(1e6) in the restatement, %d in the kernel" % (name, n_ref, n_all, n_gpu))
        assert 0.05 * n_all < n_ref < 0.95 * n_all and 0.05 * n_all < n_gpu < 0.95 * n_all


def test_few_ceps_are_the_first_columns_of_eight():
    """Coefficient c is the same sum over the mel bins, in the same order, whatever num-ceps is: with one, two or three
    coefficients (as many lanes in the DCT loop, a DCT table of another stride) the kernel gives the bytes of the first columns
    of the ceps_8_no_energy set, which test_option_parity holds to the restatement."""
    P = H.pkg()
    kw = dict(OPTION_SETS["ceps_8_no_energy"], dither=0.0)
    L, S, _ = R.geometry(R.options(**kw))
    waves = _waves(8000.0, L, S)
    eight = P.mfcc(waves, **kw)
    for nc in (1, 2, 3):
        got = P.mfcc(waves, **dict(kw, num_ceps=nc))
        for g, t in zip(got, eight):
            assert g.shape == (t.shape[0], nc) and g.tobytes() == np.ascontiguousarray(t[:, :nc]).tobytes()
    with_energy = P.mfcc(waves, **dict(kw, num_ceps=1, use_energy=True))      # and c0 is the energy when asked for
    for g, w in zip(with_energy, waves):
        if g.size:
            e = R.mfcc(w, R.options(**dict(kw, num_ceps=1, use_energy=True)), np.float64)
            assert np.abs(g - e).max() < 1e-4                                 # log of a sum of 200 squares: a few ulps of 20


DITHER_SETS = {
    "conf_mfcc_dither_1": dict(R.CONF_MFCC, dither=1.0),
    "conf_mfcc_dither_03": dict(R.CONF_MFCC, dither=0.3),
    "conf_mfcc_snip_edge_dither_1": dict(R.CONF_MFCC_SNIP_EDGE, dither=1.0),
    "conf_mfcc_snip_edge_dither_03": dict(R.CONF_MFCC_SNIP_EDGE, dither=0.3),
    "remove_dc_false_dither_1": dict(R.CONF_MFCC, dither=1.0, remove_dc_offset=False),
}


@pytest.mark.parametrize("name", list(DITHER_SETS))
def test_dither_parity(name):
    """The kernel's draws are dither_ref's: same key hash, same counter (frame within the utterance, sample within the
    window, the reflected ones included), same variance frame by frame.  The same float64 draws go to both restatements."""
    P = H.pkg()
    kw = DITHER_SETS[name]
    o = R.options(**kw)
    L, S, _ = R.geometry(o)
    one = L if o["snip_edges"] else S // 2                     # one frame; without snip-edges 40 samples under a window of 200
    waves = [speechlike(700, 12000), speechlike(701, 4000), np.zeros(8000, np.int16), speechlike(702, one), speechlike(703, 900),
             np.zeros(one, np.int16), speechlike(704, 30000)]
    keys = ["spkA-utt1", "spkA-utt2", "zero", "one-frame", "spkB-utt1", "", "sw02001-A_000098-001156"]
    got = P.mfcc(waves, keys=keys, **kw)
    assert [g.shape[0] for g in got][3] == 1
    noise = [D.draws(k, R.num_frames(len(w), o), L) for k, w in zip(keys, waves)]
    _parity(name, kw, waves, got, noise)
    # per input kind, for the log: speech, the all-zero waveform, the one-frame utterances
    for label, idx in (("speech", (0, 1, 4, 6)), ("all-zero", (2, 5)), ("one frame", (3, 5))):
        eg = max(float(np.abs(got[i] - R.mfcc(waves[i], o, np.float64, noise=noise[i])).max()) for i in idx)
        print("  %s %s: max|gpu-ref64| %.3e" % (name, label, eg))
    # another batch order gives every utterance the same bytes: the counter holds the frame within the utterance
    order = [6, 2, 0, 5, 3, 1, 4]
    again = P.mfcc([waves[i] for i in order], keys=[keys[i] for i in order], **kw)
    for j, i in enumerate(order):
        assert again[j].tobytes() == got[i].tobytes(), keys[i]
    # and the draws matter at this size: the undithered features are far outside the bar on the all-zero waveform
    plain = R.mfcc(waves[2], R.options(**dict(kw, dither=0.0)), np.float64)
    assert np.abs(got[2] - plain).max() > 1.0


# ---------------------------------------------------------------------------------------------------------------- VAD
def _vad_feats(dim, seed=0):
    """Utterances whose c0 straddles every threshold of the sweep (5, 5 +- half the mean): MFCC energies of speech, and
    uniform c0 in [-12, 25]; the other columns are noise the VAD must not read."""
    rng = np.random.default_rng(seed)
    o = R.options(**R.CONF_MFCC, dither=0.0)
    c0s = [R.mfcc(speechlike(800 + i, n), o, np.float32)[:, 0] for i, n in enumerate((8000, 40000))]
    c0s += [rng.uniform(-12, 25, n).astype(np.float32) for n in (1, 2, 3, 5, 16, 333, 1500)]
    return [np.concatenate([c[:, None], rng.standard_normal((len(c), dim - 1)).astype(np.float32) * 50], axis=1) for c in c0s]


def _tie_mask(f, v):
    """Frames where num == den * proportion in real arithmetic, proportion being the decimal the option was written as."""
    c0 = f[:, 0].astype(np.float64)
    T, ctx = len(c0), int(v["vad_frames_context"])
    p = fractions.Fraction(repr(v["vad_proportion_threshold"]))
    t = np.arange(T)
    lo, hi = np.maximum(0, t - ctx), np.minimum(T - 1, t + ctx)
    above = np.concatenate([[0], np.cumsum(c0 > R.vad_threshold(c0, v, np.float64))])
    num, den = above[hi + 1] - above[lo], hi - lo + 1
    return num * p.denominator == den * p.numerator


def _check_vad(feats, got, v, stats, fp32_thr=True):
    """Kernel against R.vad frame for frame.  Excluded: frames whose window holds a c0 within the fp32 spacing of the
    threshold (either side is right); counted in stats = [frames, excluded, ties, ties where fp32 and fp64 differ].  On a
    proportion tie the fp32 comparison is the truth (Kaldi's BaseFloat is float); elsewhere fp64 and fp32 agree."""
    ctx = int(v["vad_frames_context"])
    for f, g in zip(feats, got):
        assert g.shape == (f.shape[0],) and g.dtype == np.float32
        if not len(g):
            continue
        ref, ref32 = R.vad(f, v, np.float64), R.vad(f, v, np.float32)
        thr = float(R.vad_threshold(f[:, 0], v, np.float64))
        assert set(np.unique(g)) <= {0.0, 1.0}
        near = np.abs(f[:, 0].astype(np.float64) - thr) < np.spacing(np.float32(abs(thr)))
        k = min(ctx, len(near))                                            # a window wider than the utterance holds all of it
        shaky = np.convolve(near.astype(int), np.ones(2 * k + 1, int))[k:k + len(near)] > 0
        tie = _tie_mask(f, v)
        stats[0] += len(g)
        stats[1] += int(shaky.sum())
        stats[2] += int((tie & ~shaky).sum())
        stats[3] += int((tie & ~shaky & (ref32 != ref)).sum())
        ok = ~shaky
        if fp32_thr:                                                       # the restatement alone stays inside the cap too
            assert (ref32[ok & ~tie] == ref[ok & ~tie]).all()
            assert (g[ok & tie] == ref32[ok & tie]).all()
        assert (g[ok & ~tie] == ref[ok & ~tie]).all()


VAD_SWEEP = [dict(R.VAD_DEFAULTS, vad_frames_context=c, vad_proportion_threshold=p, vad_energy_mean_scale=m)
             for c in (0, 1, 7, 1000) for p in (1e-3, 0.5, 0.6, 0.999) for m in (0.0, 0.5, -0.5)]


@pytest.mark.parametrize("dim", [1, 23, 40])
def test_vad_sweep(dim):
    P = H.pkg()
    feats = _vad_feats(dim, seed=dim)
    empty = np.zeros((0, dim), np.float32)
    batch = [empty, empty] + feats[:4] + [empty] + feats[4:] + [empty]      # empty utterances at the start, inside, at the end
    stats = [0, 0, 0, 0]
    voiced = set()
    for v in [dict(R.VAD_DEFAULTS)] + VAD_SWEEP:
        got = P.vad(batch, **v)
        assert [len(g) for g in got] == [len(f) for f in batch]
        _check_vad(batch, got, v, stats)
        voiced.add(float(np.concatenate(got).mean()))
    print("vad sweep dim %d: %d option sets, frames %d, excluded near the threshold %d, ties %d (fp32 and fp64 differ on %d)"
          % ((dim, 1 + len(VAD_SWEEP)) + tuple(stats)))
    assert stats[1] <= 1e-3 * stats[0], stats
    assert stats[2] > 0 and len(voiced) > 20                               # the sweep meets ties and moves the decisions
    for v in (dict(R.VAD_DEFAULTS), VAD_SWEEP[0], VAD_SWEEP[17], VAD_SWEEP[-1]):     # alone: the same bytes as in the batch
        got = P.vad(batch, **v)
        for f, g in zip(batch, got):
            if len(f):
                assert P.vad([f], **v)[0].tobytes() == g.tobytes()


@pytest.mark.parametrize("v", [dict(R.VAD_DEFAULTS, vad_frames_context=2), dict(R.VAD_DEFAULTS, vad_frames_context=2, vad_energy_mean_scale=0.0),
                               dict(R.VAD_DEFAULTS, vad_frames_context=7), dict(R.VAD_DEFAULTS, vad_frames_context=1, vad_proportion_threshold=0.5),
                               dict(R.VAD_DEFAULTS, vad_frames_context=2, vad_proportion_threshold=0.5),
                               dict(R.VAD_DEFAULTS, vad_frames_context=7, vad_proportion_threshold=0.5),
                               dict(R.VAD_DEFAULTS, vad_frames_context=2, vad_proportion_threshold=0.2),
                               dict(R.VAD_DEFAULTS, vad_frames_context=1000, vad_proportion_threshold=0.5)],
                         ids=lambda v: "ctx%d_p%g_m%g" % (v["vad_frames_context"], v["vad_proportion_threshold"], v["vad_energy_mean_scale"]))
def test_vad_proportion_ties(v):
    """num == den * proportion exactly: 3 of 5 at 0.6 (5 * 0.6f rounds to 3.0f: voiced in Kaldi's float), 9 of 15, and every
    even window at 0.5, the clipped ones at the edges of an utterance included (2 frames at context 1, 4 at context 2)."""
    P = H.pkg()
    feats = _vad_feats(23, seed=99)
    rng = np.random.default_rng(5)
    lens = [4, 6, 10, 30, 2000, 2000] + list(rng.integers(2, 13, 300))          # many clipped windows: even ones tie at 0.5
    feats += [np.concatenate([rng.uniform(-12, 25, (n, 1)), np.zeros((n, 22))], axis=1).astype(np.float32) for n in lens]
    got = P.vad(feats, **v)
    stats = [0, 0, 0, 0]
    _check_vad(feats, got, v, stats)
    tie_voiced = 0
    for f, g in zip(feats, got):
        tie_voiced += int(g[_tie_mask(f, v)].sum())
    print("vad ties %s: frames %d, excluded %d, tie frames %d of which voiced %d; fp32 and fp64 restatements differ on %d of them"
          % ((v,) + tuple(stats[:3]) + (tie_voiced, stats[3])))
    assert stats[1] <= 1e-3 * stats[0] and stats[2] >= 20
    assert tie_voiced > 0              # a tie is voiced under >=: 3 >= 5 * 0.6f = 3.0f, n >= 2n * 0.5


def test_vad_thousands_of_short_utterances():
    P = H.pkg()
    rng = np.random.default_rng(11)
    feats = [np.concatenate([rng.uniform(-5, 25, (n, 1)), rng.standard_normal((n, 22))], axis=1).astype(np.float32)
             for n in rng.integers(1, 4, 5000)]
    for v in (dict(R.VAD_DEFAULTS), dict(R.CONF_VAD), dict(R.VAD_DEFAULTS, vad_frames_context=1, vad_proportion_threshold=0.5)):
        got = P.vad(feats, **v)
        stats = [0, 0, 0, 0]
        _check_vad(feats, got, v, stats)
        allg = np.concatenate(got)
        print("vad 5000 short utterances %s: frames %d, excluded %d, voiced %.3f" % (v, stats[0], stats[1], allg.mean()))
        assert stats[1] <= 1e-3 * stats[0] and 0.1 < allg.mean() < 0.9
        for i in list(range(0, 5000, 97)) + [4999]:
            assert P.vad([feats[i]], **v)[0].tobytes() == got[i].tobytes(), i


def test_vad_threshold_of_a_million_frames_with_a_common_offset():
    """c0 = 1000 + N(0, 3) over 10^6 frames, threshold = the mean (scale 1, offset 0).  One fp32 ulp at 1000 is 6.1e-5 and the
    density of c0 at the mean is 0.133 per unit: about 16 frames lie within an ulp of the threshold and are excluded with
    their windows.  A threshold summed in fp32 is off by far more (sequentially by tens; 64 partial sums of 1.6e7 each, one
    ulp 1 to 2, by about 1e-2, which flips some 10^3 frames); the kernel's fp64 sum is exact to 1e-7.  The fp32 restatement's
    own sum (numpy's pairwise one) is not held to the cap here; the count of its differences is printed."""
    P = H.pkg()
    rng = np.random.default_rng(21)
    n = 1000000
    f = np.concatenate([(1000.0 + 3.0 * rng.standard_normal((n, 1))), rng.standard_normal((n, 1))], axis=1).astype(np.float32)
    small = _vad_feats(2, seed=3)[2:6]
    for ctx in (0, 2):
        v = dict(R.VAD_DEFAULTS, vad_energy_threshold=0.0, vad_energy_mean_scale=1.0, vad_frames_context=ctx)
        got = P.vad(small + [f], **v)
        stats = [0, 0, 0, 0]
        _check_vad(small + [f], got, v, stats, fp32_thr=False)
        diff32 = int((R.vad(f, v, np.float32) != R.vad(f, v, np.float64)).sum())
        print("vad 10^6 frames ctx %d: excluded %d, voiced %.4f, fp32 restatement differs from fp64 on %d frames, its threshold by %.3e"
              % (ctx, stats[1], got[-1].mean(), diff32,
                 float(R.vad_threshold(f[:, 0], v, np.float32)) - float(R.vad_threshold(f[:, 0], v, np.float64))))
        assert stats[1] <= 1e-3 * stats[0] and 0.49 < got[-1].mean() < 0.51
        assert P.vad([f], **v)[0].tobytes() == got[-1].tobytes()


# -------------------------------------------------------------------------------------------------------------- tools
def _run(args, **kw):
    return subprocess.run(args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300, **kw)


TOOL_OPTS = dict(sample_frequency=16000.0, frame_shift=12.5, num_mel_bins=30, num_ceps=17, cepstral_lifter=10.0, energy_floor=1e6,
                 window_type="blackman", blackman_coeff=0.35, preemphasis_coefficient=0.9, remove_dc_offset=False)
TOOL_ARGV = ["--sample-frequency=16000", "--frame-shift=12.5", "--num-mel-bins=30", "--num-ceps=17", "--cepstral-lifter=10",
             "--energy-floor=1e6", "--window-type=blackman", "--blackman-coeff=0.35", "--preemphasis-coefficient=0.9",
             "--remove-dc-offset=false", "--channel=1", "--min-duration=0.5"]


def test_tool_flags_on_a_two_channel_file(tmp_path):
    """compute-mfcc-feats with a non-default value for every flag no other test passes, on channel 1 of a stereo file: the
    bytes of P.mfcc of that channel under the same options (dither at the tool's default 1, keyed by the utterance)."""
    P = H.pkg()
    d = tmp_path
    left, right = speechlike(900, 40000, 16000.0), speechlike(901, 40000, 16000.0)
    write_wav(str(d / "st.wav"), np.stack([left, right], axis=1), rate=16000, channels=2)
    write_wav(str(d / "short.wav"), np.stack([left[:4000], right[:4000]], axis=1), rate=16000, channels=2)     # 0.25 s
    (d / "wav.scp").write_text("utt-short %s/short.wav\nutt-st %s/st.wav\n" % (d, d))
    exe = os.path.join(BIN, "compute-mfcc-feats")
    r = _run([exe] + TOOL_ARGV + ["scp:%s/wav.scp" % d, "ark:%s/plain.ark" % d])
    err = r.stderr.decode()
    assert r.returncode == 0, err
    assert "WARNING" in err and "File: utt-short is too short (0.25 sec): producing no output." in err
    assert "Done 1 out of 2 utterances" in err
    got = dict(kio.read_ark(str(d / "plain.ark"), "matrix"))
    assert list(got) == ["utt-st"]
    want = P.mfcc([right], keys=["utt-st"], **TOOL_OPTS)[0]
    other = P.mfcc([left], keys=["utt-st"], **TOOL_OPTS)[0]
    plain = got["utt-st"].astype(np.float32)
    assert want.shape == (R.num_frames(40000, R.options(**TOOL_OPTS)), 17) and want.shape[0] == 1 + (40000 - 400) // 200
    assert plain.tobytes() == want.tobytes() and plain.tobytes() != other.tobytes()
    floor = np.float32(np.log(1e6))
    assert 0 < (want[:, 0] == floor).sum() < len(want)             # --energy-floor acts
    # every flag moves the features: dropping any one of them gives other bytes
    for k in TOOL_OPTS:
        if k != "sample_frequency":
            less = P.mfcc([right], keys=["utt-st"], **{a: b for a, b in TOOL_OPTS.items() if a != k})[0]
            assert less.shape != want.shape or less.tobytes() != want.tobytes(), k
    # --subtract-mean=true: that output minus its per-column mean (summed in fp64, rounded to float).  One fp32 subtraction
    # rounds by half an ulp of its result; rounding the mean to float moves it by half an ulp of the mean.
    r = _run([exe] + TOOL_ARGV + ["--subtract-mean=true", "scp:%s/wav.scp" % d, "ark:%s/cmn.ark" % d])
    assert r.returncode == 0, r.stderr.decode()
    cmn = dict(kio.read_ark(str(d / "cmn.ark"), "matrix"))["utt-st"].astype(np.float32)
    mean = want.astype(np.float64).mean(axis=0)
    exact = want.astype(np.float64) - mean[None, :]
    tol = 0.5 * np.spacing(np.abs(exact).astype(np.float32)).astype(np.float64) + 0.5 * np.spacing(np.abs(mean).astype(np.float32))[None, :]
    assert cmn.shape == want.shape and (np.abs(cmn.astype(np.float64) - exact) <= tol * (1 + 1e-6)).all()
    assert np.abs(cmn.astype(np.float64).mean(axis=0)).max() < 1e-5 and np.abs(mean).max() > 1.0
    # compute-vad with Kaldi's defaults (no option given) on what the tool writes without the floor (the floor of 13.8 lies
    # above the default threshold of 5 + mean / 2 = 13.3: every floored frame would be voiced)
    r = _run([exe] + TOOL_ARGV + ["--energy-floor=0", "scp:%s/wav.scp" % d, "ark:%s/nofloor.ark" % d])
    assert r.returncode == 0, r.stderr.decode()
    plain = dict(kio.read_ark(str(d / "nofloor.ark"), "matrix"))["utt-st"].astype(np.float32)
    assert plain.tobytes() == P.mfcc([right], keys=["utt-st"], **dict(TOOL_OPTS, energy_floor=0.0))[0].tobytes()
    r = _run([os.path.join(BIN, "compute-vad"), "ark:%s/nofloor.ark" % d, "ark:%s/vad.ark" % d])
    err = r.stderr.decode()
    assert r.returncode == 0 and "Done 1 utterances, 0 had empty features" in err, err
    vad = dict(kio.read_ark(str(d / "vad.ark"), "vector"))["utt-st"].astype(np.float32)
    assert vad.tobytes() == P.vad([plain])[0].tobytes()
    stats = [0, 0, 0, 0]
    _check_vad([plain], [vad], dict(R.VAD_DEFAULTS), stats)
    assert stats[1] <= 2 and 0 < vad.sum() < len(vad)
