"""GPU tests of the feature stage: the MFCC and energy-VAD kernels through the C ABI against tests/mfcc_ref.py, and the two
drop-in tools with the argv steps/make_mfcc.sh and sid/compute_vad_decision.sh build (stage 1 of egs/sre/v2/run_sre10.sh:78-90),
chained into nnet3-xvector-compute with the extraction script's feature pipeline.

Parity criterion per option set: max|gpu - ref64| <= 4 * max|ref32 - ref64| over the same elements, ref32 being the same
formulas with every intermediate rounded to fp32 (what a float build gives).  The 4 allows for another FFT factorisation and
other summation orders than the fp32 restatement's.  The pauses of the test signals carry a low noise floor, so no mel energy
sits at the log floor, where one ulp of the energy is a large step of its log.  Computed on the CPU beforehand, the
right-hand side max|ref32 - ref64| is 3.5e-4 to 5.9e-4 per option set on these inputs, against features of size 57 to 103: a
meaningful bar."""
import os
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest

import helpers as H
import mfcc_ref as R
from oracle import kaldi_io as kio

pytestmark = pytest.mark.gpu
BIN = os.path.join(H.ROOT, H.PKG_NAME, "bin")
CSRC = os.path.join(H.ROOT, H.PKG_NAME, "csrc")

OPTION_SETS = {
    "conf_mfcc": dict(R.CONF_MFCC),
    "conf_mfcc_snip_edge": dict(R.CONF_MFCC_SNIP_EDGE),
    "kaldi_default_16k": dict(),
    "use_energy_false": dict(R.CONF_MFCC, use_energy=False),
    "raw_energy_false": dict(R.CONF_MFCC, raw_energy=False),
    "hamming": dict(R.CONF_MFCC, window_type="hamming"),
    "hanning": dict(R.CONF_MFCC, window_type="hanning"),
    "rectangular": dict(R.CONF_MFCC, window_type="rectangular"),
    "blackman": dict(R.CONF_MFCC, window_type="blackman"),
}


def speechlike(seed, n, rate=8000.0):
    """int16 signal: bursts of band-limited noise plus tones, separated by pauses that keep a low noise floor."""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / rate
    x = rng.standard_normal(n) * 30.0                                   # the floor (never digital silence)
    pos = 0
    while pos < n:
        burst = int(rng.integers(int(0.05 * rate), int(0.6 * rate)))
        pause = int(rng.integers(int(0.02 * rate), int(0.4 * rate)))
        end = min(n, pos + burst)
        m = end - pos
        if m > 8:
            noise = rng.standard_normal(m)
            k = int(rng.integers(2, 12))                                # moving average = a low-pass of varying width
            noise = np.convolve(noise, np.ones(k) / k, mode="same")
            f1, f2 = rng.uniform(100, 0.2 * rate), rng.uniform(0.1 * rate, 0.45 * rate)
            seg = 3000.0 * noise + 2500.0 * np.sin(2 * np.pi * f1 * t[pos:end]) + 1200.0 * np.sin(2 * np.pi * f2 * t[pos:end] + 1.0)
            x[pos:end] += seg * np.hanning(m) * rng.uniform(0.3, 1.5)
        pos = end + pause
    return np.clip(np.round(x), -32768, 32767).astype(np.int16)


def parity_waves(rate):
    r = rate / 8000.0
    lens = [1, 39, 40, 199, 200, 279, 280, 1000, 8000, 24001, int(60 * 8000)]
    return [speechlike(100 + i, int(n * r) if n > 1000 else n, rate) for i, n in enumerate(lens)]


_PARITY_ROWS = {}


def _write_parity_table():
    path = os.environ.get("XVEC_MFCC_PARITY_MD")      # set by whoever refreshes profiles/mfcc_parity.md
    if not path or not _PARITY_ROWS:
        return
    with open(path, "w") as f:
        f.write("# MFCC parity: GPU kernel against tests/mfcc_ref.py (tests/test_gpu_mfcc.py::test_parity)\n\n"
                "Bar per option set: `max|gpu - ref64| <= 4 * max|ref32 - ref64|`, all with `--dither=0`, eleven utterances of "
                "1 sample to 60 s.\n\n| option set | frames | max abs(gpu - ref64) | max abs(ref32 - ref64) | bar (4 x) | inside |\n"
                "|---|---|---|---|---|---|\n")
        for name in OPTION_SETS:
            if name in _PARITY_ROWS:
                fr, g, r = _PARITY_ROWS[name]
                f.write("| %s | %d | %.3e | %.3e | %.3e | %s |\n" % (name, fr, g, r, 4 * r, "yes" if g <= 4 * r else "NO"))


@pytest.mark.parametrize("name", list(OPTION_SETS))
def test_parity(name):
    P = H.pkg()
    kw = dict(OPTION_SETS[name], dither=0.0)
    o = R.options(**kw)
    waves = parity_waves(o["sample_frequency"])
    got = P.mfcc(waves, **kw)
    err_gpu = err_32 = 0.0
    frames = 0
    for w, g in zip(waves, got):
        r64 = R.mfcc(w, o, np.float64)
        r32 = R.mfcc(w, o, np.float32)
        assert r32.dtype == np.float32 and g.dtype == np.float32
        assert g.shape == r64.shape == (R.num_frames(len(w), o), o["num_ceps"])
        frames += g.shape[0]
        if g.size:
            err_gpu = max(err_gpu, float(np.abs(g.astype(np.float64) - r64).max()))
            err_32 = max(err_32, float(np.abs(r32.astype(np.float64) - r64).max()))
    print("parity %s: frames %d  max|gpu-ref64| %.3e  max|ref32-ref64| %.3e  bar %.3e" % (name, frames, err_gpu, err_32, 4 * err_32))
    _PARITY_ROWS[name] = (frames, err_gpu, err_32)
    _write_parity_table()
    assert frames > 6000
    assert err_gpu <= 4 * err_32, (name, err_gpu, err_32)


def test_float_and_int16_inputs_give_the_same_bytes():
    P = H.pkg()
    waves = [speechlike(7, 5000), speechlike(8, 333)]
    a = P.mfcc(waves, dither=0.0, **R.CONF_MFCC)
    b = P.mfcc([w.astype(np.float32) for w in waves], dither=0.0, **R.CONF_MFCC)
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()


@pytest.mark.parametrize("name", ["conf_mfcc", "kaldi_default_16k", "use_energy_false"])
def test_digital_silence_is_the_closed_form_row(name):
    P = H.pkg()
    kw = dict(OPTION_SETS[name], dither=0.0)
    o = R.options(**kw)
    got = P.mfcc([np.zeros(20000, np.int16)], **kw)[0]
    want = R.silence_row(o)
    assert got.shape[0] == R.num_frames(20000, o) > 0
    # every log mel energy is log(FLT_EPSILON) = -15.94; a row is a sum of num_bins (23) products of size <= 4.7 whose partial
    # sums reach 76.5 (c0 without energy = sqrt(23) * -15.94; one fp32 ulp there is 7.6e-6): at most half an ulp per addition,
    # 23 * 3.8e-6 = 8.8e-5, plus the fp32 rounding of the table entries (23 * 4.7 * 6e-8 = 6.5e-6)
    assert np.abs(got - want[None, :]).max() < 1e-4, np.abs(got - want[None, :]).max()
    assert (got == got[0]).all()


def test_batch_invariance_without_dither():
    P = H.pkg()
    lens = [8000, 0, 1, 39, 40, 4321, 199, 16000, 0, 777]
    waves = [speechlike(300 + i, n) if n else np.zeros(0, np.int16) for i, n in enumerate(lens)]
    for conf in (R.CONF_MFCC, R.CONF_MFCC_SNIP_EDGE):
        full = P.mfcc(waves, dither=0.0, **conf)
        assert [f.shape[0] for f in full] == [R.num_frames(n, R.options(**conf)) for n in lens]
        assert sum(f.shape[0] == 0 for f in full) >= 3
        for i, w in enumerate(waves):
            alone = P.mfcc([w], dither=0.0, **conf)[0]
            assert alone.tobytes() == full[i].tobytes(), i
        part = P.mfcc(waves[3:8], dither=0.0, **conf)
        for i in range(5):
            assert part[i].tobytes() == full[3 + i].tobytes()


def test_dither_is_reproducible_and_independent_of_the_batch():
    P = H.pkg()
    waves = [speechlike(400 + i, n) for i, n in enumerate((4000, 900, 12000))]
    keys = ["spkA-utt1", "spkA-utt2", "spkB-utt1"]
    a = P.mfcc(waves, keys=keys, dither=1.0, **R.CONF_MFCC)
    b = P.mfcc(waves, keys=keys, dither=1.0, **R.CONF_MFCC)
    plain = P.mfcc(waves, keys=keys, dither=0.0, **R.CONF_MFCC)
    for i in range(3):
        assert a[i].tobytes() == b[i].tobytes()
        assert a[i].tobytes() != plain[i].tobytes()
        alone = P.mfcc([waves[i]], keys=[keys[i]], dither=1.0, **R.CONF_MFCC)[0]
        assert alone.tobytes() == a[i].tobytes()
    shard = P.mfcc([waves[2], waves[0]], keys=[keys[2], keys[0]], dither=1.0, **R.CONF_MFCC)   # another shard, another order
    assert shard[0].tobytes() == a[2].tobytes() and shard[1].tobytes() == a[0].tobytes()
    other = P.mfcc([waves[0]], keys=["someone-else"], dither=1.0, **R.CONF_MFCC)[0]           # the key is part of the draw
    assert other.tobytes() != a[0].tobytes()


def test_dither_statistics_on_an_all_zero_waveform():
    """x = 0, dither 1, DC removed, raw energy: exp(c0) = sum of squares of L iid N(0,1) draws minus L * mean^2, a chi-square
    with L - 1 degrees of freedom: its mean over F frames is L - 1 with standard deviation sqrt(2 (L - 1) / F).  Without the
    DC removal it is a chi-square with L degrees of freedom plus L mu^2 for any mean mu of the draws: the same kind of bound
    on it bounds the mean of the window samples (|mu| < 0.06)."""
    P = H.pkg()
    conf = dict(R.CONF_MFCC_SNIP_EDGE, dither=1.0, use_energy=True, raw_energy=True)
    L = 200
    n = 80 * 12000 + L
    z = [np.zeros(n, np.int16)]
    c0 = P.mfcc(z, keys=["zero"], remove_dc_offset=True, **conf)[0][:, 0].astype(np.float64)
    F = len(c0)
    assert F >= 10000
    e = np.exp(c0)
    sd = np.sqrt(2.0 * (L - 1) / F)
    print("dither: F %d  mean exp(c0) %.4f  expected %d  sd of the mean %.4f" % (F, e.mean(), L - 1, sd))
    assert abs(e.mean() - (L - 1)) < 6 * sd
    e2 = np.exp(P.mfcc(z, keys=["zero"], remove_dc_offset=False, **conf)[0][:, 0].astype(np.float64))
    sd2 = np.sqrt(2.0 * L / F)
    print("dither: without DC removal mean exp(c0) %.4f  expected %d  sd of the mean %.4f" % (e2.mean(), L, sd2))
    assert abs(e2.mean() - L) < 6 * sd2


def _vad_inputs():
    feats = []
    for i, n in enumerate((8000, 40000, 160000, 2400)):
        feats.append(R.mfcc(speechlike(500 + i, n), R.options(**R.CONF_MFCC, dither=0.0), np.float32))
    rng = np.random.default_rng(9)
    feats.append(np.array([[3.0] + [0.0] * 22], np.float32))                                   # a single frame
    feats.append(np.concatenate([rng.uniform(-2, 1, (300, 1)), rng.standard_normal((300, 22))], axis=1).astype(np.float32))   # silent
    feats.append(np.concatenate([rng.uniform(30, 31, (300, 1)), rng.standard_normal((300, 22))], axis=1).astype(np.float32))  # loud
    return feats


ABS_VAD = dict(vad_energy_threshold=5.5, vad_energy_mean_scale=0.0, vad_proportion_threshold=0.12, vad_frames_context=2)


def test_vad_matches_the_restatement_frame_for_frame():
    P = H.pkg()
    feats = _vad_inputs()
    got = P.vad(feats, **R.CONF_VAD)
    total = excluded = 0
    ctx = R.CONF_VAD["vad_frames_context"]
    for f, g in zip(feats, got):
        ref = R.vad(f, R.CONF_VAD, np.float64)
        ref32 = R.vad(f, R.CONF_VAD, np.float32)
        thr = float(R.vad_threshold(f[:, 0], R.CONF_VAD, np.float64))
        assert g.shape == ref.shape and set(np.unique(g)) <= {0.0, 1.0}
        # a c0 within the fp32 spacing of the threshold may fall on either side; so may the frames whose window holds it
        near = np.abs(f[:, 0].astype(np.float64) - thr) < np.spacing(np.float32(abs(thr)))
        shaky = np.convolve(near.astype(int), np.ones(2 * ctx + 1, int))[ctx:ctx + len(near)] > 0
        total += len(g)
        excluded += int(shaky.sum())
        assert (g[~shaky] == ref[~shaky]).all()
        assert (ref32[~shaky] == ref[~shaky]).all()        # the restatement alone stays inside the cap too
    assert excluded <= 1e-3 * total, (excluded, total)
    assert got[4].tolist() == [0.0]                        # thr = 5.5 + 0.5 * 3 > 3
    for i, f in enumerate(feats):                          # a batch and each utterance alone: the same decisions
        assert P.vad([f], **R.CONF_VAD)[0].tobytes() == got[i].tobytes()
    assert not P.vad([feats[5]], **ABS_VAD)[0].any()       # all silent under an absolute threshold
    assert P.vad([feats[6]], **ABS_VAD)[0].all()           # all loud above it


def _run(args, **kw):
    return subprocess.run(args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300, **kw)


def write_wav(path, x, rate=8000, channels=1):
    data = np.ascontiguousarray(x, dtype="<i2").tobytes()
    with open(path, "wb") as f:
        f.write(b"RIFF" + struct.pack("<I", 36 + len(data)) + b"WAVE" + b"fmt " +
                struct.pack("<IHHIIHH", 16, 1, channels, rate, rate * 2 * channels, 2 * channels, 16) + b"data" +
                struct.pack("<I", len(data)) + data)


def test_stage1_of_run_sre10_runs_with_the_recipes_argv_and_feeds_the_extraction(tmp_path):
    """steps/make_mfcc.sh:125-129 and sid/compute_vad_decision.sh:56-57 with their own argv, then the feats.scp and vad.scp
    just written through nnet3-xvector-compute with extract_xvectors_new.sh:79's pipeline string."""
    P = H.pkg()
    d = tmp_path
    (d / "conf").mkdir()
    (d / "conf" / "mfcc.conf").write_text("--sample-frequency=8000 \n--frame-length=25 # the default is 25\n--low-freq=20 # the default.\n"
                                          "--high-freq=3700 # the default is zero meaning use the Nyquist (4k in this case).\n"
                                          "--num-ceps=23 # higher than the default which is 12.\n--snip-edges=false\n")
    (d / "conf" / "vad.conf").write_text("--vad-energy-threshold=5.5\n--vad-energy-mean-scale=0.5\n--vad-proportion-threshold=0.12\n"
                                         "--vad-frames-context=2\n")
    lens = {"spk1-a": 40000, "spk1-b": 24000, "spk2-a": 56000, "spk2-pipe": 32000}
    waves = {k: speechlike(600 + i, n) for i, (k, n) in enumerate(lens.items())}
    for k, w in waves.items():
        write_wav(str(d / (k + ".wav")), w)
    with open(d / "wav.scp", "w") as f:
        f.write("spk1-a %s/spk1-a.wav\nspk1-b %s/spk1-b.wav\nspk1-missing %s/nosuch.wav\nspk2-a %s/spk2-a.wav\n"
                "spk2-pipe cat %s/spk2-pipe.wav |\n" % ((d,) * 5))
    env = dict(os.environ, PATH=BIN + os.pathsep + os.environ.get("PATH", ""))
    cmd = ("compute-mfcc-feats --verbose=2 --config=%s/conf/mfcc.conf scp,p:%s/wav.scp ark:- | "
           "copy-feats --write-num-frames=ark,t:%s/utt2num_frames.1 --compress=true ark:- ark,scp:%s/raw_mfcc.1.ark,%s/feats.scp"
           % ((d,) * 5))
    r = _run(["bash", "-c", "set -o pipefail; " + cmd], env=env)
    err = r.stderr.decode()
    assert r.returncode == 0, err
    assert "WARNING" in err and "spk1-missing" in err and "Done 4 out of 5 utterances" in err
    o = R.options(**R.CONF_MFCC)
    n2f = dict(l.split() for l in open(d / "utt2num_frames.1").read().splitlines())
    assert n2f == {k: str(R.num_frames(n, o)) for k, n in lens.items()}
    feats = dict(kio.read_scp(str(d / "feats.scp"), "matrix"))        # the scp offsets resolve
    assert list(feats) == ["spk1-a", "spk1-b", "spk2-a", "spk2-pipe"]
    for k, w in waves.items():
        same = P.mfcc([w], keys=[k], dither=1.0, **R.CONF_MFCC)[0]    # the tool's default dither, keyed by the utterance
        assert feats[k].astype(np.float32).tobytes() == same.tobytes(), k
    r = _run([os.path.join(BIN, "compute-vad"), "--config=%s/conf/vad.conf" % d, "scp:%s/feats.scp" % d,
              "ark,scp:%s/vad.1.ark,%s/vad.scp" % (d, d)])
    err = r.stderr.decode()
    assert r.returncode == 0, err
    assert "Done 4 utterances, 0 had empty features" in err and "Proportion of voiced frames was" in err
    vads = dict(kio.read_scp(str(d / "vad.scp"), "vector"))
    for k in lens:
        want = P.vad([feats[k]], **R.CONF_VAD)[0]
        assert vads[k].astype(np.float32).tobytes() == want.tobytes()
        assert want.sum() > 0
    # stage 6's pipeline string on what stage 1 wrote
    net, line = H.synth_model("v2_xvector")
    (d / "final.raw").write_bytes(net.to_bytes(True))
    (d / "extract.config").write_text(line + "\n")
    feat = ("ark:apply-cmvn-sliding --norm-vars=false --center=true --cmn-window=300 scp:%s/feats.scp ark:- | "
            "select-voiced-frames ark:- scp,s,cs:%s/vad.scp ark:- |" % (d, d))
    r = _run([os.path.join(BIN, "nnet3-xvector-compute"), "--use-gpu=no", "--min-chunk-size=25", "--chunk-size=10000",
              "%s/nnet3-copy --nnet-config=%s/extract.config %s/final.raw - |" % (BIN, d, d), feat,
              "ark,scp:%s/xvector.1.ark,%s/xvector.1.scp" % (d, d)], env=env)
    assert r.returncode == 0, r.stderr.decode()
    xv = dict(kio.read_scp(str(d / "xvector.1.scp"), "vector"))
    assert list(xv) == list(feats) and all(np.isfinite(v).all() and v.shape == (512,) for v in xv.values())


def test_tools_exit_codes(tmp_path):
    d = tmp_path
    write_wav(str(d / "a.wav"), speechlike(1, 100))            # shorter than a window with snip-edges: an empty matrix
    write_wav(str(d / "b.wav"), speechlike(2, 4000), rate=16000)
    (d / "wav.scp").write_text("a %s/a.wav\nb %s/b.wav\n" % (d, d))
    r = _run([os.path.join(BIN, "compute-mfcc-feats"), "--sample-frequency=8000", "--dither=0", "scp:%s/wav.scp" % d, "ark:%s/o.ark" % d])
    err = r.stderr.decode()
    assert r.returncode == 0 and "Sample frequency mismatch" in err and "Done 1 out of 2" in err, err
    got = dict(kio.read_ark(str(d / "o.ark"), "matrix"))
    assert list(got) == ["a"] and got["a"].shape[0] == 0
    r = _run([os.path.join(BIN, "compute-vad"), "ark:%s/o.ark" % d, "ark:/dev/null"])
    assert r.returncode == 1 and b"Empty features for utterance a" in r.stderr and b"Done 0 utterances, 1 had empty features" in r.stderr
    (d / "bad.scp").write_text("x %s/nosuch.wav\n" % d)
    r = _run([os.path.join(BIN, "compute-mfcc-feats"), "scp:%s/bad.scp" % d, "ark:/dev/null"])     # without ,p: fatal
    assert r.returncode == 255 and b"Failed to read wave data for key x" in r.stderr


def test_feature_kernels_use_no_scratch():
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-c", os.path.join(CSRC, "feat_kernels.hip"),
                        "-o", os.devnull, "-Rpass-analysis=kernel-resource-usage"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:]
    names = re.findall(r"Function Name: (\S+)", r.stdout)
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stdout)]
    spills = [int(x) for x in re.findall(r"[VS]GPRs Spill: (\d+)", r.stdout)]
    assert len(names) == 4 and len(scratch) == 4, r.stdout[-2000:]       # mfcc f32 / i16, the two VAD kernels
    assert not any(scratch) and not any(spills), list(zip(names, scratch))
