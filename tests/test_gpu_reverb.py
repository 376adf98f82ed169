"""GPU tests of the augmentation stage: the reverberation kernels through the C ABI against tests/reverb_ref.py, and the
drop-in tool wav-reverberate.

Float parity per case: max|gpu - ref64| <= 4 * max|ref32 - ref64| over the same samples (the criterion and the factor of
tests/test_gpu_mfcc.py: another FFT factorisation and other summation orders than the fp32 restatement's), the right-hand side
computed here from the two restatements.  A case is one utterance: one (impulse response or option set, signal length) pair,
compared and asserted on its own samples.  The
kernel's partition size is 2048 taps and filters of up to 64 taps are convolved directly, so the RIR lengths stand below, at
and above both.  int16 parity of the tool's file: no sample further than 1 from trunc(ref64), and the share of differing
samples at most 4 x the share by which trunc(ref32) differs, with a floor of 1e-4.
The kernels' own edges (partitions, early slice, chunks, saturation thresholds, group cap): tests/test_gpu_reverb_edges.py."""
import os
import subprocess

import numpy as np
import pytest

import helpers as H
import reverb_ref as R

pytestmark = pytest.mark.gpu
BIN = os.path.join(H.ROOT, H.PKG_NAME, "bin")
TOOL = os.path.join(BIN, "wav-reverberate")
RATE = 8000.0

_ROWS = []


def _record(case, samples, err_gpu, err_32):
    print("parity %s: samples %d  max|gpu-ref64| %.3e  max|ref32-ref64| %.3e  bar %.3e" % (case, samples, err_gpu, err_32, 4 * err_32))
    _ROWS.append((case, samples, err_gpu, err_32))
    path = os.environ.get("XVEC_REVERB_PARITY_MD")      # set by whoever refreshes profiles/reverb_parity.md
    if not path:
        return
    with open(path, "w") as f:
        f.write("# wav-reverberate parity: GPU kernels against tests/reverb_ref.py (tests/test_gpu_reverb.py)\n\n"
                "Bar per case: `max|gpu - ref64| <= 4 * max|ref32 - ref64|`.\n\n"
                "| case | samples | max abs(gpu - ref64) | max abs(ref32 - ref64) | bar (4 x) | inside |\n|---|---|---|---|---|---|\n")
        for c, n, g, r in _ROWS:
            f.write("| %s | %d | %.3e | %.3e | %.3e | %s |\n" % (c, n, g, r, 4 * r, "yes" if g <= 4 * r else "NO"))


def _parity(case, waves, rirs, additive, **opts):
    P = H.pkg()
    got = P.reverberate(waves, rirs=rirs, additive=additive, rate=RATE, **opts)
    kw = {k: (bool(v) if k in ("shift_output", "normalize_output") else v) for k, v in opts.items()}
    bad = []
    for u, (w, g) in enumerate(zip(waves, got)):
        args = dict(rir=None if rirs is None else rirs[u], additive=() if additive is None else additive[u], **kw)
        r64 = R.reverberate(w, RATE, dtype=np.float64, **args)
        r32 = R.reverberate(w, RATE, dtype=np.float32, **args)
        assert g.dtype == np.float32 and r32.dtype == np.float32 and g.shape == r64.shape == r32.shape, (case, u, g.shape, r64.shape)
        assert g.size and np.isfinite(g).all()
        err_gpu = float(np.abs(g.astype(np.float64) - r64).max())
        err_32 = float(np.abs(r32.astype(np.float64) - r64).max())
        name = "%s, signal %d" % (case, len(w))
        _record(name, g.size, err_gpu, err_32)
        if not err_gpu <= 4 * err_32:
            bad.append((name, err_gpu, err_32))
    assert not bad, bad


SIG_LENS = (1, 39, 8000, 480000)


@pytest.mark.parametrize("rir_len", [1, 63, 64, 65, 2047, 2048, 2049, 4000, 8000, 16001])
def test_parity_reverberation_only(rir_len):
    waves = [R.speechlike(100 + i, n) for i, n in enumerate(SIG_LENS)]
    h = R.decaying_rir(rir_len, rir_len, t60=0.2 + rir_len / 16000.0).astype(np.float32)
    _parity("rir %d" % rir_len, waves, [h] * len(waves), None)


def test_parity_ten_minutes_through_4000_taps():
    w = R.speechlike(200, 4800000)
    h = R.decaying_rir(201, 4000).astype(np.float32)
    _parity("4.8M samples, rir 4000", [w], [h], None)


def _noises(seed, lens):
    return [R.speechlike(seed + i, n).astype(np.float32) for i, n in enumerate(lens)]


OPTION_SETS = {
    "defaults": dict(),
    "shift_output=false": dict(shift_output=0),
    "normalize_output=false": dict(normalize_output=0),
    "shift and normalize false": dict(shift_output=0, normalize_output=0),
    "volume=0.5": dict(volume=0.5),
    "duration=0.5": dict(duration=0.5),
    "duration=70": dict(duration=70.0),
    "duration=70, no shift": dict(duration=70.0, shift_output=0),
}


@pytest.mark.parametrize("what", ["noise only", "both"])
@pytest.mark.parametrize("name", list(OPTION_SETS))
def test_parity_options(name, what):
    waves = [R.speechlike(300 + i, n) for i, n in enumerate(SIG_LENS)]
    h = R.decaying_rir(301, 4000).astype(np.float32)
    nz = _noises(310, (480000, 16000, 3000))
    # a background stretched over the recording, a foreground event inside it, one cut by the end, one starting beyond the end
    additive = [[(nz[0], 15.0, 0.0), (nz[1], 5.0, 0.004), (nz[2], 0.0, len(w) / RATE * 0.9), (nz[2], 10.0, len(w) / RATE + 1.0)] for w in waves]
    _parity("%s, %s" % (what, name), waves, [h] * len(waves) if what == "both" else None, additive, **OPTION_SETS[name])


def test_float_and_int16_inputs_give_the_same_bytes_and_int16_is_the_truncation():
    P = H.pkg()
    waves = [R.speechlike(400, 20000), R.speechlike(401, 333)]
    h = R.decaying_rir(402, 3000).astype(np.float32)
    a = P.reverberate(waves, rirs=[h, h], rate=RATE, return_int16=True, volume=6.0)      # loud enough to clip
    b = P.reverberate([w.astype(np.float32) for w in waves], rirs=[h, h], rate=RATE, volume=6.0)
    for (f, q, clipped), g in zip(a, b):
        assert f.tobytes() == g.tobytes()
        want, c = R.quantize(f)
        assert np.array_equal(q, want) and clipped == c
    assert a[0][2] > 0


def test_an_utterances_output_depends_on_the_utterance_alone():
    P = H.pkg()
    rng = np.random.default_rng(5)
    rir_lens = [1, 64, 65, 700, 2048, 2049, 5000, 16001]
    rir_list = [R.decaying_rir(500 + i, n).astype(np.float32) for i, n in enumerate(rir_lens)]
    target = R.speechlike(510, 50000)
    noise = R.speechlike(511, 30000).astype(np.float32)
    others = [R.speechlike(520 + i, int(n)) for i, n in enumerate(rng.integers(1, 90000, 31))]
    for t_rir in (3, 6, 1):
        alone = P.reverberate([target], rirs=[t_rir], additive=[[(noise, 8.0, 0.5)]], rate=RATE, rir_list=rir_list)[0]
        for idx in (0, 31):
            waves = others[:idx] + [target] + others[idx:]
            rirs = [int(r) if r < len(rir_lens) else None for r in rng.integers(0, len(rir_lens) + 2, 32)]
            additive = [[(noise, float(rng.uniform(0, 20)), float(rng.uniform(0, 3)))] if rng.uniform() < 0.5 else [] for _ in range(32)]
            rirs[idx] = t_rir
            additive[idx] = [(noise, 8.0, 0.5)]
            assert waves[idx] is target and len(waves) == 32
            got = P.reverberate(waves, rirs=rirs, additive=additive, rate=RATE, rir_list=rir_list)[idx]
            assert got.tobytes() == alone.tobytes(), (t_rir, idx)


def test_groups_of_bounded_spectra_give_the_same_bytes(monkeypatch):
    """The signal spectra are held for a bounded number of FFT blocks at a time (512 MiB); with the cap lowered to 40 blocks
    (XVEC_DEBUG=reverb_group_blocks) a batch goes through in several groups, one utterance larger than the cap alone."""
    P = H.pkg()
    rir_list = [R.decaying_rir(800 + i, n).astype(np.float32) for i, n in enumerate((3, 700, 5000))]
    waves = [R.speechlike(810 + i, n) for i, n in enumerate((30000, 100, 50000, 2000, 200000, 9000, 61000, 4000))]
    rirs = [1, 0, 2, None, 2, 1, 1, 0]
    whole = P.reverberate(waves, rirs=rirs, rate=RATE, rir_list=rir_list)
    monkeypatch.setenv("XVEC_DEBUG", "reverb_group_blocks=40")
    grouped = P.reverberate(waves, rirs=rirs, rate=RATE, rir_list=rir_list)
    for a, b in zip(whole, grouped):
        assert a.tobytes() == b.tobytes()


def _run(args, **kw):
    return subprocess.run(args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600, **kw)


def _share(a, b):
    return float((a != b).mean())


def test_tool_writes_the_truncation_of_the_reference(tmp_path):
    P = H.pkg()
    d = tmp_path
    x = R.speechlike(600, 60 * 8000)
    h = R.decaying_rir(601, 4000)
    n1, n2 = R.speechlike(602, 60 * 8000), R.speechlike(603, 24000)
    for name, w in (("in", x), ("rir", h), ("n1", n1), ("n2", n2)):
        assert P.write_wave(str(d / (name + ".wav")), w, 8000) == 0
    cases = {
        "reverb": (["--shift-output=true", '--impulse-response=cat %s/rir.wav |' % d], dict(rir=h)),
        "noise": (["--additive-signals=%s/n1.wav,cat %s/n2.wav |" % (d, d), "--snrs=15,5", "--start-times=0,12.5"],
                  dict(additive=[(n1, 15.0, 0.0), (n2, 5.0, 12.5)])),
        "both": (["--impulse-response=%s/rir.wav" % d, "--additive-signals=%s/n1.wav" % d, "--snrs=10", "--start-times=0",
                  "--duration=45.5"], dict(rir=h, additive=[(n1, 10.0, 0.0)], duration=45.5)),
    }
    for name, (argv, kw) in cases.items():
        out = str(d / (name + ".out.wav"))
        r = _run([TOOL] + argv + ["cat %s/in.wav |" % d if name == "noise" else "%s/in.wav" % d, out])
        assert r.returncode == 0, r.stderr.decode()
        rate, got = P.read_wave(out)
        q64, _ = R.quantize(R.reverberate(x, RATE, dtype=np.float64, **kw))
        q32, _ = R.quantize(R.reverberate(x, RATE, dtype=np.float32, **kw))
        assert rate == 8000 and got.shape == q64.shape
        worst = int(np.abs(got.astype(np.int32) - q64.astype(np.int32)).max())
        s_gpu, s_32 = _share(got, q64), _share(q32, q64)
        print("int16 parity %s: samples %d  max step %d  share gpu %.3e  share ref32 %.3e" % (name, got.size, worst, s_gpu, s_32))
        assert worst <= 1
        assert s_gpu <= max(4 * s_32, 1e-4), (name, s_gpu, s_32)
    # through stdin and stdout, as the wav.scp lines use it
    r = _run(["bash", "-c", "set -o pipefail; cat %s/in.wav | %s --impulse-response=%s/rir.wav - - > %s/piped.wav" % (d, TOOL, d, d)])
    assert r.returncode == 0, r.stderr.decode()
    assert open(d / "piped.wav", "rb").read() == open(d / "reverb.out.wav", "rb").read()


def test_tool_errors(tmp_path):
    P = H.pkg()
    d = tmp_path
    P.write_wave(str(d / "in.wav"), R.speechlike(700, 8000), 8000)
    P.write_wave(str(d / "rir16.wav"), R.decaying_rir(701, 500), 16000)
    P.write_wave(str(d / "rir.wav"), R.decaying_rir(701, 500), 8000)
    P.write_wave(str(d / "n16.wav"), R.speechlike(702, 8000), 16000)
    P.write_wave(str(d / "n.wav"), R.speechlike(702, 8000), 8000)
    out = str(d / "o.wav")
    r = _run([TOOL, "--impulse-response=%s/rir16.wav" % d, "%s/in.wav" % d, out])
    assert r.returncode == 255 and b"sampling frequency mismatch: the impulse response" in r.stderr
    r = _run([TOOL, "--additive-signals=%s/n16.wav" % d, "--snrs=5", "--start-times=0", "%s/in.wav" % d, out])
    assert r.returncode == 255 and b"sampling frequency mismatch: the additive signal" in r.stderr
    r = _run([TOOL, "--additive-signals=%s/n.wav,%s/n.wav" % (d, d), "--snrs=5", "--start-times=0,1", "%s/in.wav" % d, out])
    assert r.returncode == 255 and b"must list the same number of elements (2, 1, 2)" in r.stderr
    r = _run([TOOL, "--impulse-response=%s/nosuch.wav" % d, "%s/in.wav" % d, out])
    assert r.returncode == 255 and b"ERROR (wav-reverberate)" in r.stderr and b"nosuch.wav" in r.stderr
    assert not os.path.exists(out)
    r = _run([TOOL, "--verbose=1", "--impulse-response=%s/rir.wav" % d, "--additive-signals=%s/n.wav" % d, "--snrs=5", "--start-times=0",
              "%s/in.wav" % d, out])
    assert r.returncode == 0 and b"Wrote 8000 samples" in r.stderr, r.stderr.decode()
    assert P.read_wave(out)[1].shape == (8000,)


def test_tool_warns_once_about_clipped_samples(tmp_path):
    P = H.pkg()
    d = tmp_path
    x = R.speechlike(750, 16000)
    P.write_wave(str(d / "in.wav"), x, 8000)
    r = _run([TOOL, "--volume=8", "%s/in.wav" % d, "%s/o.wav" % d])
    want, clipped = R.quantize(x.astype(np.float32) * np.float32(8))
    assert clipped > 0 and r.returncode == 0, r.stderr.decode()
    lines = [l for l in r.stderr.decode().splitlines() if "clipped" in l]
    assert len(lines) == 1 and lines[0].startswith("WARNING (wav-reverberate[") and lines[0].count("WARNING") == 1
    assert "clipped %d samples out of total 16000" % clipped in lines[0]
    assert np.array_equal(P.read_wave(str(d / "o.wav"))[1], want)


# ---- compute-mfcc-feats on the wav.scp lines of stage 2
MFCC_CONF = ("--sample-frequency=8000 \n--frame-length=25 # the default is 25\n--low-freq=20 # the default.\n"
             "--high-freq=3700 # the default is zero meaning use the Nyquist (4k in this case).\n"
             "--num-ceps=23 # higher than the default which is 12.\n--snip-edges=false\n")


def _stage2_dir(d):
    P = H.pkg()
    (d / "conf").mkdir()
    (d / "conf" / "mfcc.conf").write_text(MFCC_CONF)
    files = {"a": R.speechlike(900, 40000), "b": R.speechlike(901, 24000), "c": R.speechlike(902, 56000),
             "rir1": R.decaying_rir(903, 3000), "rir2": R.decaying_rir(904, 40), "n1": R.speechlike(905, 30000),
             "n2": R.speechlike(906, 8000), "music": R.speechlike(907, 12000)}
    for k, w in files.items():
        P.write_wave(str(d / (k + ".wav")), w, 8000)
    P.write_wave(str(d / "rir16k.wav"), R.decaying_rir(908, 500), 16000)
    return files


def _scp_lines(d):
    """(key, entry, taken over?) in the shapes of reverberate_data_dir.py:366, :291-294, :220-232, :273-275 and
    augment_data_dir_new.py:86-116, sources as files and as pipes."""
    d = str(d)
    return [
        ("clean-a", "%s/a.wav" % d, False),
        ("rev1-a", 'cat %s/a.wav | wav-reverberate --shift-output=true --impulse-response="cat %s/rir1.wav |" - - |' % (d, d), True),
        ("rev2-b", "wav-reverberate --shift-output=true --impulse-response=%s/rir2.wav %s/b.wav - |" % (d, d), True),
        ("rev3-c", ('cat %s/c.wav | wav-reverberate --shift-output=true --impulse-response="cat %s/rir1.wav |" '
                    "--additive-signals='wav-reverberate --impulse-response=\"cat %s/rir2.wav |\" --duration=7.0 %s/n1.wav - |,"
                    "wav-reverberate --impulse-response=%s/rir1.wav %s/n2.wav - |' --start-times='0,2.5' --snrs='12,4' - - |"
                    % (d, d, d, d, d, d)), True),
        ("noise-a", ("wav-reverberate --shift-output=true --additive-signals='%s/n2.wav,cat %s/n1.wav |' --start-times='0,1.25' "
                     "--snrs='15,10' %s/a.wav - |" % (d, d, d)), True),
        ("music-b", ("cat %s/b.wav | wav-reverberate --shift-output=true --additive-signals='cat %s/music.wav | wav-reverberate "
                     "--duration=3.0 - - |' --start-times='0' --snrs='8' - - |" % (d, d)), True),
        ("babble-c", ("wav-reverberate --shift-output=true --additive-signals='wav-reverberate --duration=7.0 %s/n1.wav - |,"
                      "wav-reverberate --duration=7.0 %s/n2.wav - |,wav-reverberate --duration=7.0 %s/music.wav - |' "
                      "--start-times='0,0,0' --snrs='17,15,13' %s/c.wav - |" % (d, d, d, d)), True),
        ("loud-a", "cat %s/a.wav | wav-reverberate --volume=9 --duration=2.5 - - |" % d, True),
        ("verbose-b", "cat %s/b.wav | wav-reverberate --verbose=1 --impulse-response=%s/rir2.wav - - |" % (d, d), False),
        ("piped-c", "cat %s/c.wav | wav-reverberate --impulse-response=%s/rir2.wav - - | cat |" % (d, d), False),
    ]


def _mfcc_job(d, scp, out, dither, fuse):
    env = dict(os.environ, PATH=BIN + os.pathsep + os.environ.get("PATH", ""))
    if not fuse:
        env["XVEC_DEBUG"] = "fuse_wav=0"
    cmd = ("compute-mfcc-feats --verbose=2 --config=%s/conf/mfcc.conf %s scp,p:%s ark:- | "
           "copy-feats ark:- ark,scp:%s.ark,%s.scp" % (d, "" if dither else "--dither=0", scp, out, out))
    return _run(["bash", "-c", "set -o pipefail; " + cmd], env=env)


@pytest.mark.parametrize("dither", [1.0, 0.0])
def test_fused_and_unfused_jobs_write_the_same_bytes(tmp_path, dither):
    P = H.pkg()
    d = tmp_path
    _stage2_dir(d)
    lines = _scp_lines(d)
    for key, entry, taken in lines:
        assert (P.recognize_wav_pipeline(entry) is not None) == (taken and True), key
    (d / "wav.scp").write_text("".join("%s %s\n" % (k, e) for k, e, _ in lines))
    outs = {}
    for fuse in (True, False):
        out = str(d / ("fused" if fuse else "plain"))
        r = _mfcc_job(d, d / "wav.scp", out, dither, fuse)
        err = r.stderr.decode()
        assert r.returncode == 0, err
        assert "Done %d out of %d utterances" % (len(lines), len(lines)) in err
        n_taken = sum(t for _, _, t in lines) if fuse else 0
        assert "Took over %d wav-reverberate entries" % n_taken in err, err
        assert ("(fuse_wav=0)" in err) == (not fuse)
        assert ("clipped" in err)                       # loud-a clips, in the tool's process or here
        outs[fuse] = (open(out + ".ark", "rb").read(), open(out + ".scp").read().replace(out, "X"))
    assert outs[True][1] == outs[False][1]
    assert outs[True][0] == outs[False][0]
    assert len(outs[True][0]) > 100000


def test_stage2_entries_that_fail_are_skipped_under_scp_p(tmp_path):
    d = tmp_path
    _stage2_dir(d)
    s = str(d)
    lines = [
        ("ok-a", "cat %s/a.wav | wav-reverberate --impulse-response=%s/rir2.wav - - |" % (s, s)),
        ("bad-rate-rir", "cat %s/a.wav | wav-reverberate --impulse-response=%s/rir16k.wav - - |" % (s, s)),
        ("bad-rate-noise", "wav-reverberate --additive-signals='%s/rir16k.wav' --snrs='5' --start-times='0' %s/a.wav - |" % (s, s)),
        ("bad-counts", "wav-reverberate --additive-signals='%s/n1.wav,%s/n2.wav' --snrs='5' --start-times='0,1' %s/a.wav - |" % (s, s, s)),
        ("missing-rir", "cat %s/a.wav | wav-reverberate --impulse-response=%s/nosuch.wav - - |" % (s, s)),
        ("ok-b", "wav-reverberate --additive-signals='%s/n2.wav' --snrs='5' --start-times='0' %s/b.wav - |" % (s, s)),
    ]
    (d / "wav.scp").write_text("".join("%s %s\n" % kv for kv in lines))
    outs = {}
    for fuse in (True, False):
        out = str(d / ("fused" if fuse else "plain"))
        r = _mfcc_job(d, d / "wav.scp", out, 0.0, fuse)
        err = r.stderr.decode()
        assert r.returncode == 0, err
        assert "Done 2 out of 6 utterances" in err, err
        for key in ("bad-rate-rir", "bad-rate-noise", "bad-counts", "missing-rir"):
            assert any("WARNING" in l and key in l for l in err.splitlines()), (key, err)
        if fuse:
            assert "sampling frequency mismatch: the impulse response" in err and "must list the same number of elements (2, 1, 2)" in err
        outs[fuse] = open(out + ".ark", "rb").read()
        assert [l.split()[0] for l in open(out + ".scp")] == ["ok-a", "ok-b"]
    assert outs[True] == outs[False]
    # without ,p the first bad entry ends the job
    env = dict(os.environ, PATH=BIN + os.pathsep + os.environ.get("PATH", ""))
    r = _run([os.path.join(BIN, "compute-mfcc-feats"), "--config=%s/conf/mfcc.conf" % s, "scp:%s/wav.scp" % s, "ark:/dev/null"], env=env)
    assert r.returncode == 255 and b"Failed to read wave data for key bad-rate-rir" in r.stderr
