"""CPU tests of the host half of the feature stage: frame counts through the C ABI against hand-worked cases, the RIFF/WAVE
reader on generated files, --config parsing, and the tools' early errors (exit 255 before any device is touched)."""
import os
import struct
import subprocess

import numpy as np
import pytest

import helpers as H

BIN = os.path.join(H.ROOT, H.PKG_NAME, "bin")
CONF = dict(sample_frequency=8000.0, frame_length=25.0, low_freq=20.0, high_freq=3700.0, num_ceps=23)


def _run(args, **kw):
    return subprocess.run(args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120, **kw)


def riff(x, rate=8000, channels=1, bits=16, extra=b"", data_size=None, riff_size=None):
    data = np.ascontiguousarray(x, dtype="<i2" if bits == 16 else "u1").tobytes()
    fmt = struct.pack("<IHHIIHH", 16, 1, channels, rate, rate * channels * bits // 8, channels * bits // 8, bits)
    body = b"WAVE" + b"fmt " + fmt + extra + b"data" + struct.pack("<I", len(data) if data_size is None else data_size) + data
    return b"RIFF" + struct.pack("<I", len(body) if riff_size is None else riff_size) + body


def test_num_frames_hand_worked():
    P = H.pkg()
    # 8 kHz: L = 200, S = 80.  snip-edges=true: 1 + (n - 200) // 80 for n >= 200
    for n, f in ((0, 0), (1, 0), (199, 0), (200, 1), (279, 1), (280, 2), (8000, 98)):
        assert P.mfcc_num_frames(n, snip_edges=True, **CONF) == f, n
    # snip-edges=false: (n + 40) // 80
    for n, f in ((0, 0), (1, 0), (39, 0), (40, 1), (119, 1), (120, 2), (200, 3), (8000, 100)):
        assert P.mfcc_num_frames(n, snip_edges=False, **CONF) == f, n
    # 16 kHz defaults: L = 400, S = 160
    assert P.mfcc_num_frames(399) == 0 and P.mfcc_num_frames(400) == 1 and P.mfcc_num_frames(16000) == 98
    for bad in (dict(round_to_power_of_two=0), dict(num_ceps=24, num_mel_bins=23), dict(sample_frequency=0.0), dict(frame_length=1000.0)):
        with pytest.raises(P.XvError):
            P.mfcc_num_frames(1000, **bad)
    with pytest.raises(P.XvError, match="Invalid window type"):
        P.mfcc_options(window_type="kaiser")
    o = P.mfcc_options()
    assert (o.sample_frequency, o.dither, o.num_mel_bins, o.num_ceps, o.cepstral_lifter, o.snip_edges) == (16000.0, 1.0, 23, 13, 22.0, 1)
    assert P.utt_seed("utt1") == P.utt_seed("utt1") != P.utt_seed("utt2")


def test_a_mel_bank_with_an_empty_bin_is_refused_before_any_device(tmp_path):
    """8 kHz, L = 200 in a 256-point FFT: 128 FFT bins of 31.25 Hz; the low mel bins of a 200-bin bank are narrower than that.
    Kaldi asserts ("You may have set --num-mel-bins too large"); the option error comes before the device is looked for."""
    P = H.pkg()
    wave = [np.zeros(4000, np.int16)]
    for kw in (dict(num_mel_bins=200), dict(num_mel_bins=200, num_ceps=150), dict(num_mel_bins=100000, num_ceps=1),
               dict(num_mel_bins=60, low_freq=3000.0, high_freq=3100.0)):
        with pytest.raises(P.XvError, match="You may have set --num-mel-bins too large") as e:
            P.mfcc(wave, dither=0.0, **dict(CONF, **kw))
        assert e.value.status == P.XV_ERR_ARG and "no HIP device" not in str(e.value), kw
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="")
    r = _run([os.path.join(BIN, "compute-mfcc-feats"), "--sample-frequency=8000", "--num-mel-bins=200", "scp:x", "ark:y"], env=env)
    assert r.returncode == 255 and b"You may have set --num-mel-bins too large" in r.stderr, r.stderr.decode()[-400:]
    # the largest banks the issue's sweep uses are accepted: the refusal is of empty bins, not of large banks
    for kw in (dict(num_mel_bins=40, num_ceps=40), dict(sample_frequency=16000.0, num_mel_bins=80, num_ceps=70, high_freq=0.0)):
        assert P.mfcc_num_frames(8000, **dict(CONF, **kw)) > 0
        r = _run([os.path.join(BIN, "compute-mfcc-feats"), "--sample-frequency=%g" % dict(CONF, **kw)["sample_frequency"],
                  "--num-mel-bins=%d" % kw["num_mel_bins"], "--num-ceps=%d" % kw["num_ceps"]], env=env)
        assert r.returncode == 1 and b"Usage" in r.stderr, r.stderr.decode()[-400:]


def test_wave_read(tmp_path):
    P = H.pkg()
    rng = np.random.default_rng(0)
    mono = rng.integers(-30000, 30000, 1234).astype(np.int16)
    (tmp_path / "mono.wav").write_bytes(riff(mono))
    rate, x = P.read_wave(str(tmp_path / "mono.wav"))
    assert rate == 8000 and x.dtype == np.int16 and (x == mono).all()
    stereo = rng.integers(-30000, 30000, (500, 2)).astype(np.int16)
    (tmp_path / "st.wav").write_bytes(riff(stereo, rate=16000, channels=2))
    for ch, col in ((-1, 0), (0, 0), (1, 1)):
        rate, x = P.read_wave(str(tmp_path / "st.wav"), channel=ch)
        assert rate == 16000 and (x == stereo[:, col]).all()
    with pytest.raises(P.XvError, match="2 channels but you specified channel 2"):
        P.read_wave(str(tmp_path / "st.wav"), channel=2)
    # extra chunks in front of the data, one of odd length (padded to even)
    extra = b"LIST" + struct.pack("<I", 10) + b"INFOabcdef" + b"fact" + struct.pack("<I", 3) + b"xyz\0"
    (tmp_path / "extra.wav").write_bytes(riff(mono, extra=extra))
    assert (P.read_wave(str(tmp_path / "extra.wav"))[1] == mono).all()
    # a writer that could not seek: data size 0 / 0xFFFFFFFF, through a pipe; a size larger than what follows
    for i, size in enumerate((0, 0xFFFFFFFF, 10 * len(mono))):
        (tmp_path / ("open%d.wav" % i)).write_bytes(riff(mono, data_size=size, riff_size=0 if size != 10 * len(mono) else None))
        rate, x = P.read_wave("cat %s/open%d.wav |" % (tmp_path, i))
        assert rate == 8000 and (x == mono).all(), size
        assert (P.read_wave("%s/open%d.wav" % (tmp_path, i))[1] == mono).all()
    blob = riff(mono)
    (tmp_path / "odd.wav").write_bytes(blob[:len(blob) - 1])          # half a sample at the end is dropped
    assert (P.read_wave(str(tmp_path / "odd.wav"))[1] == mono[:-1]).all()
    for name, data, msg in (("cut.wav", blob[:30], "input ends inside"), ("nodata.wav", blob[:36], "no data chunk"),
                            ("bits8.wav", riff(np.arange(100) % 256, bits=8), "only 16-bit PCM"),
                            ("notriff.wav", b"NIST_1A\n" + bytes(100), "not a RIFF/WAVE")):
        (tmp_path / name).write_bytes(data)
        with pytest.raises(P.XvError, match=msg) as e:
            P.read_wave(str(tmp_path / name))
        assert e.value.status == P.XV_ERR_IO
    with pytest.raises(P.XvError, match="cannot open"):
        P.read_wave(str(tmp_path / "nosuch.wav"))


def test_tools_fail_early_with_exit_255(tmp_path):
    mfcc, vad = os.path.join(BIN, "compute-mfcc-feats"), os.path.join(BIN, "compute-vad")
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="")    # no device is needed for any of these
    cases = [
        ([mfcc, "--no-such-option=1", "scp:x", "ark:y"], b"Invalid option --no-such-option=1"),
        ([mfcc, "--vtln-map=ark:m", "scp:x", "ark:y"], b"VTLN is not built"),
        ([mfcc, "--vtln-warp=1.1", "scp:x", "ark:y"], b"VTLN is not built"),
        ([mfcc, "--htk-compat=true", "scp:x", "ark:y"], b"HTK-compatible features are not built"),
        ([mfcc, "--output-format=htk", "scp:x", "ark:y"], b"only Kaldi tables are written"),
        ([mfcc, "--allow-downsample=true", "scp:x", "ark:y"], b"no resampling"),
        ([mfcc, "--allow-upsample=true", "scp:x", "ark:y"], b"no resampling"),
        ([mfcc, "--round-to-power-of-two=false", "scp:x", "ark:y"], b"power-of-two"),
        ([mfcc, "--config=%s/nosuch.conf" % tmp_path, "scp:x", "ark:y"], b"cannot open"),
        ([mfcc, "--num-ceps=30", "scp:x", "ark:y"], b"num-ceps must be in"),
        ([mfcc, "--window-type=kaiser", "scp:x", "ark:y"], b"Invalid window type"),
        ([mfcc, "--dither=abc", "scp:x", "ark:y"], b"Invalid floating-point option"),
        ([vad, "--vad-energy-treshold=5", "scp:x", "ark:y"], b"Invalid option --vad-energy-treshold=5"),
        ([vad, "--config=%s/nosuch.conf" % tmp_path, "scp:x", "ark:y"], b"cannot open"),
    ]
    for args, msg in cases:
        r = _run(args, env=env)
        assert r.returncode == 255 and msg in r.stderr, (args, r.returncode, r.stderr.decode()[-400:])
    # accepted and harmless: the values that ask for nothing
    (tmp_path / "ok.conf").write_text("# a comment\n\n--sample-frequency=8000 \n--frame-length=25 # the default is 25\n"
                                      "--vtln-warp=1.0\n--htk-compat=false\n--output-format=kaldi\n--num-ceps=23 # more\n--snip-edges=false\n")
    r = _run([mfcc, "--config=%s/ok.conf" % tmp_path], env=env)
    assert r.returncode == 1 and b"Usage: compute-mfcc-feats" in r.stderr          # options fine, arguments missing
    (tmp_path / "bad.conf").write_text("--num-ceps=23\nnum-mel-bins 23\n")
    r = _run([mfcc, "--config=%s/bad.conf" % tmp_path, "scp:x", "ark:y"], env=env)
    assert r.returncode == 255 and b"should be of the form --x=y" in r.stderr
    # the command line wins over the config file: 30 ceps from the file would be refused, 13 on the command line is fine
    (tmp_path / "c30.conf").write_text("--num-ceps=30\n")
    r = _run([mfcc, "--config=%s/c30.conf" % tmp_path, "--num-ceps=13"], env=env)
    assert r.returncode == 1 and b"Usage" in r.stderr
    r = _run([mfcc, "--num-ceps=13", "--config=%s/c30.conf" % tmp_path], env=env)    # wherever --config stands
    assert r.returncode == 1 and b"Usage" in r.stderr


def test_copy_feats_writes_num_frames(tmp_path):
    from oracle import kaldi_io as kio
    utts = [("a", H.features(1, 7)), ("b", H.features(2, 120)), ("c", np.zeros((0, 23), np.float32))]
    kio.write_ark_matrices(str(tmp_path / "in.ark"), utts)
    r = _run([os.path.join(BIN, "copy-feats"), "--write-num-frames=ark,t:%s/utt2num_frames" % tmp_path, "--compress=true",
              "ark:%s/in.ark" % tmp_path, "ark,scp:%s/out.ark,%s/out.scp" % (tmp_path, tmp_path)])
    assert r.returncode == 0, r.stderr.decode()
    # (Kaldi's text form of an int32 carries a trailing space: "a 7 \n"; utils read it by fields)
    assert [l.split() for l in open(tmp_path / "utt2num_frames").read().splitlines()] == [["a", "7"], ["b", "120"], ["c", "0"]]
    got = dict(kio.read_scp(str(tmp_path / "out.scp"), "matrix"))
    assert [got[k].shape[0] for k in "abc"] == [7, 120, 0] and (got["b"] == utts[1][1]).all()
