"""Host side of the augmentation stage, no GPU: the recogniser of wav-reverberate lines (xv_recognize_wav_pipeline) on generated
wav.scp entries of every shape the augmentation scripts write and on near misses that must not be taken; the wave writer
against the wave reader; and the command line of wav-reverberate (usage, --help, refused and unknown options) by exit code
and message."""
import os
import subprocess

import numpy as np

import helpers as H
import reverb_ref as R

BIN = os.path.join(H.ROOT, H.PKG_NAME, "bin")
TOOL = os.path.join(BIN, "wav-reverberate")


def _run(args, **kw):
    return subprocess.run(args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120, **kw)


def test_wave_write_then_read_round_trip(tmp_path):
    P = H.pkg()
    x = R.speechlike(1, 5000)
    path = str(tmp_path / "a.wav")
    assert P.write_wave(path, x, 8000) == 0
    rate, y = P.read_wave(path)
    assert rate == 8000 and np.array_equal(x, y)
    raw = open(path, "rb").read()
    assert raw[:4] == b"RIFF" and raw[8:16] == b"WAVEfmt " and len(raw) == 44 + 2 * len(x)
    assert int.from_bytes(raw[4:8], "little") == len(raw) - 8 and int.from_bytes(raw[40:44], "little") == 2 * len(x)


def test_wave_write_truncates_and_saturates(tmp_path):
    P = H.pkg()
    v = np.array([0.9, -0.9, 1.5, -1.5, 32767.9, 32768.0, -32768.9, -32769.0, 1e9, -1e9], np.float32)
    path = str(tmp_path / "s.wav")
    assert P.write_wave(path, v, 16000) == 4
    rate, y = P.read_wave(path)
    want, clipped = R.quantize(v)
    assert rate == 16000 and clipped == 4 and y.tolist() == want.tolist()


def test_wave_write_to_a_command_and_empty_signal(tmp_path):
    P = H.pkg()
    x = R.speechlike(2, 777)
    path = str(tmp_path / "piped.wav")
    assert P.write_wave("| cat > %s" % path, x, 8000) == 0
    rate, y = P.read_wave("cat %s |" % path)
    assert rate == 8000 and np.array_equal(x, y)
    empty = str(tmp_path / "e.wav")
    assert P.write_wave(empty, np.zeros(0, np.float32), 8000) == 0
    assert os.path.getsize(empty) == 44


def test_defaults_and_output_length():
    P = H.pkg()
    o = P.reverb_options()
    assert (o.shift_output, o.normalize_output, o.duration, o.volume) == (1, 1, 0.0, 0.0)
    assert (o.input_wave_channel, o.rir_channel, o.noise_channel) == (0, 0, 0)
    for n, L in ((8000, 0), (8000, 1), (8000, 4000), (1, 16001)):
        for kw in (dict(), dict(shift_output=0), dict(duration=0.25), dict(duration=7.5, shift_output=0)):
            want = R.output_length(n, L, 8000.0, bool(kw.get("shift_output", 1)), kw.get("duration", 0.0))
            assert P.reverb_output_length(n, L, 8000.0, **kw) == want, (n, L, kw)


def test_usage_help_and_option_errors(tmp_path):
    r = _run([TOOL])
    assert r.returncode == 1 and b"Usage:  wav-reverberate [options...] <wav-in-rxfilename> <wav-out-wxfilename>" in r.stderr
    r = _run([TOOL, "only-one"])
    assert r.returncode == 1 and b"Usage:" in r.stderr
    r = _run([TOOL, "--help"])
    assert r.returncode == 0 and b"--impulse-response" in r.stderr and b"--shift-output" in r.stderr
    r = _run([TOOL, "--no-such-option=1", "a.wav", "b.wav"])
    assert r.returncode == 255 and b"Invalid option --no-such-option=1" in r.stderr
    r = _run([TOOL, "--multi-channel-output=true", "a.wav", "b.wav"])
    assert r.returncode == 255 and b"--multi-channel-output=true is not supported" in r.stderr
    r = _run([TOOL, "--shift-output=maybe", "a.wav", "b.wav"])
    assert r.returncode == 255 and b"Invalid format for boolean argument --shift-output=maybe" in r.stderr
    (tmp_path / "r.conf").write_text("--duration=2.5 # seconds\n--bogus=1\n")
    r = _run([TOOL, "--config=%s" % (tmp_path / "r.conf"), "a.wav", "b.wav"])
    assert r.returncode == 255 and b"Invalid option --bogus=1" in r.stderr
    r = _run([TOOL, "--print-args=false", "--verbose=1", str(tmp_path / "nosuch.wav"), str(tmp_path / "o.wav")])
    assert r.returncode == 255 and b"ERROR (wav-reverberate)" in r.stderr and not (tmp_path / "o.wav").exists()


# ---- the recogniser.  Shapes: steps/data/reverberate_data_dir.py:366 (source pipe, --impulse-response="... |"), :291-294 (plus
# additive signals), :220-232 and :273-275 (nested noise with --impulse-response / --duration); augment_data_dir_new.py:86-116.
RIR = 'sox /rirs/small room/Room001-00001.wav -r 8000 -t wav - |'


def test_recogniser_takes_reverberation_of_a_pipe_source_with_double_quotes():
    P = H.pkg()
    line = 'sph2pipe -f wav -p -c 1 /corpus/a.sph | wav-reverberate --shift-output=true --impulse-response="%s" - - |' % RIR
    d = P.recognize_wav_pipeline(line)
    assert d is not None
    assert d["source"] == "sph2pipe -f wav -p -c 1 /corpus/a.sph |" and d["impulse-response"] == RIR
    assert d["shift-output"] == "1" and d["normalize-output"] == "1" and float(d["duration"]) == 0 and float(d["volume"]) == 0
    assert not any(k.startswith("additive") for k in d)
    d2 = P.recognize_wav_pipeline("cat /a.wav | sox -t wav - -t wav - | /opt/bin/wav-reverberate --impulse-response=/r.wav --normalize-output=false --volume=0.5 --rir-channel=1 - -  |  ")
    assert d2["source"] == "cat /a.wav | sox -t wav - -t wav - |" and d2["impulse-response"] == "/r.wav"
    assert d2["normalize-output"] == "0" and float(d2["volume"]) == 0.5 and d2["channels"] == "0,1,0"


def test_recogniser_takes_a_file_source_and_single_quoted_lists_with_spaces_and_pipes():
    P = H.pkg()
    line = ("wav-reverberate --shift-output=true --additive-signals='/musan/noise/n 1.wav,sox /musan/n2.wav -r 8000 -t wav - |' "
            "--start-times='0,17.8' --snrs='15,5.5' /data/utt.wav - |")
    d = P.recognize_wav_pipeline(line)
    assert d["source"] == "/data/utt.wav" and d["impulse-response"] == ""
    assert d["additive[0].rx"] == "/musan/noise/n 1.wav" and d["additive[1].rx"] == "sox /musan/n2.wav -r 8000 -t wav - |"
    assert (float(d["additive[0].snr"]), float(d["additive[1].snr"])) == (15.0, 5.5)
    assert float(d["additive[0].start"]) == 0 and abs(float(d["additive[1].start"]) - 17.8) < 1e-6


def test_recogniser_takes_one_level_of_nesting_with_and_without_an_impulse_response():
    P = H.pkg()
    line = ("cat /data/utt.wav | wav-reverberate --shift-output=true --impulse-response=\"%s\" "
            "--additive-signals='/musan/music/m.wav wav-reverberate --duration=12.5 - - |,"
            "wav-reverberate --impulse-response=\"sox /rirs/iso.wav -r 8000 -t wav - |\" --duration=3 /noises/n.wav - |,"
            "cat /n3.wav | wav-reverberate --impulse-response=/rirs/p.wav - - |' --start-times='0,1.5,2' --snrs='15,10,5' - - |" % RIR)
    line = line.replace("/musan/music/m.wav wav-reverberate", "cat /musan/music/m.wav | wav-reverberate")
    d = P.recognize_wav_pipeline(line)
    assert d is not None and d["impulse-response"] == RIR and d["source"] == "cat /data/utt.wav |"
    assert d["additive[0].source"] == "cat /musan/music/m.wav |" and float(d["additive[0].duration"]) == 12.5 and d["additive[0].impulse-response"] == ""
    assert d["additive[1].source"] == "/noises/n.wav" and d["additive[1].impulse-response"] == "sox /rirs/iso.wav -r 8000 -t wav - |"
    assert float(d["additive[1].duration"]) == 3 and float(d["additive[1].snr"]) == 10 and float(d["additive[1].start"]) == 1.5
    assert d["additive[2].source"] == "cat /n3.wav |" and d["additive[2].impulse-response"] == "/rirs/p.wav" and float(d["additive[2].duration"]) == 0
    # the MUSAN form: '<noise file> wav-reverberate --duration=D - - |' is written with the file as a source stage
    d = P.recognize_wav_pipeline("wav-reverberate --additive-signals='wav-reverberate --duration=7 /musan/n.wav - |' --start-times='0' --snrs='15' /u.wav - |")
    assert d["additive[0].source"] == "/musan/n.wav" and float(d["additive[0].duration"]) == 7


def test_recogniser_keeps_unequal_list_lengths_for_the_tools_own_error():
    P = H.pkg()
    d = P.recognize_wav_pipeline("wav-reverberate --additive-signals='/a.wav,/b.wav' --start-times='0' --snrs='1,2' /u.wav - |")
    assert d is not None and d["additive[0].count-mismatch"] == "2, 2, 1"


NEAR_MISSES = {
    "unknown option": "cat /a.wav | wav-reverberate --impulse-response=/r.wav --foo=1 - - |",
    "verbose": "cat /a.wav | wav-reverberate --verbose=1 --impulse-response=/r.wav - - |",
    "multi-channel-output": "cat /a.wav | wav-reverberate --multi-channel-output=true --impulse-response=/r.wav - - |",
    "multi-channel-output false": "cat /a.wav | wav-reverberate --multi-channel-output=false --impulse-response=/r.wav - - |",
    "a stage after the tool": "cat /a.wav | wav-reverberate --impulse-response=/r.wav - - | sox -t wav - -t wav - |",
    "two levels of nesting": ("wav-reverberate --additive-signals='wav-reverberate --additive-signals=\"wav-reverberate --duration=1 /n.wav - |\" "
                              "--snrs=1 --start-times=0 --duration=2 /m.wav - |' --snrs=3 --start-times=0 /u.wav - |"),
    "nested with another option": "wav-reverberate --additive-signals='wav-reverberate --duration=2 --volume=1 /m.wav - |' --snrs=3 --start-times=0 /u.wav - |",
    "nested tool behind a stage": "wav-reverberate --additive-signals='wav-reverberate --duration=2 /m.wav - | sox - -t wav - |' --snrs=3 --start-times=0 /u.wav - |",
    "unbalanced double quote": 'cat /a.wav | wav-reverberate --impulse-response="sox /r.wav -t wav - | - - |',
    "unbalanced single quote": "wav-reverberate --additive-signals='/n.wav --snrs=1 --start-times=0 /u.wav - |",
    "writes a file": "cat /a.wav | wav-reverberate --impulse-response=/r.wav - /tmp/out.wav |",
    "not a pipe": "wav-reverberate --impulse-response=/r.wav /a.wav -",
    "reads stdin without a source": "wav-reverberate --impulse-response=/r.wav - - |",
    "a file and a source": "cat /a.wav | wav-reverberate --impulse-response=/r.wav /b.wav - |",
    "three positionals": "wav-reverberate --impulse-response=/r.wav /a.wav /b.wav - |",
    "a variable": "cat /a.wav | wav-reverberate --impulse-response=$RIR - - |",
    "a command substitution": "cat /a.wav | wav-reverberate --impulse-response=`ls` - - |",
    "a redirection": "cat /a.wav | wav-reverberate --impulse-response=/r.wav - - 2>/dev/null |",
    "a bad number": "cat /a.wav | wav-reverberate --duration=long - - |",
    "another tool": "cat /a.wav | wav-copy - - |",
    "the tool before the tool": "cat /a.wav | wav-reverberate --volume=2 - - | wav-reverberate --impulse-response=/r.wav - - |",
    "a plain file": "/data/a.wav",
    "a plain pipe": "sph2pipe -f wav /a.sph |",
}


def test_recogniser_leaves_near_misses_to_the_shell():
    P = H.pkg()
    for name, line in NEAR_MISSES.items():
        assert P.recognize_wav_pipeline(line) is None, name
