#!/usr/bin/env python3
"""Generates tests/golden/cli_transcripts/cases.json: exit status, stdout and stderr of the small drop-in tools (the four
multi-tool executables behind csrc/cli.h) on command lines that end before any device call - --help, wrong argument counts,
unknown, misplaced and malformed options, --config files, refused options.  tests/test_cli_transcripts.py replays them.

The fixture is written by this project's own programs (build them first); every case runs without a device
(HIP_VISIBLE_DEVICES=-1 ROCR_VISIBLE_DEVICES=) in a scratch directory that holds FILES, so no path of this machine is recorded.
A tool's usage text is recorded once, by its --help case; elsewhere it is replaced by USAGE_MARK to keep the file small.

The case "a bare --" follows the rule of the PLDA tools: `--` alone is a positional argument.  The fixture was first recorded
from the binaries of the commit before csrc/cli.h, whose other three argument loops took it for an (unknown) option; for
those tools that one case was generated from the PLDA rule (run with another positional, `--` written in its place).  Every
other case, and this one since the tools share one loop, is recorded as the binaries give it.

    python3 tests/golden/make_cli_transcript_goldens.py"""
import json
import os
import subprocess
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
BIN = os.path.join(HERE, "..", "..", "speaker-embedding-with-phonetic-information_amd", "bin")
USAGE_MARK = "<<usage>>"

FILES = {
    "mfcc.conf": "# a comment\n\n--sample-frequency=8000 \n--frame-length=25 # the default\n--num-ceps=23\n--snip-edges=false\n",
    "c30.conf": "--num-ceps=30\n",
    "vad.conf": "--vad-energy-threshold=5.5 # as the recipe\n--vad-energy-mean-scale=0.5\n",
    "reverb.conf": "--shift-output=true\n\n--volume=0.5\n",
    "badline.conf": "--verbose=1\nnum-mel-bins 23\n",
    "unknown.conf": "--from-config=1\n",
}

B, I, F, S = "bool", "int", "float", "other"   # S: strings, and what a tool reads without checking it
COMMON_UNCHECKED = [("device", S, "0"), ("verbose", S, "1"), ("print-args", S, "false"), ("config", S, "x.conf")]
IVECTOR = [("binary", B, "false"), ("normalize", B, "true"), ("scaleup", B, "false"), ("subtract-mean", B, "true")] + COMMON_UNCHECKED
PLDA_OWN = {
    "ivector-compute-lda": [("dim", I, "50"), ("total-covariance-factor", F, "0.1"), ("covariance-floor", F, "1e-5")],
    "ivector-compute-plda": [("num-em-iters", I, "5")],
    "ivector-copy-plda": [("smoothing", F, "0.1")],
    "ivector-adapt-plda": [("mean-diff-scale", F, "1.0"), ("within-covar-scale", F, "0.3"), ("between-covar-scale", F, "0.7")],
    "ivector-plda-scoring": [("normalize-length", B, "true"), ("simple-length-normalization", B, "false"), ("num-utts", S, "ark:n")],
    "compute-eer": [],
}
MFCC = [("sample-frequency", F, "8000"), ("frame-length", F, "25"), ("frame-shift", F, "10"), ("dither", F, "0"),
        ("preemphasis-coefficient", F, "0.97"), ("remove-dc-offset", B, "true"), ("window-type", S, "hamming"),
        ("blackman-coeff", F, "0.42"), ("round-to-power-of-two", B, "true"), ("snip-edges", B, "false"), ("num-mel-bins", I, "23"),
        ("low-freq", F, "20"), ("high-freq", F, "3700"), ("num-ceps", I, "13"), ("cepstral-lifter", F, "22"), ("use-energy", B, "true"),
        ("raw-energy", B, "true"), ("energy-floor", F, "0"), ("channel", I, "0"), ("min-duration", F, "0"), ("subtract-mean", B, "false"),
        ("verbose", I, "1"), ("device", I, "0"), ("print-args", B, "false"), ("output-format", S, "kaldi"), ("vtln-warp", F, "1.0"),
        ("vtln-low", F, "100"), ("vtln-high", F, "-500"), ("htk-compat", B, "false"), ("allow-downsample", B, "false"),
        ("allow-upsample", B, "false"), ("debug-mel", B, "false")]
VAD = [("vad-energy-threshold", F, "5.5"), ("vad-energy-mean-scale", F, "0.5"), ("vad-proportion-threshold", F, "0.6"),
       ("vad-frames-context", I, "2"), ("device", S, "0"), ("verbose", S, "1"), ("print-args", S, "false")]
REVERB = [("impulse-response", S, "rir.wav"), ("additive-signals", S, "n1.wav,n2.wav"), ("snrs", S, "20,15"), ("start-times", S, "0,1.5"),
          ("shift-output", B, "true"), ("normalize-output", B, "false"), ("duration", F, "2.5"), ("volume", F, "0.5"),
          ("input-wave-channel", I, "0"), ("rir-channel", I, "0"), ("noise-channel", I, "0"), ("multi-channel-output", B, "false"),
          ("verbose", I, "1"), ("device", I, "0"), ("print-args", B, "true")]

# tool -> (its options, the largest number of positional arguments it takes)
TOOLS = {"ivector-mean": (IVECTOR, 4), "ivector-subtract-global-mean": (IVECTOR, 3), "transform-vec": (IVECTOR, 3),
         "ivector-normalize-length": (IVECTOR, 2)}
for _tool, _npos in (("ivector-compute-lda", 3), ("ivector-compute-plda", 3), ("ivector-copy-plda", 2), ("ivector-adapt-plda", 3),
                     ("ivector-plda-scoring", 5), ("compute-eer", 1)):
    TOOLS[_tool] = ([("binary", B, "true")] + PLDA_OWN[_tool] + COMMON_UNCHECKED, _npos)
TOOLS.update({"compute-mfcc-feats": (MFCC, 2), "compute-vad": (VAD, 2), "wav-reverberate": (REVERB, 2)})
READS_CONFIG = {"compute-mfcc-feats": "mfcc.conf", "compute-vad": "vad.conf", "wav-reverberate": "reverb.conf"}
OVERRIDES = {"compute-mfcc-feats": "--num-ceps=13", "compute-vad": "--vad-energy-threshold=6", "wav-reverberate": "--volume=0.25"}


def command_lines(tool):
    opts, npos = TOOLS[tool]
    yield ["--help"]
    yield []
    yield ["a%d" % i for i in range(npos + 1)]
    yield ["--no-such-option=1"]
    yield ["a%d" % i for i in range(npos)] + ["--no-such-option=1"]   # behind a positional: one more positional
    yield ["--"]
    yield ["--%s=%s" % (n, v) for n, _, v in opts]
    for n, kind, _ in opts:
        for bad in {B: ["maybe"], I: ["abc", ""], F: ["abc", ""], S: []}[kind]:
            yield ["--%s=%s" % (n, bad)]
    yield ["--device=abc"]
    if tool == "ivector-compute-plda":
        yield ["--num-em-iters=-1"]
    if tool in PLDA_OWN:
        for sibling, own in PLDA_OWN.items():
            if sibling != tool:
                for n, _, v in own:
                    yield ["--%s=%s" % (n, v)]
    if tool in READS_CONFIG:
        yield ["--config=" + READS_CONFIG[tool]]
        yield ["--config=badline.conf", "x", "y"]
        yield ["--config=nosuch.conf", "x", "y"]
        # a value the file also sets, given on the command line, wherever --config stands
        yield ["--config=" + READS_CONFIG[tool], OVERRIDES[tool]]
        yield [OVERRIDES[tool], "--config=" + READS_CONFIG[tool]]
        # the pairs of the file are applied first: its unknown option is the one that is named
        yield ["--config=unknown.conf", "--from-cli=1"]
        yield ["--from-cli=1", "--config=unknown.conf"]
    else:
        yield ["--config=nosuch.conf"]          # accepted and ignored
    if tool == "compute-mfcc-feats":
        yield ["--config=c30.conf", "--num-ceps=13"]   # 30 from the file would be refused; the command line wins
        yield ["--num-ceps=13", "--config=c30.conf"]
        yield ["--config=c30.conf"]
        for refused in ("--vtln-warp=1.1", "--htk-compat=true", "--output-format=htk", "--round-to-power-of-two=false",
                        "--allow-downsample=true", "--allow-upsample=true", "--vtln-map=ark:m", "--utt2spk=ark:u", "--window-type=kaiser"):
            yield [refused]
        yield ["--num-mel-bins=200", "--sample-frequency=8000", "scp:x", "ark:y"]   # the whole option set, before any device
        yield ["--num-mel-bins=200", "--sample-frequency=8000"]                     # ... and before the argument count
    if tool == "wav-reverberate":
        yield ["--multi-channel-output=true"]


def run(tool, args, cwd):
    env = {k: v for k, v in os.environ.items() if k != "XVEC_DEVICE"}
    env.update(HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="")
    r = subprocess.run([os.path.join(BIN, tool)] + args, cwd=cwd, env=env, stdin=subprocess.DEVNULL, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, timeout=120)
    return r.returncode, r.stdout.decode(), r.stderr.decode()


def main():
    cases = []
    with tempfile.TemporaryDirectory() as d:
        for name, text in FILES.items():
            with open(os.path.join(d, name), "w") as f:
                f.write(text)
        for tool in TOOLS:
            usage = run(tool, ["--help"], d)[2]
            assert "Usage" in usage, (tool, usage)
            seen = set()
            for args in command_lines(tool):
                if tuple(args) in seen:
                    continue
                seen.add(tuple(args))
                rc, out, err = run(tool, args, d)
                assert rc in (0, 1, 255) and "HIP" not in err and "hip" not in err, (tool, args, rc, err)
                if args != ["--help"]:
                    err = err.replace(usage, USAGE_MARK)
                case = {"tool": tool, "args": args, "rc": rc, "err": err}
                if out:
                    case["out"] = out
                cases.append(case)
    os.makedirs(os.path.join(HERE, "cli_transcripts"), exist_ok=True)
    path = os.path.join(HERE, "cli_transcripts", "cases.json")
    with open(path, "w") as f:
        json.dump({"usage_mark": USAGE_MARK, "files": FILES, "cases": cases}, f, separators=(",", ":"))
    print("wrote %d cases, %d bytes" % (len(cases), os.path.getsize(path)))


if __name__ == "__main__":
    main()
