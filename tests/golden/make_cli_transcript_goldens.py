#!/usr/bin/env python3
"""Generates tests/golden/cli_transcripts/*.json: exit status, stdout and stderr of the small drop-in tools (the twelve
executables behind csrc/cli.h) on command lines that end before any device call - --help, wrong argument counts,
unknown, misplaced and malformed options, --config files, refused options.  tests/test_cli_transcripts.py replays them.
cases.json holds the four executables that came first (13 tools); each of the other eight has a file of its own, which adds
an option in underscore spelling, one own option of every sibling tool, and the executable under a foreign name (a symlink;
"argv0" in the case record).  foreign_argv0.json holds those foreign names for the executables of cases.json.

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

# The other eight executables.  SEED: a non-negative decimal integer (ToSeed).
SEED = "seed"
COMMON = [("verbose", S, "1"), ("print-args", S, "false"), ("config", S, "x.conf")]
DEV = ("device", I, "0")
BIN_OPT = ("binary", B, "false")
GMM_ACC = [BIN_OPT, ("update-flags", S, "mv"), ("gselect", S, "ark:g.ark"), ("verbose", I, "1"), DEV, ("print-args", S, "false"), ("config", S, "x.conf")]
DGMM_EST = [("min-gaussian-weight", F, "1e-5"), ("min-gaussian-occupancy", F, "10"), ("min-variance", F, "0.001"), ("remove-low-count-gaussians", B, "true")]
FGMM_EST = [("update-flags", S, "mvw"), ("min-gaussian-weight", F, "1e-5"), ("min-gaussian-occupancy", F, "100"), ("variance-floor", F, "0.001"),
            ("max-condition", F, "1e5")]
# file -> {tool: (its options, the positional arguments it takes (0: any number from two on), further command lines)};
# the first tool of a file is the one the Makefile links, the others are its copies
EXECUTABLES = {
    "cmvn": {
        "apply-cmvn-sliding": ([("norm-vars", B, "false"), ("center", B, "true"), ("cmn-window", I, "300"), ("min-cmn-window", I, "50"),
                                ("device", S, "0")] + COMMON, 2, [["--norm-vars=true"]]),
        "select-voiced-frames": (COMMON, 3, []),
        "compute-cmvn-stats": ([("spk2utt", S, "ark:s2u"), BIN_OPT, DEV] + COMMON, 2, [["--weights=ark:w.ark"]]),
        "apply-cmvn": ([("utt2spk", S, "ark:u2s"), ("norm-means", B, "true"), ("norm-vars", B, "false"), ("reverse", B, "false"),
                        ("skip-dims", S, "0:2"), DEV] + COMMON, 3, [["--skip-dims=a:b"], ["--skip-dims="], ["--norm-vars=true"]]),
    },
    "ubm": {
        "add-deltas": ([("delta-order", I, "2"), ("delta-window", I, "2"), ("truncate", I, "0"), DEV] + COMMON, 2, []),
        "fgmm-global-to-gmm": ([BIN_OPT] + COMMON, 2, []),
        "gmm-gselect": ([("n", I, "50"), DEV] + COMMON, 3, [["--write-likes=ark:l.ark"], ["--gselect=ark:g.ark"]]),
        "fgmm-global-gselect-to-post": ([("min-post", F, "0.025"), DEV] + COMMON, 4, []),
        "scale-post": (COMMON, 3, []),
        "fgmm-global-copy": ([BIN_OPT] + COMMON, 2, []),
        "gmm-global-copy": ([BIN_OPT] + COMMON, 2, []),
        "copy-gselect": ([("n", I, "20")] + COMMON, 2, []),
    },
    "ivex": {
        "ivector-extract": ([("compute-objf-change", B, "true"), ("acoustic-weight", F, "0.5"), ("max-count", F, "100"), ("num-threads", S, "4"),
                             ("verbose", I, "1"), DEV, ("print-args", S, "false"), ("config", S, "x.conf")], 4, [["--spk2utt=ark:s2u"]]),
        "ivector-extractor-copy": ([BIN_OPT] + COMMON, 2, []),
    },
    "ubm_train": {
        "fgmm-global-acc-stats": (GMM_ACC, 3, [["--weights=ark:w.ark"], ["final.ubm", "scp:f.scp", "out.acc"]]),
        "gmm-global-to-fgmm": ([BIN_OPT] + COMMON, 2, []),
        "subsample-feats": ([("n", I, "2"), ("offset", I, "1")] + COMMON, 2, [["--n=0", "ark:a", "ark:b"]]),
        "fgmm-global-sum-accs": ([BIN_OPT] + COMMON, 0, [["out.acc", "nosuch.acc"]]),
        "fgmm-global-est": ([BIN_OPT] + FGMM_EST + [("remove-low-count-gaussians", B, "true"), ("mix-up", I, "0")] + COMMON, 3, [["--mix-up=1"]]),
    },
    "dubm_train": {
        "gmm-global-acc-stats": (GMM_ACC, 3, [["--weights=ark:w.ark"], ["final.dubm", "scp:f.scp", "out.acc"]]),
        "gmm-global-init-from-feats": ([BIN_OPT, ("num-gauss", I, "8"), ("num-gauss-init", I, "4"), ("num-iters", I, "2"), ("num-frames", I, "1000"),
                                        ("num-threads", I, "4")] + DGMM_EST + [("seed", SEED, "3"), DEV] + COMMON, 2, []),
        "gmm-global-sum-accs": ([BIN_OPT] + COMMON, 0, [["out.acc", "nosuch.acc"]]),
        "gmm-global-est": ([BIN_OPT, ("update-flags", S, "mvw")] + DGMM_EST + [("mix-up", I, "16"), ("perturb-factor", F, "0.01"), ("seed", SEED, "3")]
                           + COMMON, 3, []),
    },
    "ivex_train": {
        "ivector-extractor-acc-stats": ([BIN_OPT, ("update-variances", B, "true"), ("compute-auxf", B, "true"), ("verbose", I, "1"), DEV,
                                         ("num-threads", S, "4"), ("num-samples-for-weights", S, "3"), ("cache-size", S, "100"),
                                         ("print-args", S, "false"), ("config", S, "x.conf")], 4, []),
        "ivector-extractor-init": ([BIN_OPT, ("ivector-dim", I, "8"), ("seed", I, "3"), ("use-weights", B, "false")] + COMMON, 2,
                                   [["--use-weights=true"], ["--seed=-1"]]),
        "ivector-extractor-sum-accs": ([BIN_OPT, ("parallel", B, "true")] + COMMON, 0, []),
        "ivector-extractor-est": ([BIN_OPT, ("num-threads", I, "1"), ("variance-floor-factor", F, "0.1"), ("gaussian-min-count", F, "100"),
                                   ("diagonalize", B, "true")] + COMMON, 3, []),
    },
    "post": {
        "logprob-to-post": ([("min-post", F, "0.01"), ("random-prune", B, "true"), DEV] + COMMON, 2, []),
        "fgmm-global-acc-stats-post": ([BIN_OPT, ("update-flags", S, "mv"), DEV] + COMMON, 4, [["--weights=ark:w.ark"]]),
        "fgmm-global-init-from-accs": ([BIN_OPT, ("remove-low-count-gaussians", B, "true")] + FGMM_EST + [("mix-up", I, "0")] + COMMON, 3,
                                       [["--mix-up=1"], ["--update-flags=xyz"], ["--update-flags="]]),
        "nnet3-info": (COMMON, 1, []),
    },
    "gmm_classify": {
        "fgmm-gselect": ([("n", I, "20"), ("gselect", S, "ark:g.ark"), DEV] + COMMON, 3, []),
        "fgmm-global-get-frame-likes": ([("average", B, "true"), ("gselect", S, "ark:g.ark"), DEV] + COMMON, 3, []),
        "compute-vad-from-frame-likes": ([("map", S, "m.txt"), ("priors", S, "0.5,0.5")] + COMMON, 0, []),
        "merge-vads": ([("map", S, "m.txt")] + COMMON, 3, []),
        "fgmm-global-info": (COMMON, 1, []),
    },
}
FIRST = list(TOOLS)   # cases.json
for _tools in EXECUTABLES.values():
    TOOLS.update({t: v[:2] for t, v in _tools.items()})
# Names no tool has, names that merely contain a tool's, and for the ubm executable names that contain two
FOREIGN = ["zz-other"]
FOREIGN_CONTAINS = {"cmvn": ["x-select-voiced-frames.bak", "x-apply-cmvn.bak"], "ubm": ["x-gmm-gselect.bak", "fgmm-global-gselect-to-post.gmm-gselect",
                    "x-fgmm-global-copy.bak", "x-gmm-global-copy.bak"], "ivex": ["x-ivector-extractor-copy.bak"], "ubm_train": ["x-subsample-feats.bak"],
                    "dubm_train": ["x-gmm-global-est.bak"], "ivex_train": ["x-ivector-extractor-est.bak"], "post": ["x-nnet3-info.bak"],
                    "gmm_classify": ["x-merge-vads.bak", "x-fgmm-global-info.bak"]}
# ... and the executables of cases.json, by the tool the Makefile links
FOREIGN_FIRST = {"ivector-mean": ["x-transform-vec.bak"], "ivector-compute-lda": ["x-compute-eer.bak"], "compute-mfcc-feats": ["x-compute-vad.bak"],
                 "wav-reverberate": ["x-wav-reverberate.bak"]}
_COMMON_NAMES = {"verbose", "print-args", "config", "device"}


def own_options(opts):
    return [o for o in opts if o[0] not in _COMMON_NAMES]


def new_command_lines(tool, siblings):
    """What the eight later files add to command_lines(tool)."""
    opts, _, extra = siblings[tool]
    for line in extra:
        yield line
    for n, kind, _ in opts:
        if kind == SEED:
            for bad in ("abc", "", "-1"):
                yield ["--%s=%s" % (n, bad)]
    # one option in underscore spelling: the first own one that has a dash, else --print_args
    n, _, v = next((o for o in own_options(opts) if "-" in o[0]), ("print-args", S, "false"))
    yield ["--%s=%s" % (n.replace("-", "_"), v)]
    # one own option of each sibling that this tool does not have
    for sibling, (sopts, _, _) in siblings.items():
        other = [o for o in own_options(sopts) if o[0] not in {x[0] for x in opts}]
        if sibling != tool and other:
            yield ["--%s=%s" % (other[0][0], other[0][2])]


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
        for bad in {B: ["maybe"], I: ["abc", ""], F: ["abc", ""], S: [], SEED: []}[kind]:
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


def run(tool, args, cwd, argv0=None):
    env = {k: v for k, v in os.environ.items() if k != "XVEC_DEVICE"}
    env.update(HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="")
    program = os.path.join(BIN, tool)
    if argv0 is not None:   # the same executable under another name
        program = os.path.join(cwd, argv0)
        if os.path.lexists(program):
            os.remove(program)
        os.symlink(os.path.join(BIN, tool), program)
    r = subprocess.run([program] + args, cwd=cwd, env=env, stdin=subprocess.DEVNULL, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, timeout=120)
    return r.returncode, r.stdout.decode(), r.stderr.decode()


def record(tool, lines, cwd):
    """The cases of one tool; its usage is spelt out by the --help case alone."""
    usage = run(tool, ["--help"], cwd)[2]
    assert "Usage" in usage, (tool, usage)
    seen = set()
    for args in lines:
        if tuple(args) in seen:
            continue
        seen.add(tuple(args))
        rc, out, err = run(tool, args, cwd)
        assert rc in (0, 1, 255) and "HIP" not in err and "hip" not in err, (tool, args, rc, err)
        if args != ["--help"]:
            err = err.replace(usage, USAGE_MARK)
        case = {"tool": tool, "args": args, "rc": rc, "err": err}
        if out:
            case["out"] = out
        yield case


def record_foreign(tool, names, cwd):
    """--help and no arguments of `tool`'s executable under each of `names`, in full."""
    for argv0 in names:
        for args in (["--help"], []):
            rc, out, err = run(tool, args, cwd, argv0)
            assert rc in (0, 1, 255) and "HIP" not in err and "hip" not in err, (tool, argv0, args, rc, err)
            case = {"tool": tool, "argv0": argv0, "args": args, "rc": rc, "err": err}
            if out:
                case["out"] = out
            yield case


def write(name, cases):
    path = os.path.join(HERE, "cli_transcripts", name + ".json")
    with open(path, "w") as f:
        json.dump({"usage_mark": USAGE_MARK, "files": FILES, "cases": cases}, f, separators=(",", ":"))
    print("%s: wrote %d cases, %d bytes" % (name, len(cases), os.path.getsize(path)))


def main():
    os.makedirs(os.path.join(HERE, "cli_transcripts"), exist_ok=True)
    with tempfile.TemporaryDirectory() as d:
        for name, text in FILES.items():
            with open(os.path.join(d, name), "w") as f:
                f.write(text)
        write("cases", [c for tool in FIRST for c in record(tool, command_lines(tool), d)])
        write("foreign_argv0", [c for tool, names in FOREIGN_FIRST.items() for c in record_foreign(tool, FOREIGN + names, d)])
        for name, siblings in EXECUTABLES.items():
            cases = []
            for tool in siblings:
                cases += record(tool, list(command_lines(tool)) + list(new_command_lines(tool, siblings)), d)
            cases += record_foreign(next(iter(siblings)), FOREIGN + FOREIGN_CONTAINS[name], d)
            write(name, cases)


if __name__ == "__main__":
    main()
