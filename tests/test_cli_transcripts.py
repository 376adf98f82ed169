"""Replays tests/golden/cli_transcripts/*.json (tests/golden/make_cli_transcript_goldens.py): the command lines of the
small drop-in tools that end before any device call - --help, wrong argument counts, unknown, misplaced and malformed
options, --config files, refused options - give the recorded exit status, stdout and stderr, byte for byte.  No GPU is
needed or looked for: the same result with or without one.  A case with "argv0" runs the tool's executable through a
symlink of that name; its stderr is recorded in full."""
import json
import os
import re
import subprocess
from concurrent.futures import ThreadPoolExecutor

import pytest

import helpers as H

BIN = os.path.join(H.ROOT, H.PKG_NAME, "bin")
FIXTURES = os.path.join(H.ROOT, "tests", "golden", "cli_transcripts")
TOOLS = ["ivector-mean", "ivector-subtract-global-mean", "transform-vec", "ivector-normalize-length", "ivector-compute-lda",
         "ivector-compute-plda", "ivector-copy-plda", "ivector-adapt-plda", "ivector-plda-scoring", "compute-eer",
         "compute-mfcc-feats", "compute-vad", "wav-reverberate"]
# the other fixture files: one per executable, by the tools it dispatches to; foreign_argv0: the executables of cases.json
MORE_TOOLS = {
    "foreign_argv0": ["ivector-mean", "ivector-compute-lda", "compute-mfcc-feats", "wav-reverberate"],
    "cmvn": ["apply-cmvn-sliding", "select-voiced-frames", "compute-cmvn-stats", "apply-cmvn"],
    "ubm": ["add-deltas", "fgmm-global-to-gmm", "gmm-gselect", "fgmm-global-gselect-to-post", "scale-post", "fgmm-global-copy",
            "gmm-global-copy", "copy-gselect"],
    "ivex": ["ivector-extract", "ivector-extractor-copy"],
    "ubm_train": ["fgmm-global-acc-stats", "gmm-global-to-fgmm", "subsample-feats", "fgmm-global-sum-accs", "fgmm-global-est"],
    "dubm_train": ["gmm-global-acc-stats", "gmm-global-init-from-feats", "gmm-global-sum-accs", "gmm-global-est"],
    "ivex_train": ["ivector-extractor-acc-stats", "ivector-extractor-init", "ivector-extractor-sum-accs", "ivector-extractor-est"],
    "post": ["logprob-to-post", "fgmm-global-acc-stats-post", "fgmm-global-init-from-accs", "nnet3-info"],
    "gmm_classify": ["fgmm-gselect", "fgmm-global-get-frame-likes", "compute-vad-from-frame-likes", "merge-vads", "fgmm-global-info"],
}


def _line_numbers(text):
    """Log lines name their source line, which moves with every edit: ':123)' at the end of a prefix becomes ':N)'."""
    return re.sub(r"(?m)^((?:LOG|WARNING|ERROR) \([^ ()]+\[[^\]]*\]:main\(\):[^ :()]+):\d+\)", r"\1:N)", text)


def _replay(name, tools, tmp_path):
    fixture = json.load(open(os.path.join(FIXTURES, name + ".json")))
    cases = fixture["cases"]
    assert sorted({c["tool"] for c in cases}) == sorted(tools)
    for fname, text in fixture["files"].items():
        (tmp_path / fname).write_text(text)
    env = {k: v for k, v in os.environ.items() if k != "XVEC_DEVICE"}
    env.update(HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="")
    own = [c for c in cases if "argv0" not in c]
    usage = {c["tool"]: c["err"] for c in own if c["args"] == ["--help"]}   # recorded in full by the --help case
    assert sorted(usage) == sorted({c["tool"] for c in own}) and all("Usage" in u for u in usage.values())
    for c in cases:   # one symlink per foreign name and executable, made before the threads start
        if "argv0" in c and not os.path.lexists(str(tmp_path / c["tool"] / c["argv0"])):
            os.makedirs(str(tmp_path / c["tool"]), exist_ok=True)
            os.symlink(os.path.join(BIN, c["tool"]), str(tmp_path / c["tool"] / c["argv0"]))

    def run(c):
        program = str(tmp_path / c["tool"] / c["argv0"]) if "argv0" in c else os.path.join(BIN, c["tool"])
        return subprocess.run([program] + c["args"], cwd=str(tmp_path), env=env, stdin=subprocess.DEVNULL,
                              stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)

    with ThreadPoolExecutor(8) as pool:
        results = list(pool.map(run, cases))
    wrong = []
    for c, r in zip(cases, results):
        want = (c["rc"], c.get("out", ""), _line_numbers(c["err"].replace(fixture["usage_mark"], usage.get(c["tool"], ""))))
        got = (r.returncode, r.stdout.decode(), _line_numbers(r.stderr.decode()))
        if got != want:
            wrong.append((c["tool"], c.get("argv0"), c["args"], got, want))
    assert not wrong, "%s: %d of %d cases differ; the first: %r" % (name, len(wrong), len(cases), wrong[0])


def test_early_exits_match_the_recorded_transcript(tmp_path):
    _replay("cases", TOOLS, tmp_path)


@pytest.mark.parametrize("name", sorted(MORE_TOOLS))
def test_early_exits_of_the_later_executables_match_the_recorded_transcript(name, tmp_path):
    _replay(name, MORE_TOOLS[name], tmp_path)
