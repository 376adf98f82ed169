"""Replays tests/golden/cli_transcripts/cases.json (tests/golden/make_cli_transcript_goldens.py): the command lines of the
small drop-in tools that end before any device call - --help, wrong argument counts, unknown, misplaced and malformed
options, --config files, refused options - give the recorded exit status, stdout and stderr, byte for byte.  No GPU is
needed or looked for: the same result with or without one."""
import json
import os
import re
import subprocess
from concurrent.futures import ThreadPoolExecutor

import helpers as H

BIN = os.path.join(H.ROOT, H.PKG_NAME, "bin")
FIXTURE = os.path.join(H.ROOT, "tests", "golden", "cli_transcripts", "cases.json")
TOOLS = ["ivector-mean", "ivector-subtract-global-mean", "transform-vec", "ivector-normalize-length", "ivector-compute-lda",
         "ivector-compute-plda", "ivector-copy-plda", "ivector-adapt-plda", "ivector-plda-scoring", "compute-eer",
         "compute-mfcc-feats", "compute-vad", "wav-reverberate"]


def _line_numbers(text):
    """Log lines name their source line, which moves with every edit: ':123)' at the end of a prefix becomes ':N)'."""
    return re.sub(r"(?m)^((?:LOG|WARNING|ERROR) \([^ ()]+\[[^\]]*\]:main\(\):[^ :()]+):\d+\)", r"\1:N)", text)


def test_early_exits_match_the_recorded_transcript(tmp_path):
    fixture = json.load(open(FIXTURE))
    cases = fixture["cases"]
    assert sorted({c["tool"] for c in cases}) == sorted(TOOLS)
    for name, text in fixture["files"].items():
        (tmp_path / name).write_text(text)
    env = {k: v for k, v in os.environ.items() if k != "XVEC_DEVICE"}
    env.update(HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="")
    usage = {c["tool"]: c["err"] for c in cases if c["args"] == ["--help"]}   # recorded in full by the --help case
    assert sorted(usage) == sorted(TOOLS) and all("Usage" in u for u in usage.values())

    def run(c):
        return subprocess.run([os.path.join(BIN, c["tool"])] + c["args"], cwd=str(tmp_path), env=env, stdin=subprocess.DEVNULL,
                              stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)

    with ThreadPoolExecutor(8) as pool:
        results = list(pool.map(run, cases))
    wrong = []
    for c, r in zip(cases, results):
        want = (c["rc"], c.get("out", ""), _line_numbers(c["err"].replace(fixture["usage_mark"], usage[c["tool"]])))
        got = (r.returncode, r.stdout.decode(), _line_numbers(r.stderr.decode()))
        if got != want:
            wrong.append((c["tool"], c["args"], got, want))
    assert not wrong, "%d of %d cases differ; the first: %r" % (len(wrong), len(cases), wrong[0])
