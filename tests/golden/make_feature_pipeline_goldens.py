#!/usr/bin/env python3
"""Generates tests/golden/feature_pipelines/cases.json: the feature rspecifier every extraction script of the reference builds
(`feats="ark:apply-cmvn-sliding ... |"` under egs/sre/v2/sid/nnet3*/), with its shell variables filled in the way
tests/test_host_logic.py::test_the_reference_feature_pipeline_is_recognised_as_text_and_nothing_else_is expects them.

Reads the reference's scripts from the tree given on the command line; the fixture holds only the resulting rspecifier strings
(the argument nnet3-xvector-compute receives) and the script each came from.

    python3 tests/golden/make_feature_pipeline_goldens.py <reference tree>"""
import glob
import json
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
# shell variable -> the value the test's assertions are written for
FILL = (("${sdata}", "data/x/split4/1"), ("$sdata", "data/x/split4/1"), ("$norm_vars", "false"), ("$center", "true"),
        ("$cmn_window", "300"))


def main():
    ref = sys.argv[1]
    root = os.path.join(ref, "egs/sre/v2/sid")
    cases = []
    for f in sorted(glob.glob(root + "/nnet3*/**/*.sh", recursive=True)):
        for m in re.finditer(r'feats?="(ark:apply-cmvn-sliding[^"]*)"', open(f).read()):
            s = m.group(1)
            for var, val in FILL:
                s = s.replace(var, val)
            cases.append({"source": os.path.relpath(f, ref), "rspecifier": s})
    out = os.path.join(HERE, "feature_pipelines", "cases.json")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    json.dump(cases, open(out, "w"), indent=1)
    print("wrote %d cases" % len(cases))


if __name__ == "__main__":
    main()
