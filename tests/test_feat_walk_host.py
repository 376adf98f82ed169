"""The host layer the table-joining tools share (csrc/feat_batch.h, keyed_lookup.h, feat_join.h), without a GPU: the walk over a
feature table in batches with its three problem policies, the keyed lookup (merged when the table promised sorted keys, loaded
otherwise), the selection and posterior joins, and the group-by-width packer.

`host_selftest walk <dir>` - the stand-alone program `make sanitize` builds under AddressSanitizer + UBSan - prints one line per
event; the expected dump is computed here from the inputs, a few lines per rule, and stderr has to hold the warnings' texts and
nothing else (so nothing from a sanitizer).  Shapes: 3 columns, 1 to 4 rows per utterance, a read-ahead of 4 frames."""
import errno
import os
import re
import subprocess

import numpy as np

import helpers as H
import ubm_ref as R
from oracle import kaldi_io as kio

CSRC = os.path.join(H.ROOT, H.PKG_NAME, "csrc")
EXE = os.path.join(CSRC, "build", "host_selftest_asan")
AHEAD, DIM = 4, 3

# (key, rows, cols) in table order; u03 has no rows, u04's file does not exist, u06 has another width between its neighbours
SHAPES = [("u01", 2, 3), ("u02", 3, 3), ("u03", 0, 3), ("u04", None, None), ("u05", 1, 3), ("u06", 2, 4), ("u07", 2, 3), ("u08", 2, 3),
          ("u09", 1, 3), ("u10", 4, 3), ("u11", 1, 3), ("u12", 1, 3)]
# Sorted by key.  u00 and u095 belong to no utterance; u05 is absent from the middle, u11 and u12 come after the last entry;
# u07 is a frame short, u08 ragged, u09 has no indices; the width changes from u01 to u02, which share a batch.
GSELECT = [("u00", [[0]]), ("u01", [[1, 0], [0, 1]]), ("u02", [[1], [0], [1]]), ("u06", [[0, 1], [1, 0]]), ("u07", [[0, 1]]),
           ("u08", [[0, 1], [0]]), ("u09", [[]]), ("u095", [[1]]), ("u10", [[0, 1], [1, 0], [0, 1], [1, 0]])]
# u01's second frame has no pairs; u05 and u11 are absent; u07 has a frame too many
POST = [("u01", [[(0, 0.75), (1, 0.25)], []]), ("u02", [[(1, 1.0)], [(0, 0.5), (1, 0.5)], [(0, 1.0)]]), ("u06", [[(0, 1.0)], [(1, 1.0)]]),
        ("u07", [[(0, 1.0)]] * 3), ("u08", [[(1, 1.0)], [(0, 0.125), (1, 0.875)]]), ("u09", [[(0, 1.0)]]), ("u10", [[(1, 1.0)]] * 4),
        ("u12", [[(0, 0.5), (1, 0.5)]])]
MISSING = "cannot open gone.ark for reading: " + os.strerror(errno.ENOENT)   # csrc/kio.cc Input::Open


def fnv(array):
    h = 1469598103934665603
    for byte in np.ascontiguousarray(array).tobytes():
        h = ((h ^ byte) * 1099511628211) % 2 ** 64
    return "%016x" % h


def join(values):
    return ",".join(str(v) for v in values)


def write_tables(d):
    rng = np.random.default_rng(7)
    feats = {k: rng.normal(size=(r, c)).astype(np.float32) for k, r, c in SHAPES if r is not None}
    offs = kio.write_ark_matrices(str(d / "feats.ark"), feats.items())
    for name, keep in (("feats.scp", lambda k: True), ("readable.scp", lambda k: k != "u04")):
        with open(d / name, "w") as f:
            for k, _, _ in SHAPES:
                if keep(k):
                    f.write("%s %s\n" % (k, "feats.ark:%d" % offs[k] if k in offs else "gone.ark:7"))
    (d / "gselect.ark").write_bytes(R.gselect_table_bytes(GSELECT))
    (d / "post.ark").write_bytes(R.post_table_bytes(POST))
    return feats


def walk(feats, keys):
    """The reader's rule, as events in the order the walk reports them: a batch holds matrices that can be read and have rows,
    of one column count, and is closed once it has AHEAD frames; what was skipped on the way to a batch is reported before it."""
    events, cur, skipped = [], [], []

    def close():
        events.extend(("problem", k) for k in skipped)
        events.append(("batch", list(cur)))
        del cur[:], skipped[:]

    for k in keys:
        if k not in feats or feats[k].shape[0] == 0:
            skipped.append(k)
            continue
        if cur and feats[cur[0]].shape[1] != feats[k].shape[1]:
            close()
        cur.append(k)
        if sum(feats[c].shape[0] for c in cur) >= AHEAD:
            close()
    if cur:
        close()
    return events + [("problem", k) for k in skipped]


def problem_text(feats, k):
    return "Empty feature matrix for utterance " + k if k in feats else "Failed to read features for key %s: %s" % (k, MISSING)


def offsets(feats, keys):
    return join(np.cumsum([0] + [len(feats[k]) for k in keys]))


def batch_line(feats, keys):
    return "batch\tkeys=%s\tcols=%d\trow_off=%s" % (join(keys), feats[keys[0]].shape[1], offsets(feats, keys))


def rows_of(feats, keys):
    return np.concatenate([feats[k].ravel() for k in keys]) if keys else np.zeros(0, np.float32)


def expect_batches(feats, keys, policy):
    """policy 0: both kinds of problem warned and counted; 1: a matrix without rows warned, not counted; 2: a matrix without
    rows ignored, one that cannot be read fatal."""
    out, err, errors = [], [], 0
    for kind, v in walk(feats, keys):
        if kind == "batch":
            out.append(batch_line(feats, v))
        elif policy == 2 and v in feats:
            pass
        elif policy == 2:
            return out + ["thrown\t" + problem_text(feats, v)], err
        else:
            err.append(problem_text(feats, v))
            errors += policy == 0 or v not in feats
    return out + ["errors\t%d" % errors], err


def check_gselect(sel, rows):
    """(outcome, size, width) of one utterance's selection against its frame count"""
    if sel is None:
        return "not-found", 0, 0
    if len(sel) != rows:
        return "wrong-size", len(sel), 0
    if len(sel[0]) < 1 or any(len(l) != len(sel[0]) for l in sel):
        return "ragged", len(sel), 0
    return "ok", len(sel), len(sel[0])


def expect_groups(feats, keys, table, num_gauss):
    """table None: the identity selection 0 .. num_gauss - 1.  A group ends where the width changes and at the end of a batch."""
    out, err, errors = [], [], 0
    for kind, v in walk(feats, keys):
        if kind == "problem":
            err.append(problem_text(feats, v))
            errors += 1
            continue
        groups = []   # [width, keys, gs]
        for k in v:
            rows, cols = feats[k].shape
            if cols != DIM:
                err.append("Dimension mismatch for utterance %s: the features have %d columns, the model %d" % (k, cols, DIM))
                errors += 1
                continue
            sel = table.get(k) if table is not None else [list(range(num_gauss))] * rows
            outcome, size, width = check_gselect(sel, rows)
            if outcome != "ok":
                err.append({"not-found": "No Gaussian-selection info available for utterance %s (skipping utterance)" % k,
                            "wrong-size": "Mismatch in number of frames %d for features and Gaussian selection %d, for utterance %s" % (rows, size, k),
                            "ragged": "The Gaussian selection of utterance %s does not have one length for every frame (skipping utterance)" % k}[outcome])
                errors += 1
                continue
            if not groups or groups[-1][0] != width:
                groups.append([width, [], []])
            groups[-1][1].append(k)
            groups[-1][2] += [i for l in sel for i in l]
        for width, gkeys, gs in groups:
            out.append("group\twidth=%d\tkeys=%s\toff=%s\tfeats=%s\tgs=%s" % (
                width, join(gkeys), offsets(feats, gkeys), fnv(rows_of(feats, gkeys)), fnv(np.array(gs, np.int32))))
    return out + ["errors\t%d" % errors], err


def expect_join_gselect(feats, keys, table):
    out, err = [], []
    for kind, v in walk(feats, keys):
        if kind == "problem":
            err.append(problem_text(feats, v))
            continue
        out.append(batch_line(feats, v))
        out += ["join\t%s\t%s\tsize=%d\twidth=%d" % ((k,) + check_gselect(table.get(k), len(feats[k]))) for k in v]
    return out, err


def expect_join_post(feats, keys, table):
    """Per batch, the accepted posteriors flattened: post_off[t + 1] - post_off[t] pairs for pending frame t."""
    out, err = [], []
    for kind, v in walk(feats, keys):
        if kind == "problem":
            err.append(problem_text(feats, v))
            continue
        out.append(batch_line(feats, v))
        off, idx, w, kept = [0], [], [], []
        for k in v:
            post = table.get(k)
            outcome = "not-found" if post is None else "ok" if len(post) == len(feats[k]) else "wrong-size"
            out.append("join\t%s\t%s\tsize=%d\twidth=0" % (k, outcome, 0 if post is None else len(post)))
            if outcome != "ok":
                continue
            kept.append(k)
            for frame in post:
                idx += [i for i, _ in frame]
                w += [p for _, p in frame]
                off.append(len(idx))
        out.append("post\tpost_off=%s\tpost_idx=%s\tpost_w=%s\tfeats=%s" % (
            join(off), fnv(np.array(idx, np.int32)), fnv(np.array(w, np.float32)), fnv(rows_of(feats, kept))))
    return out, err


def test_walk_lookup_and_joins_deliver_what_the_rules_say(tmp_path):
    r = subprocess.run(["make", "-C", CSRC, "sanitize"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and os.path.exists(EXE), r.stdout[-2000:]
    feats = write_tables(tmp_path)
    keys, readable = [k for k, _, _ in SHAPES], [k for k, _, _ in SHAPES if k != "u04"]
    gselect, post = dict(GSELECT), dict(POST)
    cases = [("batches\t%d\t%d\tscp:feats.scp" % (AHEAD, p), expect_batches(feats, keys, p)) for p in (0, 1, 2)]
    cases.append(("batches\t%d\t2\tscp:readable.scp" % AHEAD, expect_batches(feats, readable, 2)))
    for spec in ("ark,s,cs:gselect.ark", "ark:gselect.ark"):   # merged front to back, and loaded: the same events
        cases.append(("groups\t%d\t%d\t2\tscp:feats.scp\t%s" % (AHEAD, DIM, spec), expect_groups(feats, keys, gselect, 2)))
        cases.append(("join-gselect\t%d\tscp:feats.scp\t%s" % (AHEAD, spec), expect_join_gselect(feats, keys, gselect)))
    cases.append(("groups\t%d\t%d\t2\tscp:feats.scp\t-" % (AHEAD, DIM), expect_groups(feats, keys, None, 2)))
    for spec in ("ark,s,cs:post.ark", "ark:post.ark"):
        cases.append(("join-post\t%d\tscp:feats.scp\t%s" % (AHEAD, spec), expect_join_post(feats, keys, post)))
    (tmp_path / "walk_cases.txt").write_text("".join(line + "\n" for line, _ in cases))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([EXE, "walk", str(tmp_path)], stdin=subprocess.DEVNULL, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env,
                       text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]
    want_out = [l for line, (out, _) in cases for l in ["case\t" + line] + out]
    assert r.stdout.splitlines() == want_out
    # every line of stderr is one warning of the shared layer: "WARNING (<prog>[<version>]:main():<file>:<line>) <text>"
    got_err = [re.fullmatch(r"WARNING \(xvec-hip\[xvec-hip-0\.1\]:main\(\):[\w.]+:\d+\) (.*)", l) for l in r.stderr.splitlines()]
    assert all(got_err), r.stderr[-3000:]
    assert [m.group(1) for m in got_err] == [l for _, (_, err) in cases for l in err]
    # what the fixture is there for, so that a change to it cannot empty the test: the two groups of the first batch, the one
    # fatal problem, a frame without pairs and offsets that run across two utterances
    assert want_out.count("thrown\t" + problem_text(feats, "u04")) == 1
    assert sum(l.startswith("group\twidth=2\tkeys=u01\t") for l in want_out) == 2 and sum(l.startswith("group\twidth=1\tkeys=u02\t") for l in want_out) == 2
    assert sum(l.startswith("post\tpost_off=0,2,2,3,5,6\t") for l in want_out) == 2
