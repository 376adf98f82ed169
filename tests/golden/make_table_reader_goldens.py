#!/usr/bin/env python3
"""Generates tests/golden/table_readers/: small Kaldi tables of every kind the C++ table readers of csrc/kio.cc accept, the list
of (reader, rspecifier) pairs to read them through (cases.txt) and what the readers delivered when the fixture was recorded
(expected.txt: one line per event - key, dimensions and a hash of the value's bytes, or the error text).

The inputs are written with oracle/kaldi_io.py; the dump is what `host_selftest tables <dir>` prints (csrc/host_selftest_main.cc,
built by `make sanitize`).  All paths in the tables are relative to the fixture directory, which the program enters first, so
the dump does not depend on where the repository lies.  tests/test_table_readers.py replays it.

    python3 tests/golden/make_table_reader_goldens.py"""
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from oracle import kaldi_io as kio  # noqa: E402

OUT = os.path.join(HERE, "table_readers")
CSRC = os.path.join(ROOT, "speaker-embedding-with-phonetic-information_amd", "csrc")


def write_objects(path, items, write, binary=True):
    """key + object per entry; returns {key: (offset of the key, offset of the object)}."""
    offs = {}
    with open(os.path.join(OUT, path), "wb") as f:
        for key, obj in items:
            at = f.tell()
            f.write(key.encode() + b" ")
            offs[key] = (at, f.tell())
            if binary:
                f.write(b"\x00B")
            write(f, obj, binary)
    return offs


def write_text(path, text):
    with open(os.path.join(OUT, path), "wb") as f:
        f.write(text.encode())


def script(kind, ext, a, b, extra):
    """The script file every reader of matrices (kind "m") or vectors ("v") walks: each line takes another path through
    the code that turns an scp entry into an open, positioned file."""
    fa, fb, whole = "%s_a.ark" % kind, "%s_b.ark" % kind, "%s_whole.%s" % (kind, ext)
    lines = [
        "a1 %s:%d" % (fa, a["a1"][1]),            # consecutive offsets into one archive
        "a2 %s:%d" % (fa, a["a2"][1]),
        "b1 %s:%d" % (fb, b["b1"][1]),            # alternating between two archives
        "a3 %s:%d" % (fa, a["a3"][1]),
        "b2 %s:%d" % (fb, b["b2"][1]),
        "w1 %s" % whole,                          # a whole file
        "z1 %s:0" % whole,                        # offset 0 is not a seek
        "p1 cat %s |" % whole,                    # a pipe
        "p2 cat %s #:12 |" % whole,               # a trailing '|' is a pipe whatever it contains
        "miss missing.ark:5",                     # a missing file
        "empty   ",                               # an empty rxfilename
        "a3 %s:%d" % (fa, a["a3"][1]),
        "beyond %s:99999" % fb,                   # an offset beyond the end (of a file that is not the one in use)
        "colon %s:12x" % fa,                      # a suffix that is not all digits belongs to the path
        "a1 %s:%d" % (fa, a["a2"][1]),            # a duplicate key with another value: the first entry wins
    ] + extra + [
        "b1  \t%s:%d  " % (fb, b["b1"][1]),       # white space around the rxfilename
        "last %s:%d" % (fa, a["a2"][1]),          # a last line without a newline
    ]
    write_text("%s_mixed.scp" % kind, "\n".join(lines))
    write_text("%s_consecutive.scp" % kind, "".join("%s %s:%d\n" % (k, fa, a[k][1]) for k in ("a1", "a2", "a3")))


def main():
    os.makedirs(OUT, exist_ok=True)
    rng = np.random.default_rng(20181019)
    cases = []

    def case(reader, rspec, *ops):
        cases.append("\t".join((reader, rspec) + ops))

    # ------------------------------------------------------------------ matrices
    mats = [("a1", (8, 5)), ("a2", (1, 5)), ("a3", (3, 4))]
    mats = [(k, rng.standard_normal(s).astype(np.float32)) for k, s in mats]
    mats_b = [(k, rng.standard_normal(s).astype(np.float32)) for k, s in [("b1", (2, 3)), ("b2", (5, 1))]]

    def wm(f, m, binary):
        kio.write_matrix(f, m, binary)

    a = write_objects("m_a.ark", mats, wm)
    b = write_objects("m_b.ark", mats_b, wm)
    dm = write_objects("m_dm.ark", mats, lambda f, m, binary: kio.write_matrix(f, m, True, double=True))
    cm = write_objects("m_cm.ark", mats, lambda f, m, binary: kio.write_compressed_matrix(f, m, "CM"))
    tx = write_objects("m_txt.ark", mats, wm, binary=False)
    write_objects("m_mixed.ark", mats, lambda f, m, binary: (f.write(b"\x00B"), kio.write_matrix(f, m, True))
                  if m.shape[0] == 1 else kio.write_matrix(f, m, False), binary=False)
    with open(os.path.join(OUT, "m_whole.mat"), "wb") as f:
        f.write(b"\x00B")
        kio.write_matrix(f, mats[2][1], True)
    script("m", "mat", a, b, ["d1 m_dm.ark:%d" % dm["a1"][1], "c1 m_cm.ark:%d" % cm["a1"][1], "t1 m_txt.ark:%d" % tx["a3"][1]])
    # a failing entry of the archive that is in use: the sequential reader seeks in the file it holds
    write_text("m_beyond_same.scp", "a1 m_a.ark:%d\nbeyond m_a.ark:99999\na2 m_a.ark:%d\n" % (a["a1"][1], a["a2"][1]))
    m_archives = ["m_a.ark", "m_dm.ark", "m_cm.ark", "m_txt.ark", "m_mixed.ark"]
    m_tables = (["ark:" + f for f in m_archives] + ["ark:cat %s |" % f for f in m_archives] +
                ["ark:cat m_a.ark; exit 3 |", "ark:m_a.ark:%d" % a["a2"][0], "ark:missing.ark", "ark,s,cs:m_a.ark",
                 "scp:m_consecutive.scp", "scp:m_mixed.scp", "scp,p:m_mixed.scp", "scp:m_beyond_same.scp",
                 "scp:cat m_consecutive.scp |", "scp:missing.scp"])
    for t in m_tables:
        case("seq-matrix", t)
    for t in m_tables:
        case("indexed", t)

    # ------------------------------------------------------------------ vectors
    vecs = [(k, rng.standard_normal(n).astype(np.float32)) for k, n in [("a1", 8), ("a2", 1), ("a3", 5)]]
    vecs_b = [(k, rng.standard_normal(n).astype(np.float32)) for k, n in [("b1", 3), ("b2", 7)]]

    def wv(f, v, binary):
        kio.write_vector(f, v, binary)

    a = write_objects("v_a.ark", vecs, wv)
    b = write_objects("v_b.ark", vecs_b, wv)
    dv = write_objects("v_dv.ark", vecs, lambda f, v, binary: kio.write_vector(f, v, True, double=True))
    tx = write_objects("v_txt.ark", vecs, wv, binary=False)
    with open(os.path.join(OUT, "v_whole.vec"), "wb") as f:
        f.write(b"\x00B")
        kio.write_vector(f, vecs[2][1], True)
    script("v", "vec", a, b, ["d1 v_dv.ark:%d" % dv["a1"][1], "t1 v_txt.ark:%d" % tx["a3"][1]])
    v_archives = ["v_a.ark", "v_dv.ark", "v_txt.ark"]
    v_tables = (["ark:" + f for f in v_archives] + ["ark:cat %s |" % f for f in v_archives] +
                ["ark:cat v_a.ark; exit 3 |", "ark:v_a.ark:%d" % a["a2"][0], "ark:missing.ark",
                 "scp:v_consecutive.scp", "scp:v_mixed.scp", "scp,p:v_mixed.scp", "scp:cat v_consecutive.scp |", "scp:missing.scp"])
    for t in v_tables:
        case("seq-vector", t)
    # out of order, the same key twice, Forget then Value, an absent key, the failing entries, the duplicate key
    script_ops = ["value:b2", "value:a1", "value:a1", "forget:a1", "value:a1", "has:a1", "has:nokey", "value:nokey", "forget:nokey",
                  "value:last", "value:w1", "value:z1", "value:p1", "value:p2", "value:miss", "value:beyond", "value:a3", "value:colon",
                  "value:b1", "value:d1", "value:t1", "value:a2", "forget:a2", "forget:a2", "value:a2", "has:empty", "value:miss"]
    archive_ops = ["value:a3", "value:a1", "forget:a1", "value:a1", "has:a2", "has:nokey", "value:nokey"]
    case("ra-vector", "scp:v_mixed.scp", *script_ops)
    case("ra-vector", "scp,s,cs:v_consecutive.scp", "value:a1", "forget:a1", "value:a2", "forget:a2", "value:a3", "value:a1")
    for t in ["ark:v_a.ark", "ark:v_dv.ark", "ark:v_txt.ark", "ark:cat v_a.ark |"]:
        case("ra-vector", t, *archive_ops)
    case("ra-vector", "ark:missing.ark", "has:a1")
    case("ra-vector", "scp:missing.scp", "has:a1")

    # ------------------------------------------------------------------ double matrices (the readers take FM, DM and text)
    m_ops = [op for op in script_ops if not op.startswith("forget")] + ["value:c1"]
    case("ra-double-matrix", "scp:m_mixed.scp", *m_ops)
    case("ra-double-matrix", "scp:m_consecutive.scp", "value:a3", "value:a1", "value:a2", "value:a1")
    for t in ["ark:m_a.ark", "ark:m_dm.ark", "ark:m_txt.ark", "ark:cat m_dm.ark |"]:
        case("ra-double-matrix", t, "value:a3", "value:a1", "has:a2", "has:nokey", "value:nokey")
    case("ra-double-matrix", "ark:m_cm.ark", "has:a1")
    case("ra-double-matrix", "ark:missing.ark", "has:a1")

    # ------------------------------------------------------------------ Gaussian selection and posteriors
    gsel = [("g1", [[3, 1, 4], [1, 5], []]), ("g2", [[9]]), ("g3", [])]
    post = [("g1", [[(3, 0.75), (1, 0.25)], [(7, 1.0)], []]), ("g2", [[(2, 0.5)]]), ("g3", [])]

    def wg(f, v, binary):
        if binary:
            kio.write_int32(f, len(v))
            for l in v:
                f.write(b"\x04" + np.int32(len(l)).tobytes() + np.asarray(l, dtype="<i4").tobytes())
        else:
            f.write(("".join("".join("%d " % x for x in l) + "; " for l in v) + "\n").encode())

    def wp(f, p, binary):
        if binary:
            kio.write_int32(f, len(p))
            for frame in p:
                kio.write_int32(f, len(frame))
                for idx, w in frame:
                    kio.write_int32(f, idx)
                    kio.write_float(f, w)
        else:
            f.write(("".join("[ " + "".join("%d %.9g " % e for e in frame) + "] " for frame in p) + "\n").encode())

    for name, items, write, reader in [("g", gsel, wg, "seq-gselect"), ("p", post, wp, "seq-posterior")]:
        o = write_objects(name + "_bin.ark", items, write)
        t = write_objects(name + "_txt.ark", items, write, binary=False)
        write_text(name + ".scp", "g1 %s_bin.ark:%d\nmiss missing.ark:3\nempty \ng3 %s_txt.ark:%d\nbeyond %s_bin.ark:99999\ng2 %s_bin.ark:%d" %
                   (name, o["g1"][1], name, t["g3"][1], name, name, o["g2"][1]))
        for spec in ["ark:%s_bin.ark", "ark:%s_txt.ark", "ark,s,cs:%s_bin.ark", "ark:cat %s_bin.ark |", "ark:cat %s_txt.ark; exit 3 |",
                     "scp:%s.scp", "scp,p:%s.scp", "ark:missing_%s.ark"]:
            case(reader, spec % name)
    case("seq-gselect", "ark:p_bin.ark")   # the wrong kind of object

    # ------------------------------------------------------------------ scalar and token tables
    with open(os.path.join(OUT, "i_ok.ark"), "wb") as f:
        f.write(b"k1 12\nk2 -3 \nk3 \x00B")
        kio.write_int32(f, 70000)
        f.write(b"k4 \x00B")
        kio.write_int32(f, -1)
        f.write(b"k1 5\nk5 8")
    write_text("i_bad.ark", "k1 12\nk2 12x\nk3 4\n")
    write_text("i_two.ark", "k1 12 13\nk2 4\n")
    write_text("i_none.ark", "k1 12\nk2\n")
    with open(os.path.join(OUT, "f_ok.ark"), "wb") as f:
        f.write(b"k1 0.5\nk2 -3e-2 \nk3 \x00B")
        kio.write_float(f, 1.25)
        f.write(b"k4 \x00B")
        kio.write_double(f, 0.1)
        f.write(b"k1 5\nk5 inf")
    write_text("f_bad.ark", "k1 0.5\nk2 0.5.5\n")
    write_text("f_two.ark", "k1 0.5 0.25\nk2 4\n")
    for kind, stem in (("int32", "i"), ("float", "f")):
        for spec in ("ark:%s_ok.ark", "ark:cat %s_ok.ark |", "ark:%s_bad.ark", "ark:%s_two.ark", "scp:%s_ok.ark", "ark:%s_missing.ark"):
            case(kind, spec % stem)
    case("int32", "ark:i_none.ark")
    write_text("utt2spk", "u1 s1\nu2 s2\n\n  u3   s1  \nu1 s3\nu4 s4")
    write_text("spk2utt", "s1 u1 u3\ns2 u2\n\ns5\n s4\tu4  u5 u6")
    for kind in ("token", "token-list"):
        for spec in ("ark:utt2spk", "ark:spk2utt", "ark:cat utt2spk |", "scp:utt2spk", "ark:missing"):
            case(kind, spec)

    write_text("cases.txt", "".join(c + "\n" for c in cases))

    subprocess.check_call(["make", "-C", CSRC, "-s", "sanitize"])
    exe = os.path.join(CSRC, "build", "host_selftest_asan")
    r = subprocess.run([exe, "tables", OUT], stdin=subprocess.DEVNULL, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    if r.returncode != 0 or r.stderr:
        sys.exit("host_selftest tables failed (%d):\n%s" % (r.returncode, r.stderr.decode(errors="replace")[-3000:]))
    with open(os.path.join(OUT, "expected.txt"), "wb") as f:
        f.write(r.stdout)
    print("wrote %d cases, %d events" % (len(cases), r.stdout.count(b"\n")))


if __name__ == "__main__":
    main()
