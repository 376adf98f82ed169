"""What the table readers of csrc/kio.cc deliver, pinned byte for byte.

tests/golden/table_readers/ holds small tables of every kind (matrix, vector, double-matrix, Gaussian-selection, posterior,
int32, float, token and token-list; archives, pipes, script files with every sort of entry), the list of (reader, rspecifier)
pairs to read them through, and the dump `host_selftest tables` printed when the fixture was recorded: one line per event -
key, dimensions and a hash of the value's bytes, the indexer's entry, a pipe's exit status, or the text of the error.  The
program is the stand-alone one `make sanitize` builds under AddressSanitizer + UBSan, so a reader that delivers the right bytes
through a wild access fails here as well.  tests/golden/make_table_reader_goldens.py regenerates the fixture."""
import os
import subprocess

import helpers as H

CSRC = os.path.join(H.ROOT, H.PKG_NAME, "csrc")
EXE = os.path.join(CSRC, "build", "host_selftest_asan")
FIXTURE = os.path.join(H.ROOT, "tests", "golden", "table_readers")


def test_table_readers_deliver_the_recorded_dump():
    r = subprocess.run(["make", "-C", CSRC, "sanitize"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and os.path.exists(EXE), r.stdout[-2000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([EXE, "tables", FIXTURE], stdin=subprocess.DEVNULL, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env,
                       timeout=120)
    assert r.returncode == 0 and not r.stderr, r.stderr.decode(errors="replace")[-3000:]
    with open(os.path.join(FIXTURE, "expected.txt"), "rb") as f:
        want = f.read()
    if r.stdout != want:
        got_lines, want_lines = r.stdout.split(b"\n"), want.split(b"\n")
        diff = [(i + 1, w, g) for i, (w, g) in enumerate(zip(want_lines, got_lines)) if w != g][:10]
        assert False, "%d lines recorded, %d delivered; first differences (line, recorded, delivered): %r" % (
            len(want_lines), len(got_lines), diff)
