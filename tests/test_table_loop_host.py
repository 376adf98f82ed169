"""The host side of the x-vector table loop without a GPU: its threading primitives (csrc/stage_pipeline.h) and its batch source
(csrc/batch_source.h) as stand-alone programs under ThreadSanitizer and under AddressSanitizer + UBSan.

`make sanitize-pipeline` builds and runs stage_pipeline_selftest_main.cc both ways and builds host_selftest under
ThreadSanitizer; `make sanitize` builds host_selftest under AddressSanitizer + UBSan.  `host_selftest batches` prints the
batches the source delivers; they are compared with a restatement of the batching rule."""
import os
import subprocess

import numpy as np
import pytest

import helpers as H
from oracle import kaldi_io as kio

CSRC = os.path.join(H.ROOT, H.PKG_NAME, "csrc")
REPORTS = ("ThreadSanitizer", "AddressSanitizer", "runtime error")


@pytest.fixture(scope="module")
def programs():
    r = subprocess.run(["make", "-C", CSRC, "sanitize-pipeline", "sanitize"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=1500)
    return r


def test_make_sanitize_pipeline_passes(programs):
    out = programs.stdout
    assert programs.returncode == 0, out[-3000:]
    assert out.count("stage_pipeline selftest: ok") == 2, out[-3000:]
    for word in REPORTS:
        assert word not in out, out[-3000:]


def _fnv(chunks):
    h = 1469598103934665603
    for c in chunks:
        for byte in c.tobytes():
            h = ((h ^ byte) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return "%016x" % h


def _expected(utts, max_rows=16, max_utts=4):
    """The batching rule: an utterance closes the open batch when it would take it past 16 rows or the batch holds 4."""
    out, cur = [], []
    for k, x in utts:
        if cur and (sum(y.shape[0] for _, y in cur) + x.shape[0] > max_rows or len(cur) >= max_utts):
            out.append(cur)
            cur = []
        cur.append((k, x))
    out.append(cur)   # the table ends with the open batch, empty or not
    return ["batch\t%s\t%s" % (",".join("%s:%dx%d" % (k, x.shape[0], x.shape[1]) for k, x in b), _fnv([x for _, x in b])) for b in out]


def _batches(exe, rspec, readers, views):
    r = subprocess.run([os.path.join(CSRC, "build", exe), "batches", rspec, str(readers), str(views)], stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    for word in REPORTS:
        assert word not in r.stderr, r.stderr[-3000:]
    lines = r.stdout.splitlines()
    return [l for l in lines if l.startswith("batch")], dict(l.split("\t", 1) for l in lines if not l.startswith("batch")), r.stderr


def _table(tmp_path, n=23):
    rng = np.random.default_rng(5)
    utts = [("u%02d" % i, rng.standard_normal((1 + i % 9, 3)).astype(np.float32)) for i in range(n)]
    kio.write_ark_matrices(str(tmp_path / "f.ark"), utts, scp_path=str(tmp_path / "f.scp"))
    return utts


@pytest.mark.parametrize("exe", ["host_selftest_asan", "host_selftest_tsan"])
def test_batch_source_same_partition_and_data_on_every_path(programs, tmp_path, exe):
    assert programs.returncode == 0, programs.stdout[-3000:]
    utts = _table(tmp_path)
    want = _expected(utts)
    want[-1] += "\tlast"
    assert len(want) == 8   # rows 1..9 cycling: [1 2 3 4] [5 6] [7 8] [9 1 2 3] [4 5 6] [7 8] [9 1 2 3] [4 5]
    for rspec in ("ark:%s/f.ark" % tmp_path, "scp:%s/f.scp" % tmp_path, "ark:cat %s/f.ark |" % tmp_path):
        for readers in (1, 2, 5, 16):
            for views in (1, 0):
                got, tail, err = _batches(exe, rspec, readers, views)
                assert got == want, (rspec, readers, views, got)
                assert tail["addressable"] == ("0" if readers == 1 or "|" in rspec else "1")
                assert (tail["fail_read"], tail["status"], tail["error"]) == ("0", "0", "") and err == "", (rspec, readers, tail, err)


@pytest.mark.parametrize("exe", ["host_selftest_asan", "host_selftest_tsan"])
def test_batch_source_bad_inputs(programs, tmp_path, exe):
    """What the loop did with these inputs before the source was a unit of its own, per path (read off the loop's code: the
    stream reader drops its open batch at a damaged object and ends with an empty one; the index pass ends the table at what it
    cannot index and the readers still deliver the open batch; a bad script entry is a warning and a count on both paths)."""
    assert programs.returncode == 0, programs.stdout[-3000:]
    utts = _table(tmp_path)
    # a script file whose 12th entry names a file that is not there
    lines = (tmp_path / "f.scp").read_text().splitlines()
    lines[11] = "u11 %s/nowhere.ark:7" % tmp_path
    (tmp_path / "hole.scp").write_text("\n".join(lines) + "\n")
    want = _expected(utts[:11] + utts[12:])
    want[-1] += "\tlast"
    for readers in (1, 3):
        got, tail, err = _batches(exe, "scp:%s/hole.scp" % tmp_path, readers, 1)
        assert got == want, (readers, got)
        assert tail["fail_read"] == "1" and tail["error"] == "", tail
        assert err.count("WARNING failed to read features for u11") == 1 and err.count("WARNING") == 1, err
    # an archive cut inside its 12th object (u11: 3 rows; the batch it would have entered holds u08, u09, u10)
    blob = (tmp_path / "f.ark").read_bytes()
    at = blob.index(b"u11 ") + 4 + 15 + 10
    (tmp_path / "cut.ark").write_bytes(blob[:at])
    whole = _expected(utts)
    got, tail, err = _batches(exe, "ark:%s/cut.ark" % tmp_path, 1, 1)
    assert got == whole[:3] + ["batch\t\t%s\tlast" % _fnv([])], got   # the stream reader: three batches, then the end
    assert tail["error"] != "" and tail["fail_read"] == "0", tail
    got, tail, err = _batches(exe, "ark:%s/cut.ark" % tmp_path, 4, 1)
    assert got == whole[:3] + [_expected(utts[8:11])[0] + "\tlast"], got   # the index pass: the open batch is delivered too
    assert tail["error"] != "" and tail["fail_read"] == "0", tail
    # an empty table: one empty, last batch on both paths
    (tmp_path / "empty.ark").write_bytes(b"")
    for readers in (1, 4):
        got, tail, err = _batches(exe, "ark:%s/empty.ark" % tmp_path, readers, 1)
        assert got == ["batch\t\t%s\tlast" % _fnv([])] and tail["error"] == "" and tail["fail_read"] == "0", (readers, got, tail)
