"""CPU tests of the host half of the compressor and of stage 3's tools: object sizes through the C ABI, the table writer's
compressed entries, copy-feats without the XVEC_COMPRESS switch (no device), the refusals, and select-voiced-frames."""
import os
import subprocess

import numpy as np
import pytest

import compress_ref as C
import helpers as H
from oracle import kaldi_io as kio

BIN = os.path.join(H.ROOT, H.PKG_NAME, "bin")
NO_GPU = dict(os.environ, HIP_VISIBLE_DEVICES="")
NO_GPU.pop("XVEC_COMPRESS", None)


def _run(args, **kw):
    return subprocess.run(args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120, **kw)


def test_compressed_size_equals_the_restatement():
    P = H.pkg()
    for method in (1, 2, 3, 5):
        for rows in (0, 1, 3, 4, 5, 8, 9, 10, 64, 65, 257, 1000, 4099):
            for cols in (0, 1, 23, 24, 130):
                assert P.compressed_size(rows, cols, method) == C.compressed_size(rows, cols, method), (method, rows, cols)
    for bad in (0, 4, 6, 7, 8):
        with pytest.raises(P.XvError):
            P.compressed_size(10, 23, bad)


def test_compressed_objects_round_trip_through_copy_feats(tmp_path):
    """"key \\0B<token> <object>" as TableWriter::WriteCompressed lays it out, read by the tool's own reader: CM in, FM out, and
    the floats are the ones the independent Python reader decodes."""
    rng = np.random.default_rng(4)
    mats = {"a": rng.standard_normal((57, 23)).astype(np.float32), "b": rng.standard_normal((8, 23)).astype(np.float32),
            "c": rng.standard_normal((3, 5)).astype(np.float32)}
    src = tmp_path / "cm.ark"
    with open(src, "wb") as f:
        for i, (k, m) in enumerate(mats.items()):
            f.write(k.encode() + b" ")
            C.write_object(f, *C.compress(m, (1, 1, 5)[i]))
    want = dict(kio.read_ark(str(src), "matrix"))
    r = _run([os.path.join(BIN, "copy-feats"), "ark:%s" % src, "ark:%s/fm.ark" % tmp_path], env=NO_GPU)
    assert r.returncode == 0, r.stderr.decode()
    got = dict(kio.read_ark("%s/fm.ark" % tmp_path, "matrix"))
    assert list(got) == ["a", "b", "c"]
    for k in mats:
        # the Python reader decodes in float64, the tool in float32 as Kaldi does: a few ulp of the largest value apart
        assert np.abs(got[k] - want[k]).max() <= 4 * np.spacing(np.float32(np.abs(mats[k]).max())), k
        assert np.abs(got[k] - mats[k]).max() < 0.05


def test_without_the_switch_compress_is_ignored_and_no_device_is_touched(tmp_path):
    m = np.random.default_rng(1).standard_normal((30, 23)).astype(np.float32)
    kio.write_ark_matrices(str(tmp_path / "in.ark"), [("u1", m), ("u2", m[:9] * 2)])
    exe = os.path.join(BIN, "copy-feats")
    a = _run([exe, "ark:%s/in.ark" % tmp_path, "ark:%s/plain.ark" % tmp_path], env=NO_GPU)
    b = _run([exe, "--compress=true", "--compression-method=2", "ark:%s/in.ark" % tmp_path, "ark:%s/opt.ark" % tmp_path], env=NO_GPU)
    c = _run([exe, "--compress=true", "--compression-method=7", "ark:%s/in.ark" % tmp_path, "ark:%s/opt7.ark" % tmp_path], env=NO_GPU)
    assert a.returncode == b.returncode == c.returncode == 0, (a.stderr, b.stderr, c.stderr)
    plain = (tmp_path / "plain.ark").read_bytes()
    assert plain == (tmp_path / "opt.ark").read_bytes() == (tmp_path / "opt7.ark").read_bytes()
    assert b"--compress=true ignored" in b.stderr and b"compressed 0 matrices" in b.stderr and b"Copied 2 feature matrices" in b.stderr
    assert b"--compress" not in a.stderr
    # a text table ignores --compress even under the switch (and needs no device for it)
    t = _run([exe, "--compress=true", "ark:%s/in.ark" % tmp_path, "ark,t:%s/t.txt" % tmp_path], env=dict(NO_GPU, XVEC_COMPRESS="1"))
    assert t.returncode == 0 and b"--compress=true ignored (a text table)" in t.stderr, t.stderr
    u = _run([exe, "ark:%s/in.ark" % tmp_path, "ark,t:%s/u.txt" % tmp_path], env=NO_GPU)
    assert u.returncode == 0 and (tmp_path / "t.txt").read_bytes() == (tmp_path / "u.txt").read_bytes()


def test_refusals(tmp_path):
    m = np.random.default_rng(2).standard_normal((30, 23)).astype(np.float32)
    kio.write_ark_matrices(str(tmp_path / "in.ark"), [("u1", m)])
    on = dict(NO_GPU, XVEC_COMPRESS="1")
    for method in (4, 6, 7):
        r = _run([os.path.join(BIN, "copy-feats"), "--compress=true", "--compression-method=%d" % method, "ark:%s/in.ark" % tmp_path,
                  "ark:%s/o.ark" % tmp_path], env=on)
        assert r.returncode == 255 and b"ERROR" in r.stderr and b"compression method %d" % method in r.stderr, r.stderr
    # under the switch, a method that is built and no GPU: an error like every tool's, not a quiet copy
    r = _run([os.path.join(BIN, "copy-feats"), "--compress=true", "ark:%s/in.ark" % tmp_path, "ark:%s/o.ark" % tmp_path], env=on)
    assert r.returncode == 255 and b"ERROR" in r.stderr and b"no HIP device" in r.stderr, r.stderr
    r = _run([os.path.join(BIN, "apply-cmvn-sliding"), "--norm-vars=true", "--center=true", "--cmn-window=300", "ark:%s/in.ark" % tmp_path,
              "ark:/dev/null"], env=NO_GPU)
    assert r.returncode == 255 and b"ERROR" in r.stderr and b"norm-vars" in r.stderr, r.stderr
    r = _run([os.path.join(BIN, "apply-cmvn-sliding"), "--norm-vars=false", "ark:%s/in.ark" % tmp_path, "ark:/dev/null"], env=NO_GPU)
    assert r.returncode == 255 and b"no HIP device" in r.stderr, r.stderr
    r = _run([os.path.join(BIN, "select-voiced-frames"), "--cmn-window=300", "ark:a", "ark:b", "ark:c"], env=NO_GPU)
    assert r.returncode == 255, r.stderr
    assert _run([os.path.join(BIN, "select-voiced-frames"), "ark:a", "ark:b"], env=NO_GPU).returncode == 1     # usage


def test_select_voiced_frames_is_a_row_gather(tmp_path):
    rng = np.random.default_rng(3)
    feats = {k: rng.standard_normal((r, 23)).astype(np.float32) for k, r in (("a", 50), ("b", 7), ("novad", 9), ("short", 12),
                                                                            ("silent", 6), ("z", 31))}
    vad = {k: (rng.random(m.shape[0]) < 0.6).astype(np.float32) for k, m in feats.items()}
    vad["a"][0] = vad["b"][3] = vad["z"][30] = 1.0
    del vad["novad"]
    vad["short"] = vad["short"][:11]
    vad["silent"][:] = 0.0
    kio.write_ark_matrices(str(tmp_path / "f.ark"), list(feats.items()))
    kio.write_ark_vectors(str(tmp_path / "v.ark"), list(vad.items()), scp_path=str(tmp_path / "v.scp"))
    r = _run([os.path.join(BIN, "select-voiced-frames"), "ark:%s/f.ark" % tmp_path, "scp,s,cs:%s/v.scp" % tmp_path,
              "ark,scp:%s/o.ark,%s/o.scp" % (tmp_path, tmp_path)], env=NO_GPU)
    err = r.stderr.decode()
    assert r.returncode == 0, err
    got = dict(kio.read_scp(str(tmp_path / "o.scp"), "matrix"))
    assert list(got) == ["a", "b", "z"]
    for k in got:
        assert got[k].astype(np.float32).tobytes() == feats[k][vad[k] != 0].tobytes(), k
    assert "No VAD input found for utterance novad" in err
    assert "Mismatch in number of frames 12 for features and VAD 11, for utterance short" in err
    assert "No features were judged as voiced for utterance silent" in err
    assert "processed 3 utterances, 3 had errors" in err
    # nothing done: exit status 1
    kio.write_ark_matrices(str(tmp_path / "g.ark"), [("silent", feats["silent"]), ("novad", feats["novad"])])
    r = _run([os.path.join(BIN, "select-voiced-frames"), "ark:%s/g.ark" % tmp_path, "ark:%s/v.ark" % tmp_path, "ark:/dev/null"], env=NO_GPU)
    assert r.returncode == 1 and b"processed 0 utterances, 2 had errors" in r.stderr, r.stderr
