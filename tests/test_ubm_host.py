"""The host tools of the GMM-UBM stage (fgmm-global-to-gmm, scale-post) and the file formats behind them, run as binaries on
files written by the restatement (tests/ubm_ref.py).  No device is opened."""
import os
import struct
import subprocess

import numpy as np
import pytest

import helpers as H
import ubm_ref as R

BIN = os.path.join(H.ROOT, H.PKG_NAME, "bin")
U = 2.0 ** -24


def run(args, stdin=None, shell=False):
    env = dict(os.environ, PATH=BIN + os.pathsep + os.environ.get("PATH", ""), HIP_VISIBLE_DEVICES="")
    if not shell:
        args = [os.path.join(BIN, args[0])] + list(args[1:])
    return subprocess.run(args, input=stdin, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, shell=shell, timeout=120)


MODEL = R.random_full_model(5, 7, 6)


def check_diag(data, binary):
    """the tool's diagonal model against the restatement's.  Both invert in fp64 a matrix of condition number below 8 (Sigma =
    A A' / D + I with D x D Gaussian A has eigenvalues in [1, 8)), so the two fp64 results agree to about D * 8 * 2^-53 and each
    is then rounded to float32 once: they differ by at most one unit in the last place, 2^-23 relative (text: %.9g is exact)."""
    w, means, b, ic = MODEL
    got = R.read_diag_gmm(data)
    assert (data[:2] == b"\0B") == binary
    gc, mi, iv = R.fgmm_to_gmm(w, b, ic)
    assert np.array_equal(got["weights"], w)
    for name, want in (("gconsts", gc), ("means_invvars", mi), ("inv_vars", iv)):
        assert got[name].shape == want.shape
        assert np.all(np.abs(got[name] - want) <= 2 * U * np.abs(want)), name
    # and the means come back
    np.testing.assert_allclose(got["means_invvars"] / got["inv_vars"], means, rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize("binary_in", [True, False])
@pytest.mark.parametrize("binary_out", [True, False])
def test_fgmm_global_to_gmm_on_files(tmp_path, binary_in, binary_out):
    w, _, b, ic = MODEL
    src, dst = tmp_path / "final.ubm", tmp_path / "final.dubm"
    # stored gconsts that are wrong on purpose: they are recomputed after the read
    src.write_bytes(R.full_gmm_bytes(w, b, ic, binary_in, gconsts=np.full(len(w), 123.0)))
    r = run(["fgmm-global-to-gmm", "--binary=%s" % str(binary_out).lower(), str(src), str(dst)])
    assert r.returncode == 0, r.stderr
    assert b"LOG (fgmm-global-to-gmm" in r.stderr and b"Written diagonal GMM to" in r.stderr
    check_diag(dst.read_bytes(), binary_out)


def test_fgmm_global_to_gmm_through_standard_streams_and_a_pipe(tmp_path):
    w, _, b, ic = MODEL
    src = tmp_path / "final.ubm"
    src.write_bytes(R.full_gmm_bytes(w, b, ic, True))   # no <GCONSTS> at all
    r = run(["fgmm-global-to-gmm", "-", "-"], stdin=src.read_bytes())
    assert r.returncode == 0, r.stderr
    check_diag(r.stdout, True)
    r = run(["fgmm-global-to-gmm", "--binary=false", "cat %s |" % src, "-"])
    assert r.returncode == 0, r.stderr
    check_diag(r.stdout, False)
    # the recipe's model argument, as a shell sees it
    r = run('fgmm-global-to-gmm %s - | cat' % src, shell=True)
    assert r.returncode == 0, r.stderr
    check_diag(r.stdout, True)


def test_a_model_written_byte_by_byte_is_read(tmp_path):
    """G = 2, D = 2, laid down with struct.pack from the format as the issue states it, not with our writers: diagonal inverse
    covariances [[2, 0], [0, 4]] and [[1, 0], [0, 1]], Sigma^-1 mu = (2, 4) and (0, 1), weights 1/4 and 3/4."""
    f32 = lambda *v: struct.pack("<%df" % len(v), *v)
    i32 = lambda v: b"\x04" + struct.pack("<i", v)
    data = (b"\0B<FullGMM> <WEIGHTS> FV " + i32(2) + f32(0.25, 0.75) + b"<MEANS_INVCOVARS> FM " + i32(2) + i32(2) + f32(2, 4, 0, 1)
            + b"<INV_COVARS> FP " + i32(2) + f32(2, 0, 4) + b"FP " + i32(2) + f32(1, 0, 1) + b"</FullGMM> ")
    r = run(["fgmm-global-to-gmm", "--binary=false", "-", "-"], stdin=data)
    assert r.returncode == 0, r.stderr
    got = R.read_diag_gmm(r.stdout)
    assert got["weights"].tolist() == [0.25, 0.75]
    assert got["inv_vars"].tolist() == [[2, 4], [1, 1]]
    assert got["means_invvars"].tolist() == [[2, 4], [0, 1]]
    want = [np.log(0.25) - 0.5 * (2 * np.log(2 * np.pi) - np.log(8.0) + 2.0 + 4.0), np.log(0.75) - 0.5 * (2 * np.log(2 * np.pi) + 1.0)]
    np.testing.assert_allclose(got["gconsts"], want, rtol=2 * U)


POST = [("utt-a", [[(3, 0.75), (11, 0.25)], [(5, 1.0)], []]), ("utt-b", [[(0, 0.5), (1, 0.25), (2, 0.25)]]), ("utt-c", [[(9, 1.0)]])]


@pytest.mark.parametrize("binary_in", [True, False])
@pytest.mark.parametrize("scale", [1.0, 0.0, 0.3])
def test_scale_post_with_one_scale(tmp_path, binary_in, scale):
    src = tmp_path / "post.ark"
    src.write_bytes(R.post_table_bytes(POST, binary_in))
    for spec, binary_out in (("ark:%s", True), ("ark,t:%s", False)):
        dst = tmp_path / ("out_%d" % binary_out)
        r = run(["scale-post", "ark:%s" % src, repr(scale), spec % dst])
        assert r.returncode == 0, r.stderr
        assert b"Done 3 posteriors;  0 had no scales." in r.stderr
        got = R.read_post_table(dst.read_bytes())
        want = [(k, R.scale_post(p, scale)) for k, p in POST]
        if binary_out:
            assert got == want
            if scale == 1.0 and binary_in:
                assert dst.read_bytes() == src.read_bytes()   # reader and writer agree on every byte
        else:
            assert [k for k, _ in got] == [k for k, _ in want]
            for (_, g), (_, w) in zip(got, want):
                assert [[i for i, _ in f] for f in g] == [[i for i, _ in f] for f in w]
                np.testing.assert_allclose([p for f in g for _, p in f], [p for f in w for _, p in f], rtol=1e-7)


def test_scale_post_with_a_table_of_scales_and_through_pipes(tmp_path):
    src, scales = tmp_path / "post.ark", tmp_path / "scales.ark"
    src.write_bytes(R.post_table_bytes(POST, True))
    scales.write_bytes(b"utt-a 0.5\nutt-c \0B\x04" + struct.pack("<f", 2.0))
    r = run('cat %s | scale-post ark:- ark:%s ark:- | scale-post ark:- 1.0 ark,t:-' % (src, scales), shell=True)
    assert r.returncode == 0, r.stderr
    assert b"No scale available for key utt-b" in r.stderr and b"Done 2 posteriors;  1 had no scales." in r.stderr
    got = R.read_post_table(r.stdout)
    assert got == [("utt-a", R.scale_post(POST[0][1], 0.5)), ("utt-c", R.scale_post(POST[2][1], 2.0))]


def test_a_posterior_written_byte_by_byte_is_read(tmp_path):
    i32 = lambda v: b"\x04" + struct.pack("<i", v)
    f32 = lambda v: b"\x04" + struct.pack("<f", v)
    data = b"k1 \0B" + i32(2) + i32(2) + i32(7) + f32(0.5) + i32(8) + f32(0.5) + i32(0) + b"k2 \0B" + i32(1) + i32(1) + i32(4) + f32(1.0)
    r = run(["scale-post", "ark:-", "2", "ark,t:-"], stdin=data)
    assert r.returncode == 0, r.stderr
    assert r.stdout == b"k1 [ 7 1 8 1 ] [ ] \nk2 [ 4 2 ] \n"


def test_errors_are_worded_and_end_with_the_tools_statuses(tmp_path):
    w, _, b, ic = MODEL
    good = R.full_gmm_bytes(w, b, ic, True)
    r = run(["fgmm-global-to-gmm", "-", "-"], stdin=good[:len(good) // 2])
    assert r.returncode == 255 and b"ERROR (fgmm-global-to-gmm" in r.stderr and r.stdout == b""
    r = run(["fgmm-global-to-gmm", "-", "-"], stdin=R.diag_gmm_bytes(w, b, np.abs(b) + 1))
    assert r.returncode == 255 and b"expected token <FullGMM>, got <DiagGMM>" in r.stderr
    r = run(["fgmm-global-to-gmm", "-", "-"], stdin=good.replace(b"<INV_COVARS>", b"<INV_COVARZ>"))
    assert r.returncode == 255 and b"expected token <INV_COVARS>, got <INV_COVARZ>" in r.stderr
    r = run(["fgmm-global-to-gmm", "only-one"])
    assert r.returncode == 1 and b"Usage: fgmm-global-to-gmm" in r.stderr
    r = run(["scale-post", "ark:-", "1.0"])
    assert r.returncode == 1 and b"Usage: scale-post" in r.stderr
    r = run(["scale-post", "ark:-", "fast", "ark:-"], stdin=b"")
    assert r.returncode == 255 and b"Bad scale 'fast'" in r.stderr
    post = R.post_table_bytes(POST, True)
    r = run(["scale-post", "ark:-", "1.0", "ark:/dev/null"], stdin=post[:-3])
    assert r.returncode == 255 and b"ERROR (scale-post" in r.stderr
    # a covariance that is not positive definite cannot be inverted
    bad = ic.copy()
    bad[0, 0] = -1.0
    r = run(["fgmm-global-to-gmm", "-", "-"], stdin=R.full_gmm_bytes(w, b, bad, True))
    assert r.returncode == 255 and b"not positive definite" in r.stderr
    # the device tools refuse what is not built before they open anything
    r = run(["gmm-gselect", "--write-likes=ark:/dev/null", "a", "b", "c"])
    assert r.returncode == 255 and b"--write-likes is not built" in r.stderr
    r = run(["gmm-gselect", "--gselect=ark:x", "a", "b", "c"])
    assert r.returncode == 255 and b"--gselect is not built" in r.stderr


def test_the_c_abi_converts_like_the_tool():
    w, _, b, ic = MODEL
    P = H.pkg()
    gc, mi, iv = P.fgmm_to_gmm(w, b, ic)
    want = R.fgmm_to_gmm(w, b, ic)
    for got, ref in zip((gc, mi, iv), want):
        assert np.all(np.abs(got - ref) <= 2 * U * np.abs(ref))


# ------------------------------------------------------------------------------------------------- every format, both ways
def test_full_and_diagonal_models_round_trip_through_the_copies(tmp_path):
    """binary -> C++ reader -> text writer -> C++ reader -> binary writer gives the bytes of binary -> binary: %.9g names a float32
    exactly, and the gconsts are recomputed from the same values on every read."""
    w, _, b, ic = MODEL
    src = tmp_path / "final.ubm"
    src.write_bytes(R.full_gmm_bytes(w, b, ic, True))
    for tool, first in (("fgmm-global-copy", str(src)), ("gmm-global-copy", "fgmm-global-to-gmm %s - |" % src)):
        a, t, c = (str(tmp_path / (tool + e)) for e in (".bin", ".txt", ".bin2"))
        for args in (["--binary=true", first, a], ["--binary=false", a, t], [t, c]):
            r = run([tool] + args)
            assert r.returncode == 0, r.stderr
        assert open(a, "rb").read() == open(c, "rb").read() and open(a, "rb").read()[:2] == b"\0B"
        assert open(t, "rb").read()[:1] == b"<"
    full = R.read_full_gmm(open(str(tmp_path / "fgmm-global-copy.txt"), "rb").read())
    assert np.array_equal(full["inv_covars"], ic) and np.array_equal(full["means_invcovars"], b) and np.array_equal(full["weights"], w)
    np.testing.assert_allclose(full["gconsts"], R.full_gconsts(w, b, ic), rtol=2 * U)
    assert np.array_equal(full["gconsts"], H.pkg().fgmm_gconsts(w, b, ic))
    check_diag(open(str(tmp_path / "gmm-global-copy.txt"), "rb").read(), False)
    # the restatement's own text, and old-style tokens
    r = run(["fgmm-global-copy", "--binary=false", "-", "-"], stdin=R.full_gmm_bytes(w, b, ic, False).replace(b"<FullGMM>", b"<FullGMMBegin>")
            .replace(b"</FullGMM>", b"<FullGMMEnd>"))
    assert r.returncode == 0, r.stderr
    assert np.array_equal(R.read_full_gmm(r.stdout)["inv_covars"], ic)


def test_a_diagonal_model_written_byte_by_byte_is_read():
    f32 = lambda *v: struct.pack("<%df" % len(v), *v)
    i32 = lambda v: b"\x04" + struct.pack("<i", v)
    data = (b"\0B<DiagGMM> <GCONSTS> FV " + i32(2) + f32(99, 99) + b"<WEIGHTS> FV " + i32(2) + f32(0.5, 0.5) + b"<MEANS_INVVARS> FM " + i32(2) + i32(2)
            + f32(1, 2, 3, 4) + b"<INV_VARS> FM " + i32(2) + i32(2) + f32(1, 2, 4, 8) + b"</DiagGMM> ")
    r = run(["gmm-global-copy", "--binary=false", "-", "-"], stdin=data)
    assert r.returncode == 0, r.stderr
    got = R.read_diag_gmm(r.stdout)
    assert got["means_invvars"].tolist() == [[1, 2], [3, 4]] and got["inv_vars"].tolist() == [[1, 2], [4, 8]]
    np.testing.assert_allclose(got["gconsts"], R.diag_gconsts([0.5, 0.5], [[1, 2], [3, 4]], [[1, 2], [4, 8]]), rtol=2 * U)
    r = run(["gmm-global-copy", "-", "-"], stdin=data[:-20])
    assert r.returncode == 255 and b"ERROR (gmm-global-copy" in r.stderr


def test_the_gselect_table_round_trips_and_is_read_byte_by_byte(tmp_path):
    sel = [("utt-a", [[5, 3, 9], [1, 2, 3]]), ("utt-b", [[7, 7, 7]]), ("utt-c", [])]
    src = tmp_path / "gs.ark"
    src.write_bytes(R.gselect_table_bytes(sel, True))
    r = run(["copy-gselect", "ark:%s" % src, "ark,t:-"])
    assert r.returncode == 0, r.stderr
    assert r.stdout == b"utt-a 5 3 9 ; 1 2 3 ; \nutt-b 7 7 7 ; \nutt-c \n" and b"Copied 3 gselect entries" in r.stderr
    r2 = run(["copy-gselect", "ark:-", "ark:-"], stdin=r.stdout)
    assert r2.returncode == 0 and r2.stdout == src.read_bytes()
    r3 = run(["copy-gselect", "--n=2", "ark:-", "ark,t:-"], stdin=R.gselect_table_bytes(sel, False))
    assert R.read_gselect_table(r3.stdout) == [("utt-a", [[5, 3], [1, 2]]), ("utt-b", [[7, 7]]), ("utt-c", [])]
    i32 = lambda v: b"\x04" + struct.pack("<i", v)
    raw = b"k \0B" + i32(2) + b"\x04" + struct.pack("<i3i", 3, 4, 5, 6) + b"\x04" + struct.pack("<i", 0)
    r4 = run(["copy-gselect", "ark:-", "ark,t:-"], stdin=raw)
    assert r4.returncode == 0 and r4.stdout == b"k 4 5 6 ; ; \n"
    r5 = run(["copy-gselect", "ark:-", "ark:-"], stdin=raw[:-3])
    assert r5.returncode == 255 and b"ERROR (copy-gselect" in r5.stderr


def test_script_files_and_the_permissive_option(tmp_path):
    src = tmp_path / "post.ark"
    src.write_bytes(R.post_table_bytes(POST, True))
    ark, scp = tmp_path / "out.ark", tmp_path / "out.scp"
    r = run(["scale-post", "ark:%s" % src, "1.0", "ark,scp:%s,%s" % (ark, scp)])
    assert r.returncode == 0, r.stderr
    assert ark.read_bytes() == src.read_bytes()
    lines = scp.read_text().splitlines()
    assert [l.split()[0] for l in lines] == [k for k, _ in POST] and all(l.split()[1].startswith("%s:" % ark) for l in lines)
    r = run(["scale-post", "scp:%s" % scp, "2.0", "ark:-"])
    assert r.returncode == 0 and R.read_post_table(r.stdout) == [(k, R.scale_post(p, 2.0)) for k, p in POST]
    # an entry that cannot be opened: reported and counted, or with p skipped without a word
    lines.insert(1, "utt-gone %s/nothing.ark:0" % tmp_path)
    scp.write_text("\n".join(lines) + "\n")
    r = run(["scale-post", "scp:%s" % scp, "1.0", "ark:-"])
    assert r.returncode == 0 and b"Failed to read the posterior of utt-gone" in r.stderr and b"Done 3 posteriors;  1 had no scales." in r.stderr
    assert r.stdout == src.read_bytes()
    r = run(["scale-post", "scp,p:%s" % scp, "1.0", "ark:-"])
    assert r.returncode == 0 and b"utt-gone" not in r.stderr.split(b"\n", 1)[1] and b"Done 3 posteriors;  0 had no scales." in r.stderr
    assert r.stdout == src.read_bytes()
    # the sorted options change nothing for a table that is read front to back
    r = run(["scale-post", "ark,s,cs:%s" % src, "1.0", "ark:-"])
    assert r.returncode == 0 and r.stdout == src.read_bytes()
