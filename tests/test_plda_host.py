"""CPU tests of the host half of the PLDA back-end: the LDA / PLDA estimators of libxvec_hip.so (dense fp64 algebra on
the scatter statistics, through the C ABI) against tests/plda_ref.py, and the two host-only tools, ivector-copy-plda and
compute-eer (egs/sre/v2/run_sre10.sh:243, :252).  No GPU is needed for any of it."""
import os
import subprocess

import numpy as np
import pytest

import helpers as H
import plda_ref as R

BIN = os.path.join(H.ROOT, H.PKG_NAME, "bin")


def _run(args, **kw):
    return subprocess.run(args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120, **kw)


def _data(seed, n_spk, dim, lo=2, hi=9):
    rng = np.random.default_rng(seed)
    a = np.linalg.qr(rng.standard_normal((dim, dim)))[0]
    lb = a @ np.diag(np.sqrt(np.geomspace(30.0, 0.3, dim)))
    rows, segs = [], []
    for _ in range(n_spk):
        y = lb @ rng.standard_normal(dim) + 1.0
        k = int(rng.integers(lo, hi + 1))
        segs.append(list(range(len(rows), len(rows) + k)))
        rows.extend(y + rng.standard_normal((k, dim)) * np.linspace(0.5, 1.5, dim))
    return np.array(rows, np.float32), segs


def _align_rows(a, b):
    """b with every row's sign chosen to match a (eigenvector signs are free)."""
    s = np.sign((a * b).sum(1))
    s[s == 0] = 1
    return b * s[:, None]


def test_lda_estimator_matches_the_restatement():
    P = H.pkg()
    x, segs = _data(1, 120, 40)
    mean = R.global_mean(x)
    xc = (x - mean).astype(np.float32)
    s_tot, _, s_bet = R.scatter_stats(xc, segs)
    for f in (0.0, 0.1):
        got = P.lda_estimate(s_tot, s_bet, len(x), mean, 25, total_covariance_factor=f)
        spk = np.empty(len(x), np.int64)
        for k, s in enumerate(segs):
            spk[s] = k
        ref = R.lda(x, spk, 25, total_covariance_factor=f)
        assert got.shape == ref.shape == (25, 41) and got.dtype == np.float32
        np.testing.assert_allclose(_align_rows(ref, got), ref, rtol=1e-5, atol=1e-5 * np.abs(ref).max())
    with pytest.raises(P.XvError, match="LDA dimension 41 is out of range for input dimension 40"):
        P.lda_estimate(s_tot, s_bet, len(x), mean, 41)


def test_plda_estimator_matches_the_restatement():
    P = H.pkg()
    x, segs = _data(2, 300, 24)
    s_tot, sums, s_bet = R.scatter_stats(x, segs)
    counts = [len(s) for s in segs]
    mean, t, psi = P.plda_estimate(sums, counts, s_tot, s_bet)
    rmean, rt, rpsi, _, _ = R.plda_em(sums, counts, s_tot, s_bet)
    np.testing.assert_allclose(mean, rmean, rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(psi, rpsi, rtol=1e-9)
    np.testing.assert_allclose(_align_rows(rt, t), rt, rtol=1e-7, atol=1e-9 * np.abs(rt).max())
    assert np.all(np.diff(psi) <= 0) and psi.min() >= 0
    with pytest.raises(P.XvError):
        P.plda_estimate(sums, [0] + counts[1:], s_tot, s_bet)


def _model(dim=6, seed=4):
    rng = np.random.default_rng(seed)
    return rng.standard_normal(dim), np.linalg.qr(rng.standard_normal((dim, dim)))[0] * 0.7, np.sort(rng.uniform(0, 5, dim))[::-1]


def test_copy_plda_round_trips_and_smooths(tmp_path):
    mean, t, psi = _model()
    R.write_plda(str(tmp_path / "plda"), mean, t, psi)
    r = _run([os.path.join(BIN, "ivector-copy-plda"), "--binary=false", str(tmp_path / "plda"), str(tmp_path / "plda.txt")])
    assert r.returncode == 0, r.stderr.decode()
    assert (tmp_path / "plda.txt").read_bytes().startswith(b"<Plda>  [ ")
    r = _run([os.path.join(BIN, "ivector-copy-plda"), str(tmp_path / "plda.txt"), str(tmp_path / "plda2")])
    assert r.returncode == 0, r.stderr.decode()
    assert (tmp_path / "plda2").read_bytes() == (tmp_path / "plda").read_bytes()       # text keeps every bit of a double
    # float vectors are accepted; smoothing as Plda::SmoothWithinClassCovariance
    R.write_plda(str(tmp_path / "pldaf"), mean, t, psi, double=False)
    r = _run(["bash", "-c", "%s --smoothing=0.1 %s - | cat > %s" % (os.path.join(BIN, "ivector-copy-plda"), tmp_path / "pldaf",
                                                                   tmp_path / "smooth")])
    assert r.returncode == 0, r.stderr.decode()
    assert b"Smoothing within-class covariance by 0.1" in r.stderr
    m2, t2, p2 = R.read_plda(str(tmp_path / "smooth"))
    rt, rp = R.smooth(t.astype(np.float32).astype(np.float64), psi.astype(np.float32).astype(np.float64), 0.1)
    np.testing.assert_array_equal(m2, mean.astype(np.float32))
    np.testing.assert_allclose(t2, rt, rtol=1e-14)
    np.testing.assert_allclose(p2, rp, rtol=1e-14)


def test_copy_plda_input_errors(tmp_path):
    mean, t, psi = _model()
    R.write_plda(str(tmp_path / "plda"), mean, t, psi)
    whole = (tmp_path / "plda").read_bytes()
    (tmp_path / "cut").write_bytes(whole[:len(whole) // 2])
    r = _run([os.path.join(BIN, "ivector-copy-plda"), str(tmp_path / "cut"), str(tmp_path / "out")])
    assert r.returncode == 255 and b"ERROR (ivector-copy-plda)" in r.stderr
    r = _run([os.path.join(BIN, "ivector-copy-plda"), str(tmp_path / "plda")])
    assert r.returncode == 1 and b"Usage: ivector-copy-plda" in r.stderr
    r = _run([os.path.join(BIN, "ivector-copy-plda"), "--smoothing=x", str(tmp_path / "plda"), str(tmp_path / "out")])
    assert r.returncode == 255 and b"Invalid value for option" in r.stderr


def _eer_tool(text):
    return _run([os.path.join(BIN, "compute-eer"), "-"], input=text.encode())


def test_compute_eer_prints_the_restatement():
    rng = np.random.default_rng(3)
    tgt = rng.normal(2.0, 1.0, 500).astype(np.float32)
    non = rng.normal(-1.0, 1.5, 3000).astype(np.float32)
    lines = ["%.6g target" % s for s in tgt] + ["%.6g\tnontarget" % s for s in non]
    rng.shuffle(lines)
    r = _eer_tool("\n".join(lines) + "\n")
    assert r.returncode == 0, r.stderr.decode()
    e, thr = R.eer([float("%.6g" % s) for s in tgt], [float("%.6g" % s) for s in non])
    assert r.stdout.decode() == "%.4g\n" % (100.0 * e)
    assert ("Equal error rate is %g%%, at threshold %g" % (100.0 * e, thr)).encode() in r.stderr
    assert 5 < 100 * e < 25


@pytest.mark.parametrize("text,msg", [
    ("1.0 target\n2.0 target\n", b"No non-target scores seen."),
    ("1.0 nontarget\n", b"No target scores seen."),
    ("", b"Empty input."),
    ("1.0 target\n0.5 impostor\n", b"second field must be 'target' or 'nontarget'"),
    ("1.0 target extra\n", b"must have two fields"),
    ("x target\n1 nontarget\n", b"first field must be float"),
])
def test_compute_eer_errors(text, msg):
    r = _eer_tool(text)
    assert r.returncode == 255 and msg in r.stderr, r.stderr
    assert r.stdout == b""
