"""CPU tests of ivector-adapt-plda's host half: xv_plda_adapt (the update from the adaptation statistics, through the C
ABI) against tests/plda_adapt_ref.py, and the tool's argument and input errors, which it reports before it needs a device.
Transform rows are not compared directly: their signs and, for equal psi', their basis are not unique."""
import os
import subprocess

import numpy as np
import pytest

import helpers as H
import plda_adapt_ref as A
import plda_ref as R

BIN = os.path.join(H.ROOT, H.PKG_NAME, "bin")


def _model(rng, dim):
    mean = rng.standard_normal(dim) * 0.3
    t = np.linalg.qr(rng.standard_normal((dim, dim)))[0] * rng.uniform(0.5, 2.0, dim)[:, None]
    psi = np.sort(rng.uniform(0.05, 6.0, dim))[::-1]
    return mean, t, psi


def _adaptation_data(rng, mean, t, psi, n):
    dim = len(mean)
    tm = t / np.sqrt(1.0 + psi)[:, None]
    r = np.linalg.qr(rng.standard_normal((dim, dim)))[0]
    scale = np.sqrt(np.where(np.arange(dim) < dim // 4, 2.5, np.where(np.arange(dim) >= dim - dim // 4, 0.4, 1.0)))
    z = rng.standard_normal((n, dim)) * scale
    return (np.linalg.solve(tm, (z @ r.T).T).T + mean + 0.5 * np.linalg.solve(tm, r[:, 0])).astype(np.float32)


def _close(a, b, rtol):
    assert np.abs(a - b).max() <= rtol * np.abs(b).max(), np.abs(a - b).max() / np.abs(b).max()


@pytest.mark.parametrize("scales", [(1.0, 0.3, 0.7), (1.0, 0.75, 0.25), (0.0, 0.75, 0.25), (2.0, 0.0, 1.0)])
@pytest.mark.parametrize("dim", [8, 150])
def test_xv_plda_adapt_matches_the_restatement(dim, scales):
    P = H.pkg()
    rng = np.random.default_rng(dim)
    mean, t, psi = _model(rng, dim)
    n, m, v = A.stats(_adaptation_data(rng, mean, t, psi, 3000))
    mds, within, between = scales
    got = P.plda_adapt(n, m, v, mean, t, psi, mean_diff_scale=mds, within_covar_scale=within, between_covar_scale=between)
    ref = A.adapt(n, m, v, mean, t, psi, mean_diff_scale=mds, within_covar_scale=within, between_covar_scale=between)
    assert ref[3].max() > 1.0 and ref[3].min() < 1.0
    np.testing.assert_allclose(got[0], ref[0], rtol=1e-12, atol=1e-15)                      # the mean
    np.testing.assert_allclose(got[2], ref[2], rtol=1e-9)                                    # psi'
    np.testing.assert_allclose(got[3], ref[3], rtol=1e-9)                                    # s
    assert np.all(np.diff(got[2]) <= 0) and got[2].min() >= 0
    for a, b in zip(A.implied_covariances(got[1], got[2]), A.implied_covariances(ref[1], ref[2])):
        _close(a, b, 1e-9)


def test_defaults_are_kaldis():
    P = H.pkg()
    rng = np.random.default_rng(3)
    mean, t, psi = _model(rng, 10)
    n, m, v = A.stats(_adaptation_data(rng, mean, t, psi, 500))
    got = P.plda_adapt(n, m, v, mean, t, psi)
    ref = A.adapt(n, m, v, mean, t, psi, 1.0, 0.3, 0.7)
    np.testing.assert_allclose(got[2], ref[2], rtol=1e-9)


def test_xv_plda_adapt_argument_errors():
    P = H.pkg()
    rng = np.random.default_rng(4)
    mean, t, psi = _model(rng, 5)
    n, m, v = A.stats(_adaptation_data(rng, mean, t, psi, 100))
    with pytest.raises(P.XvError, match="bad argument"):
        P.plda_adapt(0, m, v, mean, t, psi)
    with pytest.raises(P.XvError, match="psi must not be negative"):
        P.plda_adapt(n, m, v, mean, t, np.r_[psi[:-1], -0.5])
    with pytest.raises(P.XvError, match="do not agree on dimension"):
        P.plda_adapt(n, m[:4], v, mean, t, psi)


def _run(args, **kw):
    return subprocess.run(args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120, **kw)


def test_tool_usage_and_errors_before_the_device(tmp_path):
    """Usage, bad options, an unreadable model, an empty archive and a dimension mismatch: no output file, and the exit
    codes of the other PLDA tools.  None of these reaches the device."""
    from oracle import kaldi_io as kio
    tool = os.path.join(BIN, "ivector-adapt-plda")
    rng = np.random.default_rng(5)
    mean, t, psi = _model(rng, 6)
    R.write_plda(str(tmp_path / "plda"), mean, t, psi)
    out = tmp_path / "adapted"
    r = _run([tool, str(tmp_path / "plda")])
    assert r.returncode == 1 and b"Usage: ivector-adapt-plda" in r.stderr
    r = _run([tool, "--help"])
    assert r.returncode == 0 and b"--within-covar-scale=0.3" in r.stderr
    for bad in ("--within-covar-scale=x", "--no-such-option=1", "--smoothing=0.1"):
        r = _run([tool, bad, str(tmp_path / "plda"), "ark:/dev/null", str(out)])
        assert r.returncode == 255 and b"ERROR (ivector-adapt-plda)" in r.stderr, (bad, r.stderr)
        assert not out.exists()
    (tmp_path / "empty.ark").write_bytes(b"")
    r = _run([tool, str(tmp_path / "plda"), "ark:%s" % (tmp_path / "empty.ark"), str(out)])
    assert r.returncode == 255 and b"Accumulated stats from 0 iVectors." in r.stderr, r.stderr.decode()
    assert not out.exists()
    kio.write_ark_vectors(str(tmp_path / "d7.ark"), [("u%d" % i, rng.standard_normal(7).astype(np.float32)) for i in range(4)])
    r = _run([tool, str(tmp_path / "plda"), "ark:%s" % (tmp_path / "d7.ark"), str(out)])
    assert r.returncode == 255 and b"iVector dimension 7 does not match the PLDA dimension 6" in r.stderr, r.stderr.decode()
    assert not out.exists()
    whole = (tmp_path / "plda").read_bytes()
    (tmp_path / "cut").write_bytes(whole[: len(whole) // 2])
    r = _run([tool, str(tmp_path / "cut"), "ark:%s" % (tmp_path / "d7.ark"), str(out)])
    assert r.returncode == 255 and b"ERROR (ivector-adapt-plda)" in r.stderr
    assert not out.exists()
