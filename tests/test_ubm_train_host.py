"""The host tools of full-covariance UBM training (gmm-global-to-fgmm, subsample-feats, fgmm-global-sum-accs, fgmm-global-est) run as
binaries on files written by the restatement (tests/ubm_train_ref.py).  No device is opened."""
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import helpers as H
import ubm_ref as R
import dubm_train_ref as DT
import ubm_train_ref as T
from oracle import kaldi_io as kio

BIN = os.path.join(H.ROOT, H.PKG_NAME, "bin")
U = 2.0 ** -24
F = np.float32


def run(args, stdin=None, shell=False):
    env = dict(os.environ, PATH=BIN + os.pathsep + os.environ.get("PATH", ""), HIP_VISIBLE_DEVICES="")
    if not shell:
        args = [os.path.join(BIN, args[0])] + list(args[1:])
    return subprocess.run(args, input=stdin, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, shell=shell, timeout=120)


# ------------------------------------------------------------------------------------------------------------- gmm-global-to-fgmm
def diag_model(seed=3, G=5, D=4):
    rng = np.random.default_rng(seed)
    w = rng.uniform(0.5, 1.5, G)
    iv = rng.uniform(0.5, 2.0, size=(G, D)).astype(F)
    mi = (rng.normal(size=(G, D)) * iv).astype(F)
    return (w / w.sum()).astype(F), mi, iv


def check_full(data, binary):
    w, mi, iv = diag_model()
    assert (data[:2] == b"\0B") == binary
    got = R.read_full_gmm(data)
    gc, b, ic = T.gmm_to_fgmm(w, mi, iv)
    assert np.array_equal(got["weights"], w) and np.array_equal(got["means_invcovars"], b) and np.array_equal(got["inv_covars"], ic)
    assert np.all(np.abs(got["gconsts"] - gc) <= 2 * U * np.abs(gc))


@pytest.mark.parametrize("binary", [True, False])
def test_gmm_global_to_fgmm_through_files_standard_streams_and_a_pipe(tmp_path, binary):
    w, mi, iv = diag_model()
    src, dst = tmp_path / "final.dubm", tmp_path / "0.ubm"
    src.write_bytes(R.diag_gmm_bytes(w, mi, iv, not binary))
    flag = "--binary=%s" % str(binary).lower()
    r = run(["gmm-global-to-fgmm", flag, str(src), str(dst)])
    assert r.returncode == 0, r.stderr
    assert b"LOG (gmm-global-to-fgmm" in r.stderr and b"Written full GMM to " + str(dst).encode() in r.stderr
    check_full(dst.read_bytes(), binary)
    r = run(["gmm-global-to-fgmm", flag, "-", "-"], stdin=src.read_bytes())
    assert r.returncode == 0, r.stderr
    check_full(r.stdout, binary)
    r = run(["gmm-global-to-fgmm", flag, "cat %s |" % src, "-"])
    assert r.returncode == 0, r.stderr
    check_full(r.stdout, binary)
    # and the diagonal image of the result is the model it came from
    r = run("gmm-global-to-fgmm %s - | fgmm-global-to-gmm --binary=false - -" % src, shell=True)
    assert r.returncode == 0, r.stderr
    back = R.read_diag_gmm(r.stdout)
    np.testing.assert_allclose(back["inv_vars"], iv, rtol=4 * U)
    np.testing.assert_allclose(back["means_invvars"], mi, rtol=1e-6, atol=1e-7)


# ------------------------------------------------------------------------------------------------------------- subsample-feats
UTTS = [("a", np.arange(33, dtype=F).reshape(11, 3)), ("b", np.arange(6, dtype=F).reshape(2, 3) + 100), ("c", np.arange(21, dtype=F).reshape(7, 3) - 50)]


@pytest.mark.parametrize("n,offset", [(1, 0), (1, 2), (5, 0), (5, 2), (-3, 0)])
def test_subsample_feats_keeps_or_repeats_rows(tmp_path, n, offset):
    src, dst = tmp_path / "feats.ark", tmp_path / "out.ark"
    kio.write_ark_matrices(str(src), UTTS)
    r = run(["subsample-feats", "--n=%d" % n, "--offset=%d" % offset, "ark:%s" % src, "ark:%s" % dst])
    want = [(k, T.subsample(x, n, offset)) for k, x in UTTS]
    lost = [k for k, x in want if x is None]
    want = [(k, x) for k, x in want if x is not None]
    assert r.returncode == 0, r.stderr
    got = list(kio.read_ark(str(dst)))
    assert [k for k, _ in got] == [k for k, _ in want]
    for (_, g), (_, x) in zip(got, want):
        assert np.array_equal(g, x)
    log = r.stderr.decode()
    assert "Processed %d feature matrices; %d with errors." % (len(want), len(lost)) in log
    assert "Processed 20 input frames and %d output frames." % sum(len(x) for _, x in want) in log
    for k in lost:   # offset 2 leaves nothing of the two-frame utterance
        assert "For utterance %s, output would have no rows" % k in log
    assert (lost == ["b"]) == (offset == 2)


def test_subsample_feats_statuses_and_usage(tmp_path):
    src = tmp_path / "short.ark"
    kio.write_ark_matrices(str(src), UTTS[1:2])
    r = run(["subsample-feats", "--n=5", "--offset=2", "ark:%s" % src, "ark:/dev/null"])   # nothing is written: status 1
    assert r.returncode == 1 and b"Processed 0 feature matrices; 1 with errors." in r.stderr
    r = run(["subsample-feats", "--n=0", "ark:%s" % src, "ark:/dev/null"])
    assert r.returncode == 1 and b"Usage: subsample-feats" in r.stderr
    r = run(["subsample-feats", "--n=-2", "--offset=1", "ark:%s" % src, "ark:/dev/null"])
    assert r.returncode == 255 and b"--offset=1 cannot be used with a negative --n" in r.stderr
    r = run("cat %s | subsample-feats --n=-2 ark:- ark,t:-" % src, shell=True)   # through pipes, text out
    assert r.returncode == 0 and r.stdout.split()[:5] == [b"b", b"[", b"100", b"101", b"102"]


# ------------------------------------------------------------------------------------------------------------- the accumulator file
def handmade_accs(occ, mean, cov, flags):
    """the layout as the issue states it, laid down with struct.pack, not with the restatement's writers"""
    f32 = lambda v: struct.pack("<%df" % len(v), *[float(x) for x in v])
    i32 = lambda v: b"\x04" + struct.pack("<i", v)
    G, D = np.asarray(mean).shape
    out = (b"\0B<GMMACCS> <VECSIZE> " + i32(D) + b"<NUMCOMPONENTS> " + i32(G) + b"<FLAGS> \x02" + struct.pack("<H", flags)
           + b"<OCCUPANCY> FV " + i32(G) + f32(occ) + b"<MEANACCS> FM " + i32(G) + i32(D) + f32(np.asarray(mean).reshape(-1)))
    if flags & 2:
        out += b"<FULLVARACCS> " + b"".join(b"FP " + i32(D) + f32(c) for c in cov)
    return out + b"</GMMACCS> "


def random_accs(seed, G=3, D=4):
    rng = np.random.default_rng(seed)
    return (rng.uniform(1, 500, G).astype(F), rng.normal(0, 300, size=(G, D)).astype(F), rng.normal(0, 900, size=(G, T.tri(D))).astype(F))


@pytest.mark.parametrize("flags", [7, 5, 4])
def test_sum_accs_reads_a_handmade_file_and_adds_in_fp64(tmp_path, flags):
    parts = [random_accs(s) for s in (1, 2, 3)]
    if not flags & 2:
        parts = [(o, m, np.zeros_like(c)) for o, m, c in parts]
    if not flags & 1:
        parts = [(o, np.zeros_like(m), c) for o, m, c in parts]
    paths = []
    for i, p in enumerate(parts):
        paths.append(str(tmp_path / ("x.%d.acc" % (i + 1))))
        open(paths[-1], "wb").write(handmade_accs(*p, flags))
    assert handmade_accs(*parts[0], flags) == T.accs_bytes(*parts[0], flags, True)   # the restatement writes the same bytes
    for k in (2, 3):
        want = [sum(np.asarray(p[j], np.float64) for p in parts[:k]).astype(F) for j in range(3)]   # left to right in fp64, one rounding
        r = run(["fgmm-global-sum-accs", "-"] + paths[:k])
        assert r.returncode == 0, r.stderr
        assert b"Summed %d stats" % k in r.stderr and b"Written stats to -" in r.stderr
        assert r.stdout == T.accs_bytes(*want, flags, True)
        # text out, text in, and the recipe's "fgmm-global-sum-accs - a.1.acc a.2.acc |" as an input of itself
        r = run(["fgmm-global-sum-accs", "--binary=false", str(tmp_path / "sum.txt")] + paths[:k])
        assert r.returncode == 0 and open(str(tmp_path / "sum.txt"), "rb").read()[:9] == b"<GMMACCS>"
        got = T.read_accs(open(str(tmp_path / "sum.txt"), "rb").read())
        assert got["flags"] == flags and all(np.array_equal(got[n], w) for n, w in zip(("occ", "mean", "cov"), want))
        r = run(["fgmm-global-sum-accs", "-", str(tmp_path / "sum.txt")])
        assert r.returncode == 0 and r.stdout == T.accs_bytes(*want, flags, True)
    r = run(["fgmm-global-sum-accs", "-", "fgmm-global-sum-accs - %s %s |" % (paths[0], paths[1]), paths[2]])
    assert r.returncode == 0, r.stderr
    two = [(np.asarray(parts[0][j], np.float64) + parts[1][j]).astype(F) for j in range(3)]   # rounded once by the inner tool
    assert r.stdout == T.accs_bytes(*[(np.asarray(two[j], np.float64) + parts[2][j]).astype(F) for j in range(3)], flags, True)


def test_sum_accs_refuses_what_does_not_agree(tmp_path):
    a, b, c, d = (str(tmp_path / n) for n in ("a.acc", "b.acc", "c.acc", "d.acc"))
    open(a, "wb").write(handmade_accs(*random_accs(1), 7))
    open(b, "wb").write(handmade_accs(*random_accs(2), 5))
    open(c, "wb").write(handmade_accs(*random_accs(2, G=4), 7))
    open(d, "wb").write(handmade_accs(*random_accs(2, D=3), 7))
    for other in (b, c, d):
        r = run(["fgmm-global-sum-accs", "-", a, other])
        assert r.returncode == 255 and b"cannot be added" in r.stderr and r.stdout == b""
    r = run(["fgmm-global-sum-accs", "-", a[:-1]])
    assert r.returncode == 255 and b"ERROR (fgmm-global-sum-accs" in r.stderr
    r = run(["fgmm-global-sum-accs", "-"])
    assert r.returncode == 1 and b"Usage: fgmm-global-sum-accs" in r.stderr
    data = handmade_accs(*random_accs(1), 7)
    r = run(["fgmm-global-sum-accs", "-", "-"], stdin=data[:-30])
    assert r.returncode == 255
    r = run(["fgmm-global-sum-accs", "-", "-"], stdin=data.replace(b"<MEANACCS>", b"<MEANACCZ>"))
    assert r.returncode == 255 and b"expected token <MEANACCS>, got <MEANACCZ>" in r.stderr


def test_sum_accs_takes_a_diagonal_file_only_without_variances(tmp_path):
    """the two kinds of file differ in the section that v adds: with it the other kind's token is refused by name; without it the
    files are the same, and both tools sum them to the same bytes"""
    (occ, mean, _), (occ2, mean2, _) = random_accs(1), random_accs(2)
    var = np.random.default_rng(4).uniform(1, 900, size=mean.shape).astype(F)
    r = run(["fgmm-global-sum-accs", "-", "-"], stdin=DT.accs_bytes(occ, mean, var, 7, True))
    assert r.returncode == 255 and b"expected token <FULLVARACCS>, got <DIAGVARACCS>" in r.stderr and r.stdout == b""
    a, b = str(tmp_path / "a.acc"), str(tmp_path / "b.acc")
    open(a, "wb").write(DT.accs_bytes(occ, mean, np.zeros_like(var), 5, True))
    open(b, "wb").write(DT.accs_bytes(occ2, mean2, np.zeros_like(var), 5, True))
    full, diag = run(["fgmm-global-sum-accs", "-", a, b]), run(["gmm-global-sum-accs", "-", a, b])
    assert full.returncode == 0 and diag.returncode == 0, (full.stderr, diag.stderr)
    want = [(np.asarray(x, np.float64) + y).astype(F) for x, y in ((occ, occ2), (mean, mean2))]
    assert full.stdout == diag.stdout == T.accs_bytes(*want, np.zeros((3, T.tri(4)), F), 5, True)


# ------------------------------------------------------------------------------------------------------------- fgmm-global-est
def est_case(seed=11, G=5, D=6, T_=4000):
    """a model, and accumulators built here from hard assignments of well-spread data with posteriors in [0.5, 1]: per-dimension
    standard deviations in [0.7, 2], so that every covariance has a condition number far below 10^3, with or without flooring.
    Gaussian 3 has 40 frames (an occupancy of about 30, below the default minimum), Gaussian 4 none."""
    rng = np.random.default_rng(seed)
    w, means, b, ic = R.random_full_model(seed, G, D)
    counts = [1500, 1400, 1060, 40, 0]
    frame, gauss, xs = [], [], []
    for g, c in enumerate(counts):
        scale = rng.uniform(0.7, 2.0, D)
        xs.append((means[g] + rng.normal(size=(c, D)) * scale).astype(F))
        gauss += [g] * c
    x = np.concatenate(xs)
    p = rng.uniform(0.5, 1.0, len(x)).astype(F)
    return (w, b, ic), T.acc_stats(x, np.arange(len(x)), np.array(gauss), p, G, 7)


def log_lines(stderr, prog):
    """[(level, text)] of the tool's own messages, the echo of the command line and 'Written' left out"""
    out = []
    for line in stderr.decode().splitlines():
        m = re.match(r"(LOG|WARNING) \(%s\[[^\]]*\]:main\(\):[\w.]+:\d+\) (.*)" % re.escape(prog), line)
        if m and not m.group(2).startswith("Written model to"):
            out.append((m.group(1), m.group(2)))
    return out


def check_est(got, want, removed_count):
    assert len(got["weights"]) == len(want["weights"]) == 5 - removed_count
    assert np.all(np.abs(got["weights"] - want["weights"]) <= 2 * U * np.abs(want["weights"]))
    D = got["means_invcovars"].shape[1]
    for g in range(len(got["weights"])):
        for name in ("inv_covars", "means_invcovars"):
            a, b = got[name][g].astype(np.float64), want[name][g].astype(np.float64)
            assert np.all(np.abs(a - b) <= 2 * U * np.abs(b).max()), (name, g, np.abs(a - b).max() / np.abs(b).max() / U)
        # what the bound rests on: the condition number of the covariance is below 10^3
        s = np.linalg.eigvalsh(R.unpack(want["inv_covars"][g], D))
        assert s.max() / s.min() < 1e3


@pytest.mark.parametrize("binary", [True, False])
@pytest.mark.parametrize("options", [
    dict(),
    dict(remove_low_count_gaussians=False),
    dict(min_gaussian_occupancy=10.0, variance_floor=0.9, max_condition=4.0),   # floors many eigenvalues, removes only the empty Gaussian
    dict(update_flags="v"), dict(update_flags="m"), dict(update_flags="w"), dict(update_flags="mw"),
])
def test_fgmm_global_est_against_the_restatement(tmp_path, binary, options):
    (w, b, ic), (occ, mean, cov) = est_case()
    # the tool reads float32 accumulators: the restatement gets the same rounded values
    acc_file = T.accs_bytes(occ, mean, cov, 7, binary)
    acc = T.read_accs(acc_file)
    want = T.fgmm_est(w, b, ic, acc["occ"], acc["mean"], acc["cov"], 7, **options)
    (tmp_path / "0.ubm").write_bytes(R.full_gmm_bytes(w, b, ic, binary))
    (tmp_path / "0.acc").write_bytes(acc_file)
    args = ["--%s=%s" % (k.replace("_", "-"), str(v).lower() if isinstance(v, bool) else v) for k, v in options.items()]
    r = run(["fgmm-global-est", "--binary=%s" % str(binary).lower(), "--verbose=2"] + args + [str(tmp_path / "0.ubm"), str(tmp_path / "0.acc"), str(tmp_path / "1.ubm")])
    assert r.returncode == 0, r.stderr
    assert b"Written model to " + str(tmp_path / "1.ubm").encode() in r.stderr
    data = (tmp_path / "1.ubm").read_bytes()
    assert (data[:2] == b"\0B") == binary
    got = R.read_full_gmm(data)
    assert log_lines(r.stderr, "fgmm-global-est") == want["log"], r.stderr.decode()
    removed = len(want["removed"])
    assert removed == (0 if options.get("remove_low_count_gaussians") is False else 1 if "min_gaussian_occupancy" in options else 2)
    if "variance_floor" in options:
        assert want["floored"][0] > 4 and want["floored"][1] == 4
    check_est(got, want, removed)
    np.testing.assert_allclose(got["gconsts"], want["gconsts"], rtol=1e-5, atol=1e-5)
    # the same through the C ABI
    P = H.pkg()
    py = P.fgmm_est(w, b, ic, acc["occ"].astype(np.float64), acc["mean"].astype(np.float64), acc["cov"].astype(np.float64), **options)
    assert py["removed"] == want["removed"] and py["floored"] == want["floored"]
    for name in ("weights", "means_invcovars", "inv_covars"):
        assert np.array_equal(py[name], got[name]), name
    assert abs(py["objf_after"] - want["objf_after"]) <= 1e-9 * abs(want["objf_after"]) and py["count"] == want["count"]


def test_fgmm_global_est_through_the_recipes_stats_argument(tmp_path):
    (w, b, ic), (occ, mean, cov) = est_case()
    (tmp_path / "0.ubm").write_bytes(R.full_gmm_bytes(w, b, ic, True))
    half = [(a / 2).astype(F) for a in (occ, mean, cov)]   # halving is exact, and so is adding the halves
    for j in (1, 2):
        (tmp_path / ("0.%d.acc" % j)).write_bytes(T.accs_bytes(*half, 7, True))
    (tmp_path / "whole.acc").write_bytes(T.accs_bytes(*[(2 * a.astype(np.float64)).astype(F) for a in half], 7, True))
    line = ('fgmm-global-est --remove-low-count-gaussians=false --min-gaussian-weight=0.0001 --verbose=2 %s/0.ubm "fgmm-global-sum-accs - %s/0.*.acc |" %s/1.ubm'
            % (tmp_path, tmp_path, tmp_path))
    r = run(line, shell=True)
    assert r.returncode == 0, r.stderr
    assert b"Summed 2 stats" in r.stderr and b"Overall objective function improvement is" in r.stderr
    r = run(["fgmm-global-est", "--remove-low-count-gaussians=false", "--min-gaussian-weight=0.0001", str(tmp_path / "0.ubm"), str(tmp_path / "whole.acc"), str(tmp_path / "1b.ubm")])
    assert r.returncode == 0 and (tmp_path / "1.ubm").read_bytes() == (tmp_path / "1b.ubm").read_bytes()


def test_refusals_name_what_they_refuse(tmp_path):
    r = run(["fgmm-global-acc-stats", "0.ubm", "ark:feats.ark", "0.1.acc"])
    assert r.returncode == 255 and b"without --gselect is not built" in r.stderr
    r = run(["fgmm-global-acc-stats", "--gselect=ark:gs.ark", "--weights=ark:w.ark", "0.ubm", "ark:feats.ark", "0.1.acc"])
    assert r.returncode == 255 and b"--weights is not built" in r.stderr
    r = run(["fgmm-global-est", "--mix-up=4096", "0.ubm", "0.acc", "1.ubm"])
    assert r.returncode == 255 and b"--mix-up is not built" in r.stderr
    # and what is not refused but wrong
    r = run(["fgmm-global-est", "--update-flags=x", "0.ubm", "0.acc", "1.ubm"])
    assert r.returncode == 255 and b"Invalid element 'x'" in r.stderr
    (w, b, ic), (occ, mean, cov) = est_case()
    (tmp_path / "0.ubm").write_bytes(R.full_gmm_bytes(w, b, ic, True))
    (tmp_path / "w.acc").write_bytes(T.accs_bytes(occ, np.zeros_like(mean), cov, 4, True))
    r = run(["fgmm-global-est", str(tmp_path / "0.ubm"), str(tmp_path / "w.acc"), "-"])
    assert r.returncode == 255 and b"name statistics that the accumulators (flags 'w') do not have" in r.stderr and r.stdout == b""
    r = run(["fgmm-global-est", "0.ubm", "0.acc"])
    assert r.returncode == 1 and b"Usage: fgmm-global-est" in r.stderr
    # --mix-up=0 is what the option defaults to, and w alone leaves the Gaussians as they are
    r = run(["fgmm-global-est", "--mix-up=0", "--update-flags=w", str(tmp_path / "0.ubm"), str(tmp_path / "w.acc"), str(tmp_path / "1.ubm")])
    assert r.returncode == 0, r.stderr
    assert np.array_equal(R.read_full_gmm((tmp_path / "1.ubm").read_bytes())["inv_covars"][:3], ic[:3])
