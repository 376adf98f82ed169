"""CPU tests of the host tools of diagonal UBM training through bin/: gmm-global-sum-accs, the accumulator file, gmm-global-est (the
M-step and --mix-up) against the numpy restatement (tests/dubm_train_ref.py), and the refusals.  No GPU is visible to the tools."""
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import dubm_train_ref as T
import helpers as H
import ubm_ref as R
import ubm_train_ref as FT
from oracle import kaldi_io as kio

BIN = os.path.join(H.ROOT, H.PKG_NAME, "bin")
U = 2.0 ** -24
F = np.float32


def run(args, stdin=None, shell=False):
    env = dict(os.environ, PATH=BIN + os.pathsep + os.environ.get("PATH", ""), HIP_VISIBLE_DEVICES="")
    if not shell:
        args = [os.path.join(BIN, args[0])] + list(args[1:])
    return subprocess.run(args, input=stdin, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, shell=shell, timeout=120)


# ------------------------------------------------------------------------------------------------------------- the accumulator file
def handmade_accs(occ, mean, var, flags):
    """the layout as the issue states it, laid down with struct.pack, not with the restatement's writers"""
    f32 = lambda v: struct.pack("<%df" % len(v), *[float(x) for x in v])
    i32 = lambda v: b"\x04" + struct.pack("<i", v)
    G, D = np.asarray(mean).shape
    out = (b"\0B<GMMACCS> <VECSIZE> " + i32(D) + b"<NUMCOMPONENTS> " + i32(G) + b"<FLAGS> \x02" + struct.pack("<H", flags)
           + b"<OCCUPANCY> FV " + i32(G) + f32(occ) + b"<MEANACCS> FM " + i32(G) + i32(D) + f32(np.asarray(mean).reshape(-1)))
    if flags & 2:
        out += b"<DIAGVARACCS> FM " + i32(G) + i32(D) + f32(np.asarray(var).reshape(-1))
    return out + b"</GMMACCS> "


def random_accs(seed, G=3, D=4):
    rng = np.random.default_rng(seed)
    return (rng.uniform(1, 500, G).astype(F), rng.normal(0, 300, size=(G, D)).astype(F), rng.uniform(1, 900, size=(G, D)).astype(F))


@pytest.mark.parametrize("flags", [7, 5, 4])
def test_sum_accs_adds_in_argument_order_and_the_file_round_trips(tmp_path, flags):
    parts = [random_accs(s) for s in (1, 2, 3)]
    if not flags & 2:
        parts = [(o, m, np.zeros_like(c)) for o, m, c in parts]
    if not flags & 1:
        parts = [(o, np.zeros_like(m), c) for o, m, c in parts]
    paths = []
    for i, p in enumerate(parts):
        paths.append(str(tmp_path / ("0.%d.acc" % (i + 1))))
        open(paths[-1], "wb").write(handmade_accs(*p, flags))
    assert handmade_accs(*parts[0], flags) == T.accs_bytes(*parts[0], flags, True)
    for k in (2, 3):
        want = [sum(np.asarray(p[j], np.float64) for p in parts[:k]).astype(F) for j in range(3)]   # left to right in fp64, one rounding
        r = run(["gmm-global-sum-accs", "-"] + paths[:k])
        assert r.returncode == 0, r.stderr
        assert b"Summed %d stats" % k in r.stderr and b"Written stats to -" in r.stderr
        assert r.stdout == T.accs_bytes(*want, flags, True)
    # binary -> text -> binary gives the same bytes
    r = run(["gmm-global-sum-accs", "--binary=false", str(tmp_path / "one.txt"), paths[0]])
    text = open(str(tmp_path / "one.txt"), "rb").read()
    assert r.returncode == 0 and text[:9] == b"<GMMACCS>"
    got = T.read_accs(text)
    assert got["flags"] == flags and all(np.array_equal(got[n], w) for n, w in zip(("occ", "mean", "var"), parts[0]))
    r = run(["gmm-global-sum-accs", "-", str(tmp_path / "one.txt")])
    assert r.returncode == 0 and r.stdout == open(paths[0], "rb").read()
    # sid/train_diag_ubm.sh:136, the statistics argument as the script writes it: the shell's glob gives the argument order
    r = run(["gmm-global-sum-accs", "-", "gmm-global-sum-accs - %s/0.*.acc|" % tmp_path])
    assert r.returncode == 0, r.stderr
    want = [sum(np.asarray(p[j], np.float64) for p in parts).astype(F) for j in range(3)]
    assert r.stdout == T.accs_bytes(*want, flags, True)


def test_sum_accs_refuses_what_does_not_agree(tmp_path):
    a, b, c, d = (str(tmp_path / n) for n in ("a.acc", "b.acc", "c.acc", "d.acc"))
    open(a, "wb").write(handmade_accs(*random_accs(1), 7))
    open(b, "wb").write(handmade_accs(*random_accs(2), 5))
    open(c, "wb").write(handmade_accs(*random_accs(2, G=4), 7))
    open(d, "wb").write(handmade_accs(*random_accs(2, D=3), 7))
    for other in (b, c, d):
        r = run(["gmm-global-sum-accs", "-", a, other])
        assert r.returncode == 255 and b"cannot be added" in r.stderr and r.stdout == b""
    r = run(["gmm-global-sum-accs", "-", a[:-1]])
    assert r.returncode == 255 and b"ERROR (gmm-global-sum-accs" in r.stderr
    r = run(["gmm-global-sum-accs", "-"])
    assert r.returncode == 1 and b"Usage: gmm-global-sum-accs" in r.stderr
    data = handmade_accs(*random_accs(1), 7)
    r = run(["gmm-global-sum-accs", "-", "-"], stdin=data.replace(b"<DIAGVARACCS>", b"<FULLVARACCS>"))
    assert r.returncode == 255 and b"expected token <DIAGVARACCS>, got <FULLVARACCS>" in r.stderr


def test_sum_accs_takes_a_full_covariance_file_only_without_variances(tmp_path):
    """the mirror of test_ubm_train_host's: <FULLVARACCS> is refused by name; a file with flags 5 has no such section, and both
    tools sum two of them to the same bytes"""
    (occ, mean, _), (occ2, mean2, _) = random_accs(1), random_accs(2)
    cov = np.random.default_rng(4).normal(0, 900, size=(3, FT.tri(4))).astype(F)
    r = run(["gmm-global-sum-accs", "-", "-"], stdin=FT.accs_bytes(occ, mean, cov, 7, True))
    assert r.returncode == 255 and b"expected token <DIAGVARACCS>, got <FULLVARACCS>" in r.stderr and r.stdout == b""
    a, b = str(tmp_path / "a.acc"), str(tmp_path / "b.acc")
    open(a, "wb").write(FT.accs_bytes(occ, mean, np.zeros_like(cov), 5, True))
    open(b, "wb").write(FT.accs_bytes(occ2, mean2, np.zeros_like(cov), 5, True))
    diag, full = run(["gmm-global-sum-accs", "-", a, b]), run(["fgmm-global-sum-accs", "-", a, b])
    assert diag.returncode == 0 and full.returncode == 0, (diag.stderr, full.stderr)
    want = [(np.asarray(x, np.float64) + y).astype(F) for x, y in ((occ, occ2), (mean, mean2))]
    assert diag.stdout == full.stdout == T.accs_bytes(*want, np.zeros_like(mean), 5, True)


# ------------------------------------------------------------------------------------------------------------- gmm-global-est
def est_case(seed=11, G=5, D=6):
    """a diagonal model and accumulators from hard assignments with posteriors in [0.5, 1].  Gaussian 2's last dimension has a
    standard deviation of 0.01 (below the default floor of 0.001 in variance), Gaussian 3 has 8 frames (an occupancy of about 6,
    below the default minimum of 10), Gaussian 4 none."""
    rng = np.random.default_rng(seed)
    means = rng.normal(0.0, 4.0, size=(G, D))
    iv = rng.uniform(0.3, 2.0, size=(G, D)).astype(F)
    mi = (means * iv).astype(F)
    w = rng.uniform(0.5, 1.5, G)
    w = (w / w.sum()).astype(F)
    counts = [1500, 1400, 1060, 8, 0]
    gauss, xs = [], []
    for g, c in enumerate(counts):
        scale = rng.uniform(0.7, 2.0, D)
        if g == 2:
            scale[-1] = 0.01
        xs.append((means[g] + 0.3 + rng.normal(size=(c, D)) * scale).astype(F))
        gauss += [g] * c
    x = np.concatenate(xs)
    p = rng.uniform(0.5, 1.0, len(x)).astype(F)
    return (w, mi, iv), T.acc_stats(x, np.arange(len(x)), np.array(gauss), p, G, 7)


def log_lines(stderr, prog):
    """[(level, text)] of the tool's own messages, the echo of the command line and 'Written' left out"""
    out = []
    for line in stderr.decode().splitlines():
        m = re.match(r"(LOG|WARNING) \(%s\[[^\]]*\]:main\(\):[\w.]+:\d+\) (.*)" % re.escape(prog), line)
        if m and not m.group(2).startswith("Written model to"):
            out.append((m.group(1), m.group(2)))
    return out


def check_model(got, want):
    """within the fp64-to-float rounding of the restatement: one rounding of values whose fp64 forms agree to far below 2^-24"""
    assert len(got["weights"]) == len(want["weights"])
    for name in ("weights", "means_invvars", "inv_vars"):
        a, b = got[name].astype(np.float64), np.asarray(want[name], np.float64)
        assert np.all(np.abs(a - b) <= 2 * U * np.abs(b)), (name, float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-30)) / U))


@pytest.mark.parametrize("binary", [True, False])
@pytest.mark.parametrize("options", [
    dict(),                                                            # an ordinary update: one variance floored, 3 and 4 removed
    dict(remove_low_count_gaussians=False),                            # both kept, with a warning each
    dict(min_gaussian_occupancy=1.0, min_variance=0.9),                # many floored; only the empty Gaussian goes
    dict(update_flags="w"), dict(update_flags="m"), dict(update_flags="v"), dict(update_flags="mw"),
])
def test_gmm_global_est_against_the_restatement(tmp_path, binary, options):
    (w, mi, iv), (occ, mean, var) = est_case()
    acc_file = T.accs_bytes(occ, mean, var, 7, binary)
    acc = T.read_accs(acc_file)   # the tool reads float32 accumulators: the restatement gets the same rounded values
    want = T.dgmm_est(w, mi, iv, acc["occ"], acc["mean"], acc["var"], 7, **options)
    (tmp_path / "0.dubm").write_bytes(R.diag_gmm_bytes(w, mi, iv, binary))
    (tmp_path / "0.acc").write_bytes(acc_file)
    args = ["--%s=%s" % (k.replace("_", "-"), str(v).lower() if isinstance(v, bool) else v) for k, v in options.items()]
    r = run(["gmm-global-est", "--binary=%s" % str(binary).lower()] + args + [str(tmp_path / "0.dubm"), str(tmp_path / "0.acc"), str(tmp_path / "1.dubm")])
    assert r.returncode == 0, r.stderr
    assert b"Written model to " + str(tmp_path / "1.dubm").encode() in r.stderr
    data = (tmp_path / "1.dubm").read_bytes()
    assert (data[:2] == b"\0B") == binary
    got = R.read_diag_gmm(data)
    assert log_lines(r.stderr, "gmm-global-est") == want["log"], r.stderr.decode()
    keep_all = options.get("remove_low_count_gaussians") is False
    assert want["removed"] == ([] if keep_all else [4] if "min_gaussian_occupancy" in options else [3, 4])
    if keep_all:
        assert [l[1].split(",")[0] for l in want["log"][:2]] == ["Gaussian has too little data but not removing it because remove-low-count-gaussians == false: i = 3",
                                                                  "Gaussian has too little data but not removing it because remove-low-count-gaussians == false: i = 4"]
    upd = options.get("update_flags", "mvw")
    if "min_variance" in options:
        assert want["floored"][1] == 4 and want["floored"][0] > 4
    else:   # without m the variance is taken around the old mean, 0.3 away: (0.3)^2 is above the floor
        assert want["floored"] == ((1, 1) if "m" in upd else (0, 0))
    assert (("WARNING", "%d variances floored in %d Gaussians." % want["floored"]) in want["log"]) == (want["floored"][0] > 0)
    check_model(got, want)
    np.testing.assert_allclose(got["gconsts"], want["gconsts"], rtol=1e-5, atol=1e-5)
    # only what the update flags name is copied back: the rest keeps its bits
    keep = [g for g in range(5) if g not in want["removed"]]
    if "v" not in upd:
        assert np.array_equal(got["inv_vars"], iv[keep])
    if "m" not in upd and "v" not in upd:
        assert np.array_equal(got["means_invvars"], mi[keep])
    if "w" not in upd and not want["removed"]:
        assert np.array_equal(got["weights"], w)
    if "m" in upd or "v" in upd:
        assert not np.array_equal(got["means_invvars"][:3], mi[:3])
    # the same through the C ABI
    P = H.pkg()
    py = P.dgmm_est(w, mi, iv, acc["occ"].astype(np.float64), acc["mean"].astype(np.float64), acc["var"].astype(np.float64), **options)
    assert py["removed"] == want["removed"] and py["floored"] == want["floored"] and py["split_of"] == []
    for name in ("weights", "means_invvars", "inv_vars"):
        assert np.array_equal(py[name], got[name]), name
    assert abs(py["objf_after"] - want["objf_after"]) <= 1e-9 * abs(want["objf_after"]) and py["count"] == want["count"]


def test_the_last_gaussian_is_never_removed(tmp_path):
    (w, mi, iv), (occ, mean, var) = est_case()
    small = [(a * 1e-3) for a in (occ, mean, var)]   # every occupancy below the minimum
    acc = T.read_accs(T.accs_bytes(*small, 7, True))
    want = T.dgmm_est(w, mi, iv, acc["occ"], acc["mean"], acc["var"], 7)
    assert want["removed"] == [0, 1, 2, 3] and "it is the last Gaussian: i = 4" in want["log"][4][1]
    (tmp_path / "0.dubm").write_bytes(R.diag_gmm_bytes(w, mi, iv, True))
    (tmp_path / "0.acc").write_bytes(T.accs_bytes(*small, 7, True))
    r = run(["gmm-global-est", str(tmp_path / "0.dubm"), str(tmp_path / "0.acc"), str(tmp_path / "1.dubm")])
    assert r.returncode == 0 and log_lines(r.stderr, "gmm-global-est") == want["log"], r.stderr.decode()
    got = R.read_diag_gmm((tmp_path / "1.dubm").read_bytes())
    assert got["weights"].tolist() == [1.0] and np.array_equal(got["inv_vars"], iv[4:])


def test_mix_up_splits_the_heaviest_gaussians_and_is_keyed_by_the_seed(tmp_path):
    (w, mi, iv), (occ, mean, var) = est_case()
    acc_file = T.accs_bytes(occ, mean, var, 7, True)
    acc = T.read_accs(acc_file)
    (tmp_path / "0.dubm").write_bytes(R.diag_gmm_bytes(w, mi, iv, True))
    (tmp_path / "0.acc").write_bytes(acc_file)
    base = T.dgmm_est(w, mi, iv, acc["occ"], acc["mean"], acc["var"], 7)   # 3 Gaussians survive
    assert len(base["weights"]) == 3
    out = {}
    for name, extra in (("a", ["--seed=5"]), ("b", ["--seed=5"]), ("c", ["--seed=6"]), ("d", [])):
        r = run(["gmm-global-est", "--mix-up=5", "--perturb-factor=0.05"] + extra + [str(tmp_path / "0.dubm"), str(tmp_path / "0.acc"), str(tmp_path / (name + ".dubm"))])
        assert r.returncode == 0 and b"Splitting to 5 Gaussians." in r.stderr, r.stderr
        out[name] = (tmp_path / (name + ".dubm")).read_bytes()
    assert out["a"] == out["b"] and out["a"] != out["c"] and out["c"] != out["d"]
    got = R.read_diag_gmm(out["a"])
    # the tool's own update (float32, as it stores it), split by the restatement
    r = run(["gmm-global-est", str(tmp_path / "0.dubm"), str(tmp_path / "0.acc"), str(tmp_path / "plain.dubm")])
    plain = R.read_diag_gmm((tmp_path / "plain.dubm").read_bytes())
    w2, mi2, iv2, split_of = T.split(plain["weights"], plain["means_invvars"], plain["inv_vars"], 5, 0.05, 5)
    order = np.argsort(-plain["weights"], kind="stable")
    assert split_of == [int(order[0]), int(order[1])] or split_of[0] == int(order[0])   # the heaviest first; then whatever is heaviest
    assert np.array_equal(got["weights"], w2) and np.array_equal(got["inv_vars"], iv2)
    assert np.all(np.abs(got["means_invvars"] - mi2) <= 2 * U * np.abs(mi2))   # cos and log may differ in the last fp64 bit
    assert not np.array_equal(got["means_invvars"][3], got["means_invvars"][split_of[0]])
    py = H.pkg().dgmm_est(w, mi, iv, acc["occ"].astype(np.float64), acc["mean"].astype(np.float64), acc["var"].astype(np.float64), mix_up=5,
                          perturb_factor=0.05, seed=5)
    assert py["split_of"] == split_of and np.array_equal(py["means_invvars"], got["means_invvars"])
    # a target that is not above the model's size changes nothing
    r = run(["gmm-global-est", "--mix-up=3", str(tmp_path / "0.dubm"), str(tmp_path / "0.acc"), str(tmp_path / "same.dubm")])
    assert r.returncode == 0 and (tmp_path / "same.dubm").read_bytes() == (tmp_path / "plain.dubm").read_bytes()


def test_est_through_the_scripts_stats_argument(tmp_path):
    (w, mi, iv), (occ, mean, var) = est_case()
    (tmp_path / "0.dubm").write_bytes(R.diag_gmm_bytes(w, mi, iv, True))
    half = [(a / 2).astype(F) for a in (occ, mean, var)]   # halving is exact, and so is adding the halves
    for j in (1, 2):
        (tmp_path / ("0.%d.acc" % j)).write_bytes(T.accs_bytes(*half, 7, True))
    (tmp_path / "whole.acc").write_bytes(T.accs_bytes(*[(2 * a.astype(np.float64)).astype(F) for a in half], 7, True))
    # sid/train_diag_ubm.sh:136-137
    line = ('gmm-global-est --remove-low-count-gaussians=false --min-gaussian-weight=0.0001 %s/0.dubm "gmm-global-sum-accs - %s/0.*.acc|" %s/1.dubm'
            % (tmp_path, tmp_path, tmp_path))
    r = run(line, shell=True)
    assert r.returncode == 0, r.stderr
    assert b"Summed 2 stats" in r.stderr and b"Overall objective function improvement is" in r.stderr
    r = run(["gmm-global-est", "--remove-low-count-gaussians=false", "--min-gaussian-weight=0.0001", str(tmp_path / "0.dubm"), str(tmp_path / "whole.acc"), str(tmp_path / "1b.dubm")])
    assert r.returncode == 0 and (tmp_path / "1.dubm").read_bytes() == (tmp_path / "1b.dubm").read_bytes()


def test_refusals_usage_errors_and_tools_that_need_a_gpu(tmp_path):
    r = run(["gmm-global-acc-stats", "0.dubm", "ark:feats.ark", "0.1.acc"])
    assert r.returncode == 255 and b"without --gselect is not built" in r.stderr
    r = run(["gmm-global-acc-stats", "--gselect=ark:gs.ark", "--weights=ark:w.ark", "0.dubm", "ark:feats.ark", "0.1.acc"])
    assert r.returncode == 255 and b"--weights is not built" in r.stderr
    r = run(["gmm-global-est", "--update-flags=x", "0.dubm", "0.acc", "1.dubm"])
    assert r.returncode == 255 and b"Invalid element 'x'" in r.stderr
    (w, mi, iv), (occ, mean, var) = est_case()
    (tmp_path / "0.dubm").write_bytes(R.diag_gmm_bytes(w, mi, iv, True))
    (tmp_path / "w.acc").write_bytes(T.accs_bytes(occ, np.zeros_like(mean), np.zeros_like(var), 4, True))
    r = run(["gmm-global-est", str(tmp_path / "0.dubm"), str(tmp_path / "w.acc"), "-"])   # update flags the file lacks
    assert r.returncode == 255 and b"name statistics that the accumulators (flags 'w') do not have" in r.stderr and r.stdout == b""
    r = run(["gmm-global-est", "--update-flags=w", str(tmp_path / "0.dubm"), str(tmp_path / "w.acc"), str(tmp_path / "1.dubm")])
    assert r.returncode == 0, r.stderr
    for tool, n in (("gmm-global-est", 2), ("gmm-global-acc-stats", 2), ("gmm-global-init-from-feats", 1), ("gmm-global-sum-accs", 1)):
        r = run([tool] + ["x"] * n)
        assert r.returncode == 1 and b"Usage: " + tool.encode() in r.stderr
    r = run(["gmm-global-init-from-feats", "--no-such-option=1", "ark:x", "y"])
    assert r.returncode != 0
    # the two device tools without a device: the project's message, exit 255
    rng = np.random.default_rng(0)
    kio.write_ark_matrices(str(tmp_path / "f.ark"), [("u1", rng.normal(size=(50, 6)).astype(F))])
    (tmp_path / "gs.ark").write_bytes(R.gselect_table_bytes([("u1", np.zeros((50, 2), np.int32))], True))
    r = run(["gmm-global-acc-stats", "--gselect=ark:%s/gs.ark" % tmp_path, str(tmp_path / "0.dubm"), "ark:%s/f.ark" % tmp_path, str(tmp_path / "x.acc")])
    assert r.returncode == 255 and b"no HIP device available" in r.stderr and not (tmp_path / "x.acc").exists()
    r = run(["gmm-global-init-from-feats", "--num-gauss=2", "--num-threads=32", "--num-iters=2", "ark:%s/f.ark" % tmp_path, str(tmp_path / "x.dubm")])
    assert r.returncode == 255 and b"no HIP device available" in r.stderr and not (tmp_path / "x.dubm").exists()
    # what the host does before it needs the device
    r = run(["gmm-global-init-from-feats", "--num-gauss=8", "ark:%s/f.ark" % tmp_path, str(tmp_path / "x.dubm")])
    assert r.returncode == 255 and b"Too few frames to train on" in r.stderr
    assert b"Number of frames read 50 was less than target number 200000, using all we read." in r.stderr
    r = run(["gmm-global-init-from-feats", "--num-gauss=2", "--num-frames=20", "ark:%s/f.ark" % tmp_path, str(tmp_path / "x.dubm")])
    assert b"Kept 20 out of 50 input frames = 40%." in r.stderr
