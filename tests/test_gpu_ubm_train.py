"""Full-covariance UBM training on the device: the fp64 accumulator kernels (csrc/ubm_train_kernels.h) against the numpy restatement
(tests/ubm_train_ref.py), the fused E-step of fgmm-global-acc-stats against the tested pieces, and lines 75-108 of
sid/train_full_ubm.sh with their argv."""
import functools
import gzip
import os
import re
import subprocess

import numpy as np
import pytest

import helpers as H
import ubm_ref as R
import ubm_train_ref as T
from oracle import kaldi_io as kio

pytestmark = pytest.mark.gpu
P = H.pkg()
BIN = os.path.join(H.ROOT, H.PKG_NAME, "bin")
F = np.float32

_HDR = open(os.path.join(H.ROOT, H.PKG_NAME, "csrc", "ubm_train_kernels.h")).read()
C = int(re.search(r"kFgmmAccPairChunk = (\d+);", _HDR).group(1))
FB = int(re.search(r"kFgmmAccFrameBlock = (\d+);", _HDR).group(1))
LENGTHS = [0, 1, 3, 4, 5, C - 1, C, C + 1, 2 * C + 3]   # the bucket of Gaussian g has LENGTHS[g] pairs
G = len(LENGTHS)
DIMS = [1, 15, 16, 17, 33, 60, 96]


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


@functools.lru_cache(maxsize=None)
def pairs(seed=0):
    """(post_off [rows + 1], gauss [pairs]): one Gaussian per bucket length, the pairs dealt over frames of 0 to 4 pairs each, and
    frame 0 naming Gaussian 8 twice"""
    rng = np.random.default_rng(seed)
    gauss = rng.permutation(np.repeat(np.arange(G), LENGTHS))
    first = np.nonzero(gauss == 8)[0][:2]
    rest = np.delete(np.arange(len(gauss)), first)
    gauss = np.concatenate([gauss[first], gauss[rest]])
    counts = [2]
    while sum(counts) < len(gauss):
        counts.append(min(int(rng.integers(0, 5)), len(gauss) - sum(counts)))
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    frame = np.repeat(np.arange(len(counts)), counts)
    assert np.bincount(gauss, minlength=G).tolist() == LENGTHS and gauss[0] == gauss[1] == 8
    return off, gauss.astype(np.int32), frame


@functools.lru_cache(maxsize=None)
def integer_case(D, seed=1):
    """integer frames in [-4, 4], posteriors that are multiples of 2^-10 in (0, 1], and the restatement's sums, which are exact"""
    off, gauss, frame = pairs()
    rng = np.random.default_rng(seed + D)
    x = rng.integers(-4, 5, size=(len(off) - 1, D)).astype(F)
    p = (rng.integers(1, 1025, size=len(gauss)) / 1024.0).astype(F)
    ref = T.acc_stats(x, frame, gauss, p, G, 7)
    # every product and every partial sum is a multiple of 2^-10 below 2^53 * 2^-10: exact doubles in any order
    assert T.abs_terms(x, frame, gauss, p, G)[2].max() * 2.0 ** 10 < 2.0 ** 53
    return x, p, ref


def as_post(off, gauss, p):
    return [(gauss[off[t]:off[t + 1]], p[off[t]:off[t + 1]]) for t in range(len(off) - 1)]


@pytest.mark.parametrize("D", DIMS)
def test_integer_sums_equal_the_restatement_bit_for_bit(D):
    off, gauss, _ = pairs()
    x, p, ref = integer_case(D)
    acc = P.FgmmAccumulator(G, D, "mvw")
    acc.accumulate(x, as_post(off, gauss, p))
    got = acc.get()
    for name, a, b in zip(("occ", "mean", "cov"), got, ref):
        assert np.array_equal(bits(a), bits(b)), (name, D, np.argwhere(bits(a) != bits(b))[:5].tolist())
    assert not got[0][0] and not got[1][0].any() and not got[2][0].any()   # the empty bucket


@pytest.mark.parametrize("flags,D", [("w", 17), ("mw", 17), ("m", 33), ("v", 16), ("w", 96)])
def test_flags_gate_the_arrays(flags, D):
    off, gauss, _ = pairs()
    x, p, ref = integer_case(D)
    acc = P.FgmmAccumulator(G, D, flags)
    acc.accumulate(x, as_post(off, gauss, p))
    occ, mean, cov = acc.get()
    want = T.augment_flags(T.parse_flags(flags))
    assert np.array_equal(bits(occ), bits(ref[0]))
    assert np.array_equal(bits(mean), bits(ref[1] if want & 1 else np.zeros_like(ref[1])))
    assert np.array_equal(bits(cov), bits(ref[2] if want & 2 else np.zeros_like(ref[2])))


def test_three_calls_into_one_accumulator_add_block_by_block():
    D = 17
    off, gauss, _ = pairs()
    acc = P.FgmmAccumulator(G, D, "mvw")
    total = [0.0, 0.0, 0.0]
    for seed in (1, 2, 3):
        x, p, ref = integer_case(D, seed)
        acc.accumulate(x, as_post(off, gauss, p))
        total = [t + r for t, r in zip(total, ref)]   # exact: still integers over 2^10
    for a, b in zip(acc.get(), total):
        assert np.array_equal(bits(a), bits(b))


@pytest.mark.parametrize("D", [33, 60])
def test_random_sums_are_within_the_summation_bound(D):
    """fp32 Gaussian frames, uniform posteriors.  Every element within n_g 2^-52 sum_k p_k |x_ki| |x_kj| of the fp64 restatement: the
    worst case of any summation order with exact products (gamma_{n + 1} sum |terms|, about n 2^-53 sum |terms|) for the kernel and
    for the restatement, which sums in another order."""
    off, gauss, frame = pairs()
    rng = np.random.default_rng(100 + D)
    x = rng.normal(0.0, 3.0, size=(len(off) - 1, D)).astype(F)
    p = rng.uniform(0.0, 1.0, size=len(gauss)).astype(F)
    p[p == 0] = 1.0
    ref = T.acc_stats(x, frame, gauss, p, G, 7)
    a_occ, a_mean, a_cov, n_g = T.abs_terms(x, frame, gauss, p, G)
    acc = P.FgmmAccumulator(G, D, "mvw")
    acc.accumulate(x, as_post(off, gauss, p))
    worst = 0.0
    for name, got, want, s in zip(("occ", "mean", "cov"), acc.get(), ref, (a_occ, a_mean, a_cov)):
        bound = (n_g.reshape((-1,) + (1,) * (s.ndim - 1)) * 2.0 ** -52) * s
        err = np.abs(got - want)
        ratio = float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), 0.0)))
        print("D = %d  %-4s  worst error / bound = %.4f" % (D, name, ratio))
        worst = max(worst, ratio)
        assert np.all(err <= bound), (name, ratio)
        assert np.all(got[bound == 0] == 0)
    assert worst > 0.0   # the two orders do differ: the comparison is not one of a thing with itself


# ------------------------------------------------------------------------------------------------------------------- the tool
def _sh(line, cwd=None):
    env = dict(os.environ, PATH=BIN + os.pathsep + os.environ.get("PATH", ""))
    return subprocess.run(["/bin/sh", "-c", line], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, cwd=cwd, timeout=300)


def test_the_tools_partition_does_not_depend_on_the_utterances(tmp_path):
    Gm, n, D = 4, 2, 8
    rows = 2 * FB + 5
    w, means, b, ic = R.random_full_model(21, Gm, D, spread=1.0)
    x = R.frames_around(22, means, rows)
    rng = np.random.default_rng(23)
    gs = rng.integers(0, Gm, size=(rows, n)).astype(np.int32)   # some frames name a Gaussian twice
    (tmp_path / "0.ubm").write_bytes(R.full_gmm_bytes(w, b, ic, True))
    # 37 utterances of odd lengths; the last takes what is left
    lens = [2 * int(k) + 1 for k in rng.integers(100, 700, size=36)]
    lens.append(rows - sum(lens))
    assert lens[-1] > 0 and len(lens) == 37
    cuts = np.concatenate([[0], np.cumsum(lens)])
    out = []
    for name, bounds in (("one", [0, rows]), ("many", cuts)):
        keys = ["utt%03d" % i for i in range(len(bounds) - 1)]
        kio.write_ark_matrices(str(tmp_path / (name + ".ark")), [(k, x[bounds[i]:bounds[i + 1]]) for i, k in enumerate(keys)])
        (tmp_path / (name + ".gs")).write_bytes(R.gselect_table_bytes([(k, gs[bounds[i]:bounds[i + 1]]) for i, k in enumerate(keys)], True))
        r = _sh("fgmm-global-acc-stats --gselect=ark,s,cs:%s.gs 0.ubm ark,s,cs:%s.ark %s.acc" % (name, name, name), cwd=str(tmp_path))
        assert r.returncode == 0, r.stderr
        assert ("Done %d files; 0 with errors." % len(keys)).encode() in r.stderr
        assert re.search(rb"Overall likelihood per frame = \S+ over %d \(weighted\) frames\." % rows, r.stderr), r.stderr
        out.append((tmp_path / (name + ".acc")).read_bytes())
    assert out[0] == out[1]
    # the same from the tested pieces: Ubm.post's posteriors, block by block, into FgmmAccumulator.accumulate
    fm = P.Ubm.full(P.fgmm_gconsts(w, b, ic), b, ic)   # the gconsts the tool computes when it reads 0.ubm
    acc = P.FgmmAccumulator(Gm, D, "mvw")
    for r0 in range(0, rows, FB):
        post = fm.post([x[r0:r0 + FB]], [gs[r0:r0 + FB]], min_post=0.0)[0]
        assert all(len(i) == n for i, _ in post)   # no posterior underflows to 0 here: the pairs are the selection's
        acc.accumulate(x[r0:r0 + FB], post)
    assert out[0] == T.accs_bytes(*acc.get(), 7, True)
    # and the fused call on its own, with the log-sums of Ubm.post
    acc2 = P.FgmmAccumulator(Gm, D, "mvw")
    logsum = acc2.accumulate_gselect(fm, x[:FB], gs[:FB])
    _, _, want_logsum = fm.post([x[:FB]], [gs[:FB]], min_post=0.0, return_details=True)
    assert np.array_equal(logsum.view(np.uint32), want_logsum[0].view(np.uint32))


def test_limits_are_errors_that_name_them():
    w, means, b, ic = R.random_full_model(31, 70, 6)
    fm = P.Ubm.full(P.fgmm_gconsts(w, b, ic), b, ic)
    acc = P.FgmmAccumulator(70, 6, "mvw")
    x = np.zeros((3, 6), F)
    with pytest.raises(P.XvError, match="take 1 to 64"):
        acc.accumulate_gselect(fm, x, np.zeros((3, 65), np.int32))
    with pytest.raises(P.XvError, match="limit of 96"):
        P.FgmmAccumulator(2, 97, "mvw")
    with pytest.raises(P.XvError, match="name Gaussian 70; the accumulators have 70"):
        acc.accumulate(x, [(np.array([70], np.int32), np.ones(1, F))] * 3)
    with pytest.raises(P.XvError, match="names Gaussian 70; the model has 70"):
        acc.accumulate_gselect(fm, x, np.full((3, 2), 70, np.int32))
    assert not acc.get()[0].any()   # nothing was accumulated on the way


# ------------------------------------------------------------------------------------------------------------------- the recipe
def test_train_full_ubm_lines_run_with_the_recipes_argv(tmp_path):
    srcdir, dirr, data = tmp_path / "diag", tmp_path / "full", tmp_path / "data"
    for d in (srcdir, dirr, data / "split2" / "1", data / "split2" / "2"):
        d.mkdir(parents=True)
    sdata = data / "split2"
    nj, num_gselect, subsample, G0, raw_dim = 2, 4, 5, 8, 4
    _, means, _, _ = R.random_full_model(41, G0 - 1, raw_dim, spread=4.0)
    rng = np.random.default_rng(42)
    for job in (1, 2):
        utts = [("spk%d-%s" % (job, c), R.frames_around(100 * job + i, means, 1500 + 100 * i)) for i, c in enumerate("abcde")]
        vads = [(k, (rng.uniform(size=len(u)) < 0.95).astype(F)) for k, u in utts]
        kio.write_ark_matrices(str(sdata / str(job) / "raw.ark"), utts, scp_path=str(sdata / str(job) / "feats.scp"))
        kio.write_ark_vectors(str(sdata / str(job) / "vad.ark"), vads, scp_path=str(sdata / str(job) / "vad.scp"))
    (srcdir / "delta_opts").write_text("--delta-window=3 --delta-order=2\n")
    delta_opts = (srcdir / "delta_opts").read_text().strip()
    # train_full_ubm.sh:69, the string as the script builds it
    feats = ("ark,s,cs:add-deltas %s scp:%s/JOB/feats.scp ark:- | apply-cmvn-sliding --norm-vars=false --center=true --cmn-window=300 ark:- ark:- | "
             "select-voiced-frames ark:- scp,s,cs:%s/JOB/vad.scp ark:- | subsample-feats --n=%d ark:- ark:- |" % (delta_opts, sdata, sdata, subsample))
    # final.dubm: 7 Gaussians on frames of the prepared features and one where no data lies
    r = _sh(feats[len("ark,s,cs:"):].replace("JOB", "1") + " cat > %s/prepared.ark" % tmp_path)
    assert r.returncode == 0, r.stderr
    prepared = np.concatenate([m for _, m in kio.read_ark(str(tmp_path / "prepared.ark"))])
    D = prepared.shape[1]
    assert D == 12 and 1300 < len(prepared) < 1700   # about 3000 frames reach the E-step in the two jobs
    centres = [prepared[0].astype(np.float64)]   # farthest-point start and a few rounds of k-means: every Gaussian gets its share
    for _ in range(G0 - 2):
        centres.append(prepared[np.argmax(np.min([((prepared - c) ** 2).sum(1) for c in centres], axis=0))].astype(np.float64))
    for _ in range(5):
        owner = np.argmin([((prepared - c) ** 2).sum(1) for c in centres], axis=0)
        centres = [prepared[owner == k].mean(0) if np.any(owner == k) else c for k, c in enumerate(centres)]
    mu = np.concatenate([np.stack(centres), np.full((1, D), 60.0)]).astype(np.float64)
    iv = np.tile(1.0 / prepared.var(0), (G0, 1))
    (srcdir / "final.dubm").write_bytes(R.diag_gmm_bytes(np.full(G0, 1.0 / G0, F), (mu * iv).astype(F), iv.astype(F), True))

    def jobs(line):
        for job in range(1, nj + 1):
            r = _sh(line.replace("JOB", str(job)))
            assert r.returncode == 0, r.stderr.decode()
            yield r.stderr.decode()

    # :75
    r = _sh("gmm-global-to-fgmm %s/final.dubm %s/0.ubm" % (srcdir, dirr))
    assert r.returncode == 0 and b"Written full GMM to" in r.stderr, r.stderr
    # :87
    for log in jobs('gmm-gselect --n=%d "fgmm-global-to-gmm %s/0.ubm - |" "%s" "ark:|gzip -c >%s/gselect.JOB.gz"' % (num_gselect, dirr, feats, dirr)):
        assert "Done 5 files, 0 with errors" in log
    assert gzip.open(str(dirr / "gselect.1.gz")).read(6) == b"spk1-a"
    likes = []
    num_iters = 2
    for x in range(num_iters):
        # :97
        tot, frames = 0.0, 0
        for log in jobs('fgmm-global-acc-stats "--gselect=ark,s,cs:gunzip -c %s/gselect.JOB.gz|" %s/%d.ubm "%s" %s/%d.JOB.acc' % (dirr, dirr, x, feats, dirr, x)):
            assert "Done 5 files; 0 with errors." in log
            m = re.search(r"Overall likelihood per frame = (\S+) over (\d+) \(weighted\) frames\.", log)
            assert m, log
            tot += float(m.group(1)) * int(m.group(2))
            frames += int(m.group(2))
        assert 2600 < frames < 3400
        likes.append(tot / frames)
        # :100-108
        lowcount_opt = "--remove-low-count-gaussians=%s" % ("true" if x + 1 == num_iters else "false")
        r = _sh('fgmm-global-est %s --min-gaussian-weight=0.0001 --verbose=2 %s/%d.ubm "fgmm-global-sum-accs - %s/%d.*.acc |" %s/%d.ubm'
                % (lowcount_opt, dirr, x, dirr, x, dirr, x + 1))
        assert r.returncode == 0, r.stderr.decode()
        log = r.stderr.decode()
        assert "Summed 2 stats" in log and re.search(r"Overall objective function improvement is \S+ per frame over \S+ frames", log), log
        if x + 1 == num_iters:
            assert log.count("Too little data - removing Gaussian") == 1, log
        else:
            assert "remove-low-count-gaussians == false: i = 7" in log and "removing Gaussian" not in log, log
    print("likelihood per frame, pass by pass: %s" % likes)
    assert likes[1] >= likes[0], likes
    # :118, and the model reads back: the Gaussian that no frame selected is gone
    os.rename(str(dirr / ("%d.ubm" % num_iters)), str(dirr / "final.ubm"))
    r = _sh("fgmm-global-copy --binary=false %s/final.ubm -" % dirr)
    assert r.returncode == 0, r.stderr
    final = R.read_full_gmm(r.stdout)
    assert final["weights"].shape == (G0 - 1,) and abs(float(final["weights"].sum()) - 1.0) < 1e-6
    assert final["inv_covars"].shape == (G0 - 1, T.tri(D)) and np.all(np.isfinite(final["gconsts"]))
    sig = [np.linalg.inv(R.unpack(p, D)) for p in final["inv_covars"]]
    assert all(np.abs(s @ bb - 60.0).min() > 30.0 for s, bb in zip(sig, final["means_invcovars"].astype(np.float64)))


def test_acc_stats_words_and_counts_what_it_skips(tmp_path):
    """fgmm-global-acc-stats on five utterances, one usable: a key the --gselect table does not have, a selection a frame short
    and one of another width are warned and counted; a matrix without rows is warned and not counted."""
    Gm, D = 4, 8
    w, means, b, ic = R.random_full_model(51, Gm, D, spread=1.0)
    (tmp_path / "0.ubm").write_bytes(R.full_gmm_bytes(w, b, ic, True))
    x = R.frames_around(52, means, 12)
    kio.write_ark_matrices(str(tmp_path / "f.ark"), [("a", x[0:3]), ("b", x[3:5]), ("c", x[5:8]), ("d", x[8:12]), ("e", x[:0])])
    (tmp_path / "f.gs").write_bytes(R.gselect_table_bytes([("a", [[0, 1]] * 3), ("c", [[1, 2]] * 2), ("d", [[3]] * 4)], True))
    r = _sh("fgmm-global-acc-stats --gselect=ark,s,cs:f.gs 0.ubm ark,s,cs:f.ark f.acc", cwd=str(tmp_path))
    log = r.stderr.decode()
    assert r.returncode == 0, log
    for text in (") No gselect information for utterance b\n", ") gselect information for utterance c has wrong size 2 vs. 3\n",
                 ") The Gaussian selection of utterance d does not have the 2 indices per frame of the utterances before it (skipping utterance)\n",
                 ") Empty feature matrix for utterance e\n", ") Done 1 files; 3 with errors.\n"):
        assert log.count(text) == 1, log
    assert re.search(r"Overall likelihood per frame = \S+ over 3 \(weighted\) frames\.", log), log
