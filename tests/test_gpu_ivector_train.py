"""GPU tests of i-vector extractor training (csrc/ivex_train_kernels.hip, csrc/ivex_train.cc): the rank update alone against numpy
for equality on small integers, the posterior kernel within bounds computed from the restatement's own Q, the statistics against
the restatement (tests/ivector_train_ref.py), determinism over how the utterances are split, five passes of EM, and
sid/train_ivector_extractor.sh:103-155 through real pipes."""
import os
import re
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import helpers as H
import ivector_cases as C
import ivector_ref as R
import ivector_train_ref as T
import ubm_ref as UR
from oracle import kaldi_io as kio
from ivector_cases import eps_of, random_utts

pytestmark = pytest.mark.gpu
P = H.pkg()
BIN = os.path.join(H.ROOT, H.PKG_NAME, "bin")
U53 = 2.0 ** -53
SLOTS = C.SLOTS
KEYS = ("gamma", "Y", "R", "S", "ivector_sum", "ivector_scatter")


# ------------------------------------------------------------------------------------------------------------------- rank update
@pytest.mark.parametrize("slots", [1, 3, 4, 5, 63, 64])
def test_the_rank_update_alone_equals_numpy_on_small_integers(slots):
    """small integers: every product and every partial sum is exact, so every order gives the same bits.  C carries two guard rows
    and three guard columns that must come back as they went; the slots beyond the filled count hold NaN and must not be read into
    the sum."""
    rng = np.random.default_rng(slots)
    for M in (1, 15, 16, 17, 33, 130):       # 130: more than one workgroup of 64 rows
        for N in (1, 15, 17, 136):           # 136: more than one column chunk of 128
            A = rng.integers(-8, 9, (SLOTS, M)).astype(np.float64)
            B = rng.integers(-8, 9, (SLOTS, N)).astype(np.float64)
            A[slots:], B[slots:] = np.nan, np.nan
            C = rng.integers(-100, 101, (M + 2, N + 3)).astype(np.float64)
            want = C.copy()
            want[:M, :N] += A[:slots].T @ B[:slots]
            got = P.ivex_rank_update(A, B, C, slots, M, N)
            assert np.array_equal(got, want), (M, N, slots)


def test_the_rank_update_refuses_what_it_cannot_run():
    with pytest.raises(P.XvError, match="slots"):
        P.ivex_rank_update(np.zeros((64, 2)), np.zeros((64, 2)), np.zeros((2, 2)), 65, 2, 2)
    with pytest.raises(P.XvError, match="ldc >= N"):
        P.ivex_rank_update(np.zeros((64, 2)), np.zeros((64, 3)), np.zeros((2, 2)), 4, 2, 3)


# ------------------------------------------------------------------------------------------------------------------- posterior
def feats_posts(utts):
    return [x for x, _ in utts], [p for _, p in utts]


@pytest.mark.parametrize("shape", C.POSTERIOR_CASES)
def test_the_posterior_kernel_within_bounds_from_the_restatements_q(shape):
    """S below, and across, the solve's panel width of 32; D at its limit; then S around one and two wavefronts of columns of Z
    (a wave skips the rows of Z above its lowest column, which is row 0 for the first wave), the recipes' 400, and kIvexMaxS, where
    every thread owns a column and the packed-index recovery sees its largest argument.  With eps = eps_of(Q) (Higham's backward
    error of the Cholesky factor carried to a solution, cond_2(Q) 4 S (3 S + 1) u):
      Var     every column of the inverse is a solve with the factor, and forming L^-T L^-1 is a second pass with the same constant:
              |Var - Q^-1| <= 2 eps |Q^-1|_2.  What the device holds is the scatter Var + m m': the solution's error eps |m| enters
              through both factors of m m', and the sum is rounded once.
      Q Var   the residual of the same inverse: |Q Var - I| <= 2 eps, plus what taking m m' off the scatter again costs.
      logdet  S logarithms summed in order, S u sum |log L_ii|, and the factor's relative error eps on each of the S diagonals."""
    G, D, S = shape
    m = C.posterior_model(G, D, S)
    ie = P.IvectorExtractor(**m)
    n = C.posterior_utts_count(S)
    utts = random_utts(S, n, G, D)
    feats, posts = feats_posts(utts)
    before = ie.extract(feats, posts)
    acc = P.IvexAccumulator(ie)
    assert not acc.accumulate(feats, posts).any()
    pend = acc.pending()
    after = ie.extract(feats, posts)
    for a, b in zip(before, after):   # what ivector-extract returns is what it returned before there was an accumulator
        assert a.tobytes() == b.tobytes()
    assert pend["m"].shape == (n, S)
    sim_U = R.derived(m["M"], m["sigma_inv"])
    worst = np.zeros(4)
    for u, (x, post) in enumerate(utts):
        e = T.e_step(x, post, m, sim_U)
        Q, mu = e["Q"], e["m"]
        eps = eps_of(Q)
        assert eps < 1e-6, "a precondition of the test's inputs"
        got_m = pend["m"][u]
        assert np.all(np.abs(got_m - mu) <= eps * np.linalg.norm(mu))
        want = got_m.copy()
        want[0] -= m["prior_offset"]
        assert np.array_equal(want.astype(np.float32), after[0][u])
        n_inv = np.linalg.norm(e["var"], 2)
        sc = R.unpack(pend["scatter"][u], S)
        bound = 2 * eps * n_inv + 2 * eps * np.linalg.norm(mu) * np.abs(mu)[:, None] + 2 * U53 * np.abs(e["scatter"])
        worst[0] = max(worst[0], (np.abs(sc - e["scatter"]) / bound).max())
        var = sc - np.outer(got_m, got_m)
        back = 4 * U53 * (np.abs(sc) + np.outer(np.abs(got_m), np.abs(got_m)))   # the scatter's rounding and the subtraction
        res = np.abs(Q @ var - np.eye(S))
        res_bound = 2 * eps + np.abs(Q) @ back + S * U53 * (np.abs(Q) @ np.abs(var))
        worst[1] = max(worst[1], (res / res_bound).max())
        L = np.linalg.cholesky(Q)
        ld_bound = 2 * (S * U53 * np.sum(np.abs(np.log(np.diag(L)))) + S * eps) + U53 * abs(e["logdet"])
        worst[2] = max(worst[2], abs(pend["logdet"][u] - e["logdet"]) / ld_bound)
        ax_bound = (S * S + 8) * U53 * e["auxf_post_abs"] + 2 * eps * e["auxf_post_abs"]
        worst[3] = max(worst[3], abs(pend["auxf"][u] - e["auxf_post"]) / ax_bound)
    print("S = %d: worst error / bound: scatter %.3g, Q Var - I %.3g, logdet %.3g, objective %.3g" % ((S,) + tuple(worst)))
    assert np.all(worst <= 1.0), worst


# ------------------------------------------------------------------------------------------------------------------- integer models
def fused_rank_update(A, B):
    """C[i][j] = the chain fma(A[k][i], B[k][j], C) over k ascending from zero, every step rounded once: exact rational arithmetic"""
    out = np.zeros((A.shape[1], B.shape[1]))
    for i in range(A.shape[1]):
        for j in range(B.shape[1]):
            c = 0.0
            for k in range(A.shape[0]):
                c = float(Fraction(float(A[k, i])) * Fraction(float(B[k, j])) + Fraction(c))
            out[i, j] = c
    return out


def test_integer_models_give_the_restatements_bits():
    """gamma and S_g are sums of exact products of small dyadic numbers: one set of bits in any order.  Y and R are the rank update
    of the fetched m and scatter: the matrix cores add the products of a k step into the accumulator with one rounding each, k
    ascending, which numpy restates in exact rational arithmetic."""
    G, D, S = 4, 6, 5
    m = R.integer_model(4065, G, D, S)
    ie = P.IvectorExtractor(**m)
    utts = [R.integer_utterance(100 + u, 6 + 3 * u, G, D) for u in range(10)]
    feats, posts = feats_posts(utts)
    acc = P.IvexAccumulator(ie)
    assert not acc.accumulate(feats, posts).any()
    pend = acc.pending()
    st = acc.get()
    gam = np.stack([R.stats(x, p, G)[0] for x, p in utts])
    X = np.stack([R.stats(x, p, G)[1].reshape(-1) for x, p in utts])
    assert np.array_equal(st["gamma"], gam.sum(axis=0))
    s2 = sum(np.stack([R.pack(s) for s in T.second_moment(x, p, G)]) for x, p in utts)
    assert np.array_equal(st["S"], s2)
    assert st["num_ivectors"] == 10 and st["frames"] == gam.sum()
    assert np.array_equal(st["R"], fused_rank_update(gam, pend["scatter"]))
    assert np.array_equal(st["Y"].reshape(G * D, S), fused_rank_update(X, pend["m"]))
    assert np.array_equal(st["ivector_sum"], fused_rank_update(np.ones((10, 1)), pend["m"])[0])
    assert np.array_equal(st["ivector_scatter"], fused_rank_update(np.ones((10, 1)), pend["scatter"])[0])


# ------------------------------------------------------------------------------------------------------------------- determinism
def run_acc(ie, utts, sizes, **kw):
    """accumulate in calls of the given sizes, cycling through them; returns (statistics, the concatenated status)"""
    acc = P.IvexAccumulator(ie, **kw)
    status, i, k = [], 0, 0
    while i < len(utts):
        n = sizes[k % len(sizes)]
        k += 1
        feats, posts = feats_posts(utts[i:i + n])
        status.append(acc.accumulate(feats, posts))
        i += n
    st = acc.get()
    acc.close()
    return st, np.concatenate(status)


def same_bits(a, b):
    return all(np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in a)


def test_how_the_utterances_are_split_over_calls_changes_no_bit():
    """70 utterances, more than one flush of 64.  Gaussian 0 has a negative 'inverse covariance', on purpose, and only the one bad
    utterance lands on it: its Q is not positive definite, an arithmetic flag of that utterance."""
    G, D, S = 6, 5, 7
    m = R.random_model(21, G, D, S)
    m["sigma_inv"][0] = R.pack(-8.0 * np.eye(D))
    rng = np.random.default_rng(3)
    utts = []
    for x, post in random_utts(5, 70, G - 1, D):
        utts.append((x, [(idx + 1, w) for idx, w in post]))   # Gaussians 1 .. G - 1
    ie = P.IvectorExtractor(**m)
    whole, status = run_acc(ie, utts, [70])
    assert not status.any() and whole["num_ivectors"] == 70
    by_one, _ = run_acc(ie, utts, [1])
    mixed, _ = run_acc(ie, utts, [7, 64])
    assert same_bits(whole, by_one) and same_bits(whole, mixed)
    bad = (rng.integers(-4, 5, (9, D)).astype(np.float32), [(np.array([0, 1], np.int32), np.array([1.0, 0.25], np.float32))] * 9)
    assert np.linalg.eigvalsh(T.e_step(*bad, m)["Q"]).min() < 0
    with_bad, status = run_acc(ie, utts[:35] + [bad] + utts[36:], [13])
    assert status.tolist() == [0] * 35 + [1] + [0] * 34 and with_bad["num_ivectors"] == 69
    without, _ = run_acc(ie, utts[:35] + utts[36:], [69])
    assert same_bits(with_bad, without)
    assert not same_bits(whole, without)


def test_the_split_changes_no_bit_at_a_size_beyond_two_wavefronts():
    """the same at S = 129 with 66 utterances: the posterior kernel on three wavefronts of columns, the small sums over 34
    workgroups and a flush of 64 followed by one of two"""
    G, D, S = C.SPLIT_SHAPE
    m = R.random_model(21, G, D, S, m_scale=C.m_scale_for(S))
    utts = random_utts(5, C.SPLIT_UTTS, G, D)
    ie = P.IvectorExtractor(**m)
    whole, status = run_acc(ie, utts, [C.SPLIT_UTTS])
    assert not status.any() and whole["num_ivectors"] == C.SPLIT_UTTS
    by_one, _ = run_acc(ie, utts, [1])
    mixed, _ = run_acc(ie, utts, [7, SLOTS])
    assert same_bits(whole, by_one) and same_bits(whole, mixed)


def test_frames_beyond_a_block_of_the_second_moment_change_no_bit_either():
    """the frames of the accepted utterances are cut into blocks of kFgmmAccFrameBlock (16384) for S_g: 7 utterances of about
    5000 frames straddle two block boundaries"""
    G, D, S = 3, 4, 5
    m = R.random_model(2, G, D, S)
    ie = P.IvectorExtractor(**m)
    utts = random_utts(8, 7, G, D, lo=4500, hi=5500)
    a, _ = run_acc(ie, utts, [7])
    b, _ = run_acc(ie, utts, [1, 2])
    assert sum(len(x) for x, _ in utts) > 2 * 16384 and same_bits(a, b)


# ------------------------------------------------------------------------------------------------------------------- random models
@pytest.mark.parametrize("update_variances", [True, False])
def test_random_models_within_the_any_order_bound_of_the_restatement(update_variances):
    """Every statistic within n 2^-53 sum |term| of the restatement's, with n the number of terms of its longest sum, plus, where the
    solve enters, the solve's own error from the restatement's Q (eps = eps_of(Q), as in the posterior kernel's test):
      gamma, S_g, frames   sums over (frame, Gaussian) pairs: n = the number of pairs, no other term.
      Y, ivector_sum       70 utterances, each term a product with X_u, itself a sum over at most n_u pairs: n = 70 + max n_u; the
                           solution's error eps |m_u| enters each utterance's term once.
      R, ivector_scatter   the same n; the scatter's error is the posterior test's 2 eps |Q^-1|_2 + 2 eps |m| |m_a|.
      auxf                 per utterance sums of S^2 terms and of its pairs on top of the 70: n = 70 + S^2 + max n_u; the posterior
                           part moves by 2 eps of its absolute terms."""
    _statistics_within_the_bound(C.STATS_CASES[0], update_variances)


@pytest.mark.parametrize("shape", C.STATS_CASES[1:])
def test_the_small_sums_beyond_one_workgroup_stay_within_the_same_bound(shape):
    """ivex_small_sums_kernel has one thread per element of gamma, ivector_sum, ivector_scatter and the objective, in workgroups of
    kIvexTrainThreads: at G = 5 the elements fill one workgroup up to S = 20, S = 21 is the first with a second one, and S = 70 has
    eleven.  70 utterances, so that the flush at kIvexTrainSlots still happens.  The bounds are those of the test above."""
    assert (C.small_sums_elements(shape[0], shape[2]) > C.TRAIN_THREADS) == (shape != C.STATS_CASES[1])
    _statistics_within_the_bound(shape, True)


def _statistics_within_the_bound(shape, update_variances):
    G, D, S = shape
    m = R.random_model(9, G, D, S, m_scale=C.m_scale_for(S))
    ie = P.IvectorExtractor(**m)
    utts = random_utts(12, 70, G, D)
    got, _ = run_acc(ie, utts, [70], update_variances=update_variances)
    want, ab = T.accumulate(utts, m, update_variances=update_variances, with_abs=True)
    pairs = [sum(len(idx) for idx, _ in post) for _, post in utts]
    assert got["num_ivectors"] == want["num_ivectors"] == 70
    assert (got["S"] is None) == (not update_variances)
    sim_U = R.derived(m["M"], m["sigma_inv"])
    solve = {k: np.zeros_like(np.asarray(want[k], dtype=np.float64)) for k in ("Y", "R", "ivector_sum", "ivector_scatter", "auxf")}
    for x, post in utts:
        e = T.e_step(x, post, m, sim_U)
        eps = eps_of(e["Q"])
        dm = eps * np.linalg.norm(e["m"]) * np.ones(S)
        dsc = R.pack(2 * eps * np.linalg.norm(e["var"], 2) + 2 * eps * np.linalg.norm(e["m"]) * np.abs(e["m"])[:, None] * np.ones((S, S)))
        solve["Y"] += np.abs(e["X"])[:, :, None] * dm[None, None, :]
        solve["R"] += np.abs(e["gamma"])[:, None] * dsc[None, :]
        solve["ivector_sum"] += dm
        solve["ivector_scatter"] += dsc
        solve["auxf"] += 2 * eps * e["auxf_post_abs"]
    n_of = dict(gamma=sum(pairs), S=sum(pairs), frames=sum(pairs), Y=70 + max(pairs), ivector_sum=70 + max(pairs), R=70 + max(pairs),
                ivector_scatter=70 + max(pairs), auxf=70 + S * S + max(pairs))
    for k in KEYS + ("auxf", "frames"):
        if want[k] is None:
            continue
        bound = n_of[k] * U53 * np.maximum(np.asarray(ab[k]), 1e-300) + solve.get(k, 0.0)
        ratio = np.max(np.abs(np.asarray(got[k]) - np.asarray(want[k])) / bound)
        print("%s: worst error / bound %.3g" % (k, ratio))
        assert ratio <= 1.0, k


# ------------------------------------------------------------------------------------------------------------------- EM
def test_five_passes_of_em_do_not_lower_the_bound():
    """The data of tests/ivector_train_ref.py's em_data; variance_floor_factor 1e-3, so that the variance floor stays out of play.
    Every pass the restatement accumulates from the same model as the device (the device's own chain of models), so the two
    objectives differ by summation order alone: n 2^-53 sum |term|, n the number of frames."""
    utts, model = T.em_data(0)
    feats, posts = feats_posts(utts)
    n = sum(len(x) for x in feats)
    objf = []
    for it in range(5):
        ie = P.IvectorExtractor(**model)
        acc = P.IvexAccumulator(ie)
        assert not acc.accumulate(feats, posts).any()
        st = acc.get()
        acc.close()
        want, ab = T.accumulate(utts, model, with_abs=True)
        tol = n * U53 * ab["auxf"]
        print("pass %d: objective per frame %.12g (restatement %.12g), |difference| / bound %.3g" %
              (it, st["auxf"] / st["frames"], want["auxf"] / want["frames"], abs(st["auxf"] - want["auxf"]) / tol))
        assert abs(st["auxf"] - want["auxf"]) <= tol and st["frames"] == want["frames"] == n
        objf.append((st["auxf"] / st["frames"], tol / n))
        out = P.ivex_est(st, model["w_vec"], model["M"], model["sigma_inv"], model["prior_offset"], variance_floor_factor=1e-3)
        model = {k: out[k] for k in ("w_vec", "M", "sigma_inv", "prior_offset")}
        ie.close()
    for (a, _), (b, tol) in zip(objf, objf[1:]):
        assert b >= a - tol, objf
    assert objf[-1][0] > objf[0][0] + 0.1


# ------------------------------------------------------------------------------------------------------------------- refusals
def test_limits_and_refusals_name_themselves():
    m = R.integer_model(1, 4, 2, 3)
    ie = P.IvectorExtractor(**m)
    acc = P.IvexAccumulator(ie)
    x = np.zeros((2, 2), np.float32)
    one = (np.array([0], np.int32), np.array([1.0], np.float32))
    with pytest.raises(P.XvError, match="name Gaussian 4"):
        acc.accumulate([x], [[one, (np.array([4], np.int32), np.array([1.0], np.float32))]])
    with pytest.raises(P.XvError, match="columns"):
        acc.accumulate([np.zeros((2, 3), np.float32)], [[one, one]])
    assert acc.get()["num_ivectors"] == 0


# ------------------------------------------------------------------------------------------------------------------- the recipe
def _sh(line):
    env = dict(os.environ, PATH=BIN + os.pathsep + os.environ.get("PATH", ""))
    return subprocess.run(["/bin/sh", "-c", line], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, timeout=300)


LIMIT = "timeout -k 10 120 "


def test_train_ivector_extractor_lines_run_with_the_recipes_argv(tmp_path):
    """train_ivector_extractor.sh:103, 113-116, 131 + 138 (two acc-stats children as "-|" arguments of sum-accs --parallel=true), 149
    and 155, two iterations, then an ivector-extract that reads the result.  Every step that opens the device runs under its own
    time limit, the children included."""
    d, data = tmp_path / "extractor", tmp_path / "split2"
    d.mkdir()
    G, S, nj = 8, 10, 2
    w, means, b, ic = UR.random_full_model(31, G, 60, spread=1.0)
    (d / "final.ubm").write_bytes(UR.full_gmm_bytes(w, b, ic, True))
    rng = np.random.default_rng(4)
    for j in (1, 2):
        (data / str(j)).mkdir(parents=True)
        utts = [("spk%d-%s" % (j, c), rng.normal(0.0, 4.0, size=(int(rng.integers(150, 220)), 20)).astype(np.float32)) for c in "abcd"]
        vads = [(k, (rng.uniform(size=len(x)) < 0.9).astype(np.float32)) for k, x in utts]
        kio.write_ark_matrices(str(data / str(j) / "raw.ark"), utts, scp_path=str(data / str(j) / "feats.scp"))
        kio.write_ark_vectors(str(data / str(j) / "vad.ark"), vads, scp_path=str(data / str(j) / "vad.scp"))
    feats = ("ark,s,cs:add-deltas --delta-window=3 --delta-order=2 scp:%s/JOB/feats.scp ark:- | apply-cmvn-sliding --norm-vars=false --center=true "
             "--cmn-window=300 ark:- ark:- | select-voiced-frames ark:- scp,s,cs:%s/JOB/vad.scp ark:- |" % (data, data))
    r = _sh("fgmm-global-to-gmm %s/final.ubm %s/final.dubm && ivector-extractor-init --ivector-dim=%d --use-weights=false %s/final.ubm %s/0.ie" % (d, d, S, d, d))
    assert r.returncode == 0, r.stderr
    for j in (1, 2):
        line = (LIMIT + 'gmm-gselect --n=5 %s/final.dubm "%s" ark:- | ' + LIMIT + 'fgmm-global-gselect-to-post --min-post=0.025 %s/final.ubm "%s" '
                'ark,s,cs:- ark:- | scale-post ark:- 1.0 "ark:|gzip -c >%s/post.JOB.gz"') % (d, feats, d, feats, d)
        r = _sh(line.replace("JOB", str(j)))
        assert r.returncode == 0, r.stderr
    for x in (0, 1):
        args = ["%sivector-extractor-acc-stats --num-threads=4 --num-samples-for-weights=3 %s/%d.ie '%s' 'ark,s,cs:gunzip -c %s/post.JOB.gz|' -|"
                .replace("JOB", str(j)) % (LIMIT, d, x, feats.replace("JOB", str(j)), d) for j in (1, 2)]
        r = _sh(LIMIT + 'ivector-extractor-sum-accs --parallel=true "%s" "%s" %s/acc.%d.1' % (args[0], args[1], d, x))
        log = r.stderr.decode()
        assert r.returncode == 0, log
        # one child at a time: the second one's first line comes after the first one's last
        starts = [mt.start() for mt in re.finditer(r"^ivector-extractor-acc-stats --num-threads=4", log, re.M)]
        ends = [mt.start() for mt in re.finditer(r"LOG \(ivector-extractor-acc-stats.*Wrote stats to -", log)]
        assert len(starts) == 2 and len(ends) == 2 and starts[0] < ends[0] < starts[1] < ends[1], log
        assert len(re.findall(r"LOG \(ivector-extractor-acc-stats\S* Done 4 files, 0 with errors\.", log)) == 2, log
        assert len(re.findall(r"Overall auxf/frame on training data was \S+ per frame over \S+ frames\.", log)) == 2, log
        r = _sh("ivector-extractor-sum-accs %s/acc.%d.1 %s/acc.%d && ivector-extractor-est --num-threads=4 %s/%d.ie %s/acc.%d %s/%d.ie" %
                (d, x, d, x, d, x, d, x, d, x + 1))
        assert r.returncode == 0, r.stderr
        assert b"variances floored in" in r.stderr
    st = P.ivex_stats_read(str(d / "acc.1"))
    assert st["num_ivectors"] == 8 and st["S"] is not None
    (d / "final.ie").write_bytes((d / "2.ie").read_bytes())
    r = _sh((LIMIT + 'ivector-extract %s/final.ie "%s" "ark,s,cs:gunzip -c %s/post.1.gz|" ark,t:%s/ivector.1.ark') % (d, feats.replace("JOB", "1"), d, d))
    assert r.returncode == 0, r.stderr
    assert re.search(rb"Done 4 files, 0 with errors", r.stderr)
    vecs = [l for l in (d / "ivector.1.ark").read_text().splitlines() if l.strip()]
    assert len(vecs) == 4 and all(len(l.split()) == S + 3 for l in vecs)


def test_a_posterior_a_frame_short_is_warned_about_and_counted(tmp_path):
    G, D, S = 4, 6, 5
    (tmp_path / "0.ie").write_bytes(R.ie_bytes(**R.random_model(9, G, D, S)))
    rng = np.random.default_rng(10)
    lens = {"a": 5, "b": 4, "c": 6}
    kio.write_ark_matrices(str(tmp_path / "f.ark"), [(k, rng.normal(size=(n, D)).astype(np.float32)) for k, n in lens.items()])
    post = {k: [[(int(rng.integers(0, G)), 1.0)] for _ in range(n)] for k, n in lens.items()}
    post["b"] = post["b"][:-1]
    (tmp_path / "p.post").write_bytes(UR.post_table_bytes(sorted(post.items()), True))
    r = _sh(LIMIT + "ivector-extractor-acc-stats %s/0.ie ark,s,cs:%s/f.ark ark,s,cs:%s/p.post %s/0.acc" % ((tmp_path,) * 4))
    log = r.stderr.decode()
    assert r.returncode == 0, log
    assert log.count(") Size mismatch between posterior 3 and features 4 for utterance b\n") == 1, log
    assert re.search(r"LOG \(ivector-extractor-acc-stats\S* Done 2 files, 1 with errors\.\n", log), log
    assert P.ivex_stats_read(str(tmp_path / "0.acc"))["num_ivectors"] == 2
