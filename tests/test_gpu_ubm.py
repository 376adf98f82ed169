"""GPU tests of the GMM-UBM stage (csrc/ubm_kernels.hip): deltas against the float32 restatement for equality, the two GMM
kernels against the float64 restatement (tests/ubm_ref.py) exactly on integer models and within the summation bound on random
ones, batch independence, and the command lines of sid/extract_ivectors.sh:58-68 through real pipes."""
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import helpers as H
import ubm_ref as R
from oracle import kaldi_io as kio

pytestmark = pytest.mark.gpu
P = H.pkg()
BIN = os.path.join(H.ROOT, H.PKG_NAME, "bin")

_HDR = open(os.path.join(H.ROOT, H.PKG_NAME, "csrc", "ubm_kernels.h")).read()
FB = int(re.search(r"kUbmFrameBlock = (\d+);", _HDR).group(1))
GT = int(re.search(r"kUbmGaussTile = (\d+);", _HDR).group(1))
DB = int(re.search(r"kDeltaRowBlock = (\d+);", _HDR).group(1))
FRAMES = [1, FB - 1, FB, FB + 1, 2 * FB + 3]
# (Gaussians, n, D): every Gaussian count {1, n, n + 1, GT - 1, GT, GT + 1, 2 GT + 5}, every n and every D at least once
CASES = [(1, 1, 1), (20, 20, 23), (21, 20, 60), (GT - 1, 30, 69), (GT, 64, 23), (GT + 1, 1, 60), (2 * GT + 5, 20, 60),
         (2 * GT + 5, 64, 69), (30, 30, 1), (65, 64, 60)]


# ------------------------------------------------------------------------------------------------------------------- deltas
@pytest.mark.parametrize("window", [1, 2, 3])
@pytest.mark.parametrize("order", [0, 1, 2, 3])
def test_deltas_equal_the_restatement_bit_for_bit(order, window):
    rng = np.random.default_rng(10 * order + window)
    # T = 1, T below the window, and row counts around the kernel's row block
    mats = [rng.normal(0.0, 10.0, size=(t, 20)).astype(np.float32) for t in (1, 2, 5, DB - 1, DB, DB + 1, 2 * DB + 3)]
    for truncate in (0, 13):
        got = P.add_deltas(mats, order=order, window=window, truncate=truncate)
        for x, g in zip(mats, got):
            want = R.add_deltas(x, order, window, truncate)
            assert g.shape == want.shape
            assert np.array_equal(g.view(np.uint32), want.view(np.uint32)), (x.shape, truncate)


# ------------------------------------------------------------------------------------------------------------------- exact
@functools.lru_cache(maxsize=None)
def integer_models(G, D):
    """Small integers and powers of two; gconst_g carries g * 2^-12 (diagonal) or g * 2^-10 (full), which makes every score of a
    frame different from every other (the rest of a score is a multiple of 1/2)."""
    rng = np.random.default_rng(1000 * G + D)
    g = np.arange(G)
    diag = dict(gconsts=(rng.integers(-8, 9, G) + g * 2.0 ** -12).astype(np.float32), means_invvars=rng.integers(-3, 4, (G, D)).astype(np.float32),
                inv_vars=(2.0 ** rng.integers(0, 3, (G, D))).astype(np.float32))
    ic = np.zeros((G, D * (D + 1) // 2), np.float32)
    for k in range(G):
        a = np.tril(rng.integers(-1, 2, (D, D)), -1).astype(np.float64)
        ic[k] = R.pack(a + a.T + np.diag(rng.integers(1, 3, D)))
    full = dict(gconsts=(rng.integers(-8, 9, G) + g * 2.0 ** -10).astype(np.float32), means_invcovars=rng.integers(-2, 3, (G, D)).astype(np.float32),
                inv_covars=ic)
    return diag, full


@pytest.mark.parametrize("G,n,D", CASES)
def test_integer_models_score_and_select_exactly(G, n, D):
    diag, full = integer_models(G, D)
    dm = P.Ubm.diag(diag["gconsts"], diag["means_invvars"], diag["inv_vars"])
    fm = P.Ubm.full(full["gconsts"], full["means_invcovars"], full["inv_covars"])
    rng = np.random.default_rng(G + n + D)
    for T in FRAMES:
        x = rng.integers(-4, 5, (T, D)).astype(np.float32)
        # every product and every partial sum is a multiple of 2^-12 below 2^12 in magnitude: 24 bits, whatever the order
        assert R.diag_abs_terms(x, **diag).max() * 2.0 ** 12 < 2.0 ** 24
        ll = R.diag_loglikes(x, **diag)
        assert all(len(np.unique(row)) == G for row in ll), "the restatement has a tie"
        want = R.gselect(ll, n)
        (sel,), (got_ll,) = dm.gselect([x], n, return_loglikes=True)
        assert np.array_equal(sel, want), (T, "selection")
        assert np.array_equal(got_ll.astype(np.float64), np.take_along_axis(ll, want, 1)), (T, "diagonal log-likelihoods")
        # the full model on a selection of its own: popular Gaussians, repeats across frames, any order inside a frame
        x2 = (x // 2).astype(np.float32)   # [-2, 2]
        pick = np.stack([rng.permutation(G)[:n] for _ in range(T)]).astype(np.int32)
        pick[::3, 0] = pick[0, 0]
        assert R.full_loglikes(x2, sel=pick, absolute=True, **full).max() * 2.0 ** 10 < 2.0 ** 24
        want_ll = R.full_loglikes(x2, sel=pick, **full)
        _, (got_full,), _ = fm.post([x2], [pick], return_details=True)
        assert np.array_equal(got_full.astype(np.float64), want_ll), (T, "full log-likelihoods: every (frame, slot) its own Gaussian's")


FT = int(re.search(r"kUbmFullFrameTile = (\d+);", _HDR).group(1))


def _split(T, n, G):
    """workgroups per Gaussian of the full-covariance kernel for a call of T frames (csrc/ubm.cc UbmPost)"""
    return max(1, min(64, (T * n // G) // (4 * FT)))


@pytest.mark.parametrize("T", [8 * FB + 3, 12 * FB + 5, 40 * FB + 1])
def test_full_scores_are_exact_with_several_workgroups_per_gaussian(T):
    """G = n: every frame lands in every bucket, so a bucket has T frames and the kernel runs 2, 3 and 10 workgroups per Gaussian,
    each taking every split-th tile of kUbmFullFrameTile frames; T is no multiple of the tile.  Exact against the fp64 restatement,
    and the same bits as the frames run in pieces small enough for one workgroup per Gaussian."""
    G = n = 20
    D = 23
    _, full = integer_models(G, D)
    fm = P.Ubm.full(**full)
    assert _split(T, n, G) == {8 * FB + 3: 2, 12 * FB + 5: 3, 40 * FB + 1: 10}[T]
    rng = np.random.default_rng(T)
    x = rng.integers(-2, 3, (T, D)).astype(np.float32)
    pick = np.stack([rng.permutation(G) for _ in range(T)]).astype(np.int32)
    assert R.full_loglikes(x, sel=pick, absolute=True, **full).max() * 2.0 ** 10 < 2.0 ** 24
    want = R.full_loglikes(x, sel=pick, **full)
    post, (ll,), (logsum,) = fm.post([x], [pick], min_post=0.025, return_details=True)
    assert np.array_equal(ll.astype(np.float64), want)
    piece = 4 * FT - 1
    assert _split(piece, n, G) == 1
    for a in range(0, T, piece):
        post_p, (ll_p,), (ls_p,) = fm.post([x[a:a + piece]], [pick[a:a + piece]], min_post=0.025, return_details=True)
        assert np.array_equal(ll_p.view(np.uint32), ll[a:a + piece].view(np.uint32))
        assert np.array_equal(ls_p.view(np.uint32), logsum[a:a + piece].view(np.uint32))
        for (i0, p0), (i1, p1) in zip(post_p[0], post[0][a:a + piece]):
            assert np.array_equal(i0, i1) and np.array_equal(p0.view(np.uint32), p1.view(np.uint32))


def test_a_call_longer_than_one_part_is_exact_in_every_part():
    """UbmPost sends 65536 frames at a time through buffers sized for the first part.  One call of 65536 + FB + 1 frames (the
    first part at 64 workgroups per Gaussian, the second at one) against the fp64 restatement, exactly, and the posteriors of
    the frames on both sides of the seam against the same frames in a call of their own."""
    G, n, D = 21, 20, 8
    _, full = integer_models(G, D)
    fm = P.Ubm.full(**full)
    T = 65536 + FB + 1
    assert _split(65536, n, G) == 64 and _split(FB + 1, n, G) == 1
    rng = np.random.default_rng(3)
    x = rng.integers(-2, 3, (T, D)).astype(np.float32)
    pick = np.argsort(rng.random((T, G)), axis=1)[:, :n].astype(np.int32)
    want = R.full_loglikes(x, sel=pick, **full)
    post, (ll,), (logsum,) = fm.post([x], [pick], min_post=0.025, return_details=True)
    assert np.array_equal(ll.astype(np.float64), want)
    a, b = 65536 - 40, 65536 + FB + 1
    post_s, _, (ls_s,) = fm.post([x[a:b]], [pick[a:b]], min_post=0.025, return_details=True)
    assert np.array_equal(ls_s.view(np.uint32), logsum[a:b].view(np.uint32))
    for (i0, p0), (i1, p1) in zip(post_s[0], post[0][a:b]):
        assert np.array_equal(i0, i1) and np.array_equal(p0.view(np.uint32), p1.view(np.uint32))


# ------------------------------------------------------------------------------------------------------------------- random
RANDOM = [(2 * GT + 5, 20, 60), (GT + 1, 30, 23)]
T_RANDOM = 6 * FB + 3


@functools.lru_cache(maxsize=None)
def random_case(G, D):
    # spread and noise 1: on these seeds the restatement alone excuses under 5 % of the frames (gap rule, min-post margin)
    w, means, b, ic = R.random_full_model(77 + G + D, G, D, spread=1.0)
    gc_f = R.full_gconsts(w, b, ic).astype(np.float32)
    gc_d, mi, iv = (a.astype(np.float32) for a in R.fgmm_to_gmm(w, b, ic))
    x = R.frames_around(5 + D, means, T_RANDOM, noise=1.0)
    diag = dict(gconsts=gc_d, means_invvars=mi, inv_vars=iv)
    full = dict(gconsts=gc_f, means_invcovars=b, inv_covars=ic)
    ll = R.diag_loglikes(x, **diag)
    eps = R.gamma(2 * D + 1 + 3) * R.diag_abs_terms(x, **diag)
    return x, diag, full, ll, eps


@pytest.mark.parametrize("G,n,D", RANDOM)
def test_random_models_select_within_the_summation_bound(G, n, D):
    """|device - fp64| <= gamma_m S for any order of the m - 3 = 2 D + 1 terms, S the sum of their absolute values (ubm_ref.gamma).
    Selected: fp64 score >= (n-th largest) - 2 eps; not selected: <= (n-th largest) + 2 eps; the order descending within 2 eps;
    where the n-th and (n + 1)-th are more than 2 eps apart the set is the restatement's, and at most 5 % of frames are not."""
    x, diag, full, ll, eps = random_case(G, D)
    dm = P.Ubm.diag(**{k: diag[k] for k in ("gconsts", "means_invvars", "inv_vars")})
    (sel,), (got,) = dm.gselect([x], n, return_loglikes=True)
    want = R.gselect(ll, n)
    e = eps.max(1)
    err = np.abs(got - np.take_along_axis(ll, sel, 1))
    print("worst error / bound %.3g" % float((err / np.take_along_axis(eps, sel, 1)).max()))
    assert np.all(err <= np.take_along_axis(eps, sel, 1))
    srt = -np.sort(-ll, axis=1)
    nth, nxt = srt[:, n - 1], srt[:, n]
    chosen = np.zeros(ll.shape, bool)
    np.put_along_axis(chosen, sel, True, 1)
    assert np.all(chosen.sum(1) == n)
    assert np.all(np.where(chosen, ll, np.inf) >= (nth - 2 * e)[:, None])
    assert np.all(np.where(chosen, -np.inf, ll) <= (nth + 2 * e)[:, None])
    picked = np.take_along_axis(ll, sel, 1)
    assert np.all(picked[:, :-1] >= picked[:, 1:] - 2 * e[:, None])
    clear = nth - nxt > 2 * e
    print("frames excused by the gap rule: %d of %d" % (int((~clear).sum()), len(clear)))
    assert (~clear).mean() <= 0.05
    assert np.array_equal(np.sort(sel[clear], 1), np.sort(want[clear], 1))


@pytest.mark.parametrize("min_post", [0.0, 0.025, 0.6])
@pytest.mark.parametrize("G,n,D", RANDOM)
def test_random_models_give_posteriors_within_the_bound(G, n, D, min_post):
    """Log-likelihoods within gamma_m S, m - 3 = D^2 + D + 1; with eps the largest bound of a frame every posterior is within
    exp(2 eps) - 1 relative of the restatement's, and the index lists are equal except on frames where an fp64 posterior lies
    within that margin of min_post (at most 5 % of the frames)."""
    x, diag, full, ll_d, _ = random_case(G, D)
    fm = P.Ubm.full(**{k: full[k] for k in ("gconsts", "means_invcovars", "inv_covars")})
    sel = R.gselect(ll_d, n)
    (post,), (got_ll,), (logsum,) = fm.post([x], [sel], min_post=min_post, return_details=True)
    ll = R.full_loglikes(x, sel=sel, **full)
    eps = R.gamma(D * D + D + 1 + 3) * R.full_loglikes(x, sel=sel, absolute=True, **full)
    err = np.abs(got_ll - ll)
    print("worst error / bound %.3g" % float((err / eps).max()))
    assert np.all(err <= eps)
    e = eps.max(1)
    raw, want_logsum = R.posteriors(ll, 0.0)
    want, _ = R.posteriors(ll, min_post)
    # no fp64 posterior is below float32's normal range: none can come out as 0 and be dropped for that reason alone
    assert raw.min() > 2.0 ** -120
    # the log-sum: within eps of the log-likelihoods' errors, plus the softmax's own float32 roundings - ll - max, expf and logf
    # (2 ulp each), n additions, max + log(sum) - which are below 8 * 2^-24 of the magnitudes they act on, |max| <= |logsum| + log n
    assert np.all(np.abs(logsum - want_logsum) <= e + 8 * 2.0 ** -24 * (np.abs(want_logsum) + np.log(n) + 1.0))
    margin = np.expm1(2 * e)
    near = (np.abs(raw - min_post) <= margin[:, None] * min_post).any(1) if min_post else np.zeros(len(x), bool)
    print("frames excused by the min-post margin: %d of %d" % (int(near.sum()), len(near)))
    assert near.mean() <= 0.05
    forced = 0
    for t in range(len(x)):
        idx, p = post[t]
        assert abs(float(p.sum()) - 1.0) < 1e-5
        if near[t]:
            continue
        keep = want[t] != 0.0
        forced += int(keep.sum() == 1 and raw[t].max() < min_post)
        assert idx.tolist() == sel[t][keep].tolist(), t
        assert np.all(np.abs(p - want[t][keep]) <= margin[t] * want[t][keep]), t
    if min_post == 0.6:
        assert forced > 0, "no frame took the arg-max branch"


# ------------------------------------------------------------------------------------------------------------------- batches
def test_an_utterance_has_the_same_bytes_alone_and_in_a_batch():
    G, n, D = 2 * GT + 5, 20, 60
    x_all, diag, full, _, _ = random_case(G, D)
    dm = P.Ubm.diag(**diag)
    fm = P.Ubm.full(**full)
    rng = np.random.default_rng(9)
    others = [rng.normal(0.0, 3.0, size=(int(r), D)).astype(np.float32) for r in rng.integers(1, 3 * FB, size=37)]
    for u, T in enumerate(FRAMES):
        x = x_all[u:u + T]
        (sel,), (ll,) = dm.gselect([x], n, return_loglikes=True)
        k = (5 * u + 3) % 38
        batch = others[:k] + [x] + others[k:]
        sel_b, ll_b = dm.gselect(batch, n, return_loglikes=True)
        assert np.array_equal(sel, sel_b[k]) and np.array_equal(ll.view(np.uint32), ll_b[k].view(np.uint32)), T
        (post,), (fl,), (ls,) = fm.post([x], [sel], min_post=0.025, return_details=True)
        post_b, fl_b, ls_b = fm.post(batch, sel_b, min_post=0.025, return_details=True)
        assert np.array_equal(fl.view(np.uint32), fl_b[k].view(np.uint32)) and np.array_equal(ls.view(np.uint32), ls_b[k].view(np.uint32)), T
        for (i0, p0), (i1, p1) in zip(post, post_b[k]):
            assert np.array_equal(i0, i1) and np.array_equal(p0.view(np.uint32), p1.view(np.uint32)), T


def test_limits_are_errors_that_name_them():
    diag, _ = integer_models(65, 60)
    dm = P.Ubm.diag(**diag)
    x = np.zeros((3, 60), np.float32)
    with pytest.raises(P.XvError, match="limit of 64"):
        dm.gselect([x], 65)
    with pytest.raises(P.XvError, match="limit of 96"):
        P.Ubm.diag(np.zeros(2, np.float32), np.zeros((2, 97), np.float32), np.ones((2, 97), np.float32))


# ------------------------------------------------------------------------------------------------------------------- the recipe
def _sh(line, cwd=None):
    env = dict(os.environ, PATH=BIN + os.pathsep + os.environ.get("PATH", ""))
    return subprocess.run(["/bin/sh", "-c", line], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, cwd=cwd, timeout=300)


def test_extract_ivectors_lines_run_with_the_recipes_argv(tmp_path):
    srcdir, sdata = tmp_path / "extractor", tmp_path / "split1" / "1"
    srcdir.mkdir()
    sdata.mkdir(parents=True)
    G, D = 70, 60
    w, means, b, ic = R.random_full_model(31, G, D, spread=1.0)
    (srcdir / "final.ubm").write_bytes(R.full_gmm_bytes(w, b, ic, True))
    (srcdir / "delta_opts").write_text("--delta-window=3 --delta-order=2\n")
    rng = np.random.default_rng(4)
    lens = {"spk1-a": 3 * FB + 5, "spk1-b": 41, "spk2-a": 150, "spk3-a": 97}
    utts = [(k, rng.normal(0.0, 4.0, size=(lens[k], 20)).astype(np.float32)) for k in sorted(lens)]
    vads = [(k, (rng.uniform(size=lens[k]) < 0.8).astype(np.float32)) for k in sorted(lens)]
    kio.write_ark_matrices(str(sdata / "raw.ark"), utts, scp_path=str(sdata / "feats.scp"))
    kio.write_ark_vectors(str(sdata / "vad.ark"), vads, scp_path=str(sdata / "vad.scp"))

    # extract_ivectors.sh:55-68, the strings as the script builds them (JOB = 1), up to and including scale-post
    delta_opts = (srcdir / "delta_opts").read_text().strip()
    feats = ("ark,s,cs:add-deltas %s scp:%s/feats.scp ark:- | apply-cmvn-sliding --norm-vars=false --center=true --cmn-window=300 ark:- ark:- | "
             "select-voiced-frames ark:- scp,s,cs:%s/vad.scp ark:- |" % (delta_opts, sdata, sdata))
    dubm = "fgmm-global-to-gmm %s/final.ubm -|" % srcdir
    line = ('gmm-gselect --n=20 "%s" "%s" ark:- | fgmm-global-gselect-to-post --min-post=0.025 %s/final.ubm "%s" ark,s,cs:- ark:- | '
            'scale-post ark:- 1.0 ark:-' % (dubm, feats, srcdir, feats))
    r = _sh(line)
    assert r.returncode == 0, r.stderr
    log = r.stderr.decode()
    assert re.search(r"LOG \(gmm-gselect.*Done 4 files, 0 with errors, average UBM log-likelihood is \S+ over \d+ frames\.", log), log
    assert re.search(r"LOG \(fgmm-global-gselect-to-post.*Done 4 files, 0 with errors, average log-likelihood per frame is \S+ over \d+ frames\.", log), log
    assert "Done 4 posteriors;  0 had no scales." in log and "Written diagonal GMM to -" in log
    got = R.read_post_table(r.stdout)
    assert [k for k, _ in got] == sorted(lens)

    # the same through the C ABI, on the features the tools themselves make
    r2 = _sh(feats[len("ark,s,cs:"):] + " cat > %s/prepared.ark" % tmp_path)
    assert r2.returncode == 0, r2.stderr
    prepared = dict(kio.read_ark(str(tmp_path / "prepared.ark")))
    for (k, raw), (_, v) in zip(utts, vads):   # deltas of the raw features sit under the mean normalisation: check the shape and the rows
        assert prepared[k].shape == (int(v.sum()), D)
    r3 = _sh("fgmm-global-to-gmm --binary=false %s/final.ubm -" % srcdir)
    dgm = R.read_diag_gmm(r3.stdout)
    dm = P.Ubm.diag(dgm["gconsts"], dgm["means_invvars"], dgm["inv_vars"])
    fm = P.Ubm.full(P.fgmm_gconsts(w, b, ic), b, ic)   # the gconsts the tool computes when it reads final.ubm
    keys = sorted(lens)
    sel = dm.gselect([prepared[k] for k in keys], 20)
    post = fm.post([prepared[k] for k in keys], sel, min_post=0.025)
    for (k, frames), want in zip(got, post):
        assert len(frames) == len(want)
        for f, (idx, p) in zip(frames, want):
            assert [i for i, _ in f] == idx.tolist(), k
            assert np.array_equal(np.array([q for _, q in f], np.float32).view(np.uint32), p.view(np.uint32)), k

    # text tables and a text model between the tools, one utterance missing from the selection: warned, counted, exit 0
    with open(sdata / "feats.scp") as f:
        lines = f.readlines()
    (sdata / "feats3.scp").write_text("".join(l for l in lines if not l.startswith("spk2-a")))
    r = _sh('fgmm-global-to-gmm --binary=false %s/final.ubm %s/final.dubm && gmm-gselect --n=100 %s/final.dubm "%s" ark,t:%s/gselect.txt'
            % (srcdir, tmp_path, tmp_path, feats.replace("feats.scp", "feats3.scp"), tmp_path))
    # --n=100 on 70 Gaussians is clamped with Kaldi's warning; 70 is still above the device's 64, which is then refused by name
    assert b"You asked for 100 Gaussians but GMM only has 70" in r.stderr
    assert r.returncode == 255 and b"--n=70 is above the limit of 64" in r.stderr
    # on a model the device takes whole, the clamped selection is every Gaussian, best first
    (tmp_path / "small.dubm").write_bytes(R.diag_gmm_bytes(dgm["weights"][:40], dgm["means_invvars"][:40], dgm["inv_vars"][:40], False))
    r = _sh('gmm-gselect --n=100 %s/small.dubm "%s" ark,t:%s/gselect.txt' % (tmp_path, feats.replace("feats.scp", "feats3.scp"), tmp_path))
    assert r.returncode == 0, r.stderr
    assert b"You asked for 100 Gaussians but GMM only has 40" in r.stderr and b"Done 3 files, 0 with errors" in r.stderr
    sel_txt = R.read_gselect_table((tmp_path / "gselect.txt").read_bytes())
    assert [k for k, _ in sel_txt] == [k for k in keys if k != "spk2-a"]
    assert all(sorted(row) == list(range(40)) for _, s in sel_txt for row in s)
    r = _sh('gmm-gselect --n=20 %s/final.dubm "%s" ark,t:- | fgmm-global-gselect-to-post --min-post=0.025 %s/final.ubm "%s" ark,s,cs:- ark,t:%s/post.txt'
            % (tmp_path, feats.replace("feats.scp", "feats3.scp"), srcdir, feats, tmp_path))
    assert r.returncode == 0, r.stderr
    assert b"No Gaussian-selection info available for utterance spk2-a" in r.stderr
    assert b"Done 3 files, 1 with errors, average log-likelihood per frame" in r.stderr
    txt = R.read_post_table((tmp_path / "post.txt").read_bytes())
    assert [(k, [[i for i, _ in f] for f in fr]) for k, fr in txt] == [(k, [[i for i, _ in f] for f in fr]) for k, fr in got if k != "spk2-a"]

    # a selection whose length is not the frame count is an error of that utterance
    bad = [(k, s[:-1] if k == "spk1-b" else s) for k, s in R.read_gselect_table(_sh('gmm-gselect --n=20 %s/final.dubm "%s" ark:-' % (tmp_path, feats)).stdout)]
    (tmp_path / "bad.ark").write_bytes(R.gselect_table_bytes(bad, True))
    r = _sh('fgmm-global-gselect-to-post %s/final.ubm "%s" ark:%s/bad.ark ark:/dev/null' % (srcdir, feats, tmp_path))
    assert r.returncode == 0 and b"for utterance spk1-b" in r.stderr and b"Done 3 files, 1 with errors" in r.stderr

    # limits and refusals
    big = R.diag_gmm_bytes(np.full(80, 1 / 80, np.float32), np.zeros((80, D), np.float32), np.ones((80, D), np.float32))
    (tmp_path / "big.dubm").write_bytes(big)
    r = _sh('gmm-gselect --n=65 %s/big.dubm "%s" ark:/dev/null' % (tmp_path, feats))
    assert r.returncode == 255 and b"limit of 64" in r.stderr
    r = _sh('gmm-gselect --write-likes=ark:/dev/null %s/big.dubm "%s" ark:/dev/null' % (tmp_path, feats))
    assert r.returncode == 255 and b"--write-likes is not built" in r.stderr
