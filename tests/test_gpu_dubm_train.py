"""Diagonal UBM training on the device: the accumulator kernels and both E-steps (csrc/dubm_train_kernels.h) against the numpy
restatement (tests/dubm_train_ref.py) and against the selection kernel's own scores, and lines 105-137 of sid/train_diag_ubm.sh with
their argv."""
import functools
import gzip
import os
import re
import subprocess

import numpy as np
import pytest

import dubm_train_ref as T
import helpers as H
import ubm_ref as R
from oracle import kaldi_io as kio

pytestmark = pytest.mark.gpu
P = H.pkg()
BIN = os.path.join(H.ROOT, H.PKG_NAME, "bin")
F = np.float32
U = 2.0 ** -24

_CSRC = os.path.join(H.ROOT, H.PKG_NAME, "csrc")
C = int(re.search(r"kFgmmAccPairChunk = (\d+);", open(os.path.join(_CSRC, "ubm_train_kernels.h")).read()).group(1))
_HDR = open(os.path.join(_CSRC, "dubm_train_kernels.h")).read()
FC = int(re.search(r"kDgmmDenseFrameChunk = (\d+);", _HDR).group(1))
FB = int(re.search(r"kDgmmAccFrameBlock = (\d+);", _HDR).group(1))
LENGTHS = [0, 1, 3, C - 1, C, C + 1, 2 * C + 3]   # the bucket of Gaussian g has LENGTHS[g] pairs
G_SPARSE = len(LENGTHS)
DIMS = [1, 15, 16, 17, 33, 60, 96]


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def same_bits(got, want, what):
    for name, a, b in zip(("occ", "mean", "var"), got, want):
        assert np.array_equal(bits(a), bits(b)), (what, name, np.argwhere(bits(a) != bits(b))[:5].tolist())


# ------------------------------------------------------------------------------------------------------------------- exact, sparse
@functools.lru_cache(maxsize=None)
def pairs(seed=0):
    """(post_off [rows + 1], gauss [pairs], frame [pairs]): one Gaussian per bucket length, the pairs dealt over frames of 0 to 4 pairs
    each, and frame 0 naming Gaussian 6 twice"""
    rng = np.random.default_rng(seed)
    gauss = rng.permutation(np.repeat(np.arange(G_SPARSE), LENGTHS))
    first = np.nonzero(gauss == 6)[0][:2]
    rest = np.delete(np.arange(len(gauss)), first)
    gauss = np.concatenate([gauss[first], gauss[rest]])
    counts = [2]
    while sum(counts) < len(gauss):
        counts.append(min(int(rng.integers(0, 5)), len(gauss) - sum(counts)))
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    frame = np.repeat(np.arange(len(counts)), counts)
    assert np.bincount(gauss, minlength=G_SPARSE).tolist() == LENGTHS and gauss[0] == gauss[1] == 6
    return off, gauss.astype(np.int32), frame


@functools.lru_cache(maxsize=None)
def integer_case(D, seed=1):
    """integer frames in [-4, 4], posteriors that are multiples of 2^-10 in (0, 1], and the restatement's sums, which are exact"""
    off, gauss, frame = pairs()
    rng = np.random.default_rng(seed + D)
    x = rng.integers(-4, 5, size=(len(off) - 1, D)).astype(F)
    p = (rng.integers(1, 1025, size=len(gauss)) / 1024.0).astype(F)
    ref = T.acc_stats(x, frame, gauss, p, G_SPARSE, 7)
    # every product and every partial sum is a multiple of 2^-10 below 2^53 * 2^-10: exact doubles in any order
    assert T.abs_terms(x, frame, gauss, p, G_SPARSE)[2].max() * 2.0 ** 10 < 2.0 ** 53
    return x, p, ref


def as_post(off, gauss, p):
    return [(gauss[off[t]:off[t + 1]], p[off[t]:off[t + 1]]) for t in range(len(off) - 1)]


@pytest.mark.parametrize("D", DIMS)
def test_sparse_integer_sums_equal_the_restatement_bit_for_bit(D):
    off, gauss, _ = pairs()
    x, p, ref = integer_case(D)
    acc = P.DgmmAccumulator(G_SPARSE, D, "mvw")
    acc.accumulate(x, as_post(off, gauss, p))
    got = acc.get()
    same_bits(got, ref, D)
    assert not got[0][0] and not got[1][0].any() and not got[2][0].any()   # the empty bucket


@pytest.mark.parametrize("flags,D", [("w", 17), ("mw", 17), ("m", 33), ("v", 16), ("w", 96)])
def test_flags_gate_the_arrays(flags, D):
    off, gauss, _ = pairs()
    x, p, ref = integer_case(D)
    want = T.augment_flags(T.parse_flags(flags))
    gated = (ref[0], ref[1] if want & 1 else np.zeros_like(ref[1]), ref[2] if want & 2 else np.zeros_like(ref[2]))
    acc = P.DgmmAccumulator(G_SPARSE, D, flags)
    acc.accumulate(x, as_post(off, gauss, p))
    same_bits(acc.get(), gated, "sparse")
    dense = np.zeros((len(x), G_SPARSE), F)   # the same pairs as a dense matrix: the repeated pair of frame 0 added up (exact)
    np.add.at(dense, (pairs()[2], gauss), p)
    acc = P.DgmmAccumulator(G_SPARSE, D, flags)
    acc.accumulate_dense_post(x, dense)
    same_bits(acc.get(), gated, "dense")


def test_three_calls_into_one_accumulator_add_block_by_block():
    D = 17
    off, gauss, frame = pairs()
    acc, acc_d = P.DgmmAccumulator(G_SPARSE, D, "mvw"), P.DgmmAccumulator(G_SPARSE, D, "mvw")
    total = [0.0, 0.0, 0.0]
    for seed in (1, 2, 3):
        x, p, ref = integer_case(D, seed)
        acc.accumulate(x, as_post(off, gauss, p))
        dense = np.zeros((len(x), G_SPARSE), F)
        np.add.at(dense, (frame, gauss), p)
        acc_d.accumulate_dense_post(x, dense)
        total = [t + r for t, r in zip(total, ref)]   # exact: still integers over 2^10
    same_bits(acc.get(), total, "sparse")
    same_bits(acc_d.get(), total, "dense")


# ------------------------------------------------------------------------------------------------------------------- exact, dense
DENSE_G = [1, 15, 16, 17, 64, 65, 130]
DENSE_ROWS = [1, 3, 4, 63, 64, 65, FC + 1]


@pytest.mark.parametrize("D", [1, 17, 33, 60, 96])
def test_dense_mfma_sums_equal_the_restatement_bit_for_bit(D):
    """The accumulation kernel alone on an asymmetric pattern: a wrong f64 fragment map (rows for columns, the f32 row formula) or a
    mask error moves a sum to another (Gaussian, column) or drops it.  Integer frames, posteriors that are multiples of 2^-10; a whole
    Gaussian and a whole frame of zeros."""
    rng = np.random.default_rng(7000 + D)
    for G in DENSE_G:
        for rows in DENSE_ROWS:
            x = rng.integers(-4, 5, size=(rows, D)).astype(F)
            post = (rng.integers(0, 1025, size=(rows, G)) / 1024.0).astype(F)
            post *= (rng.uniform(size=(rows, G)) < 0.7)   # scattered zeros
            if G > 2:
                post[:, G // 2] = 0
            if rows > 2:
                post[rows // 2, :] = 0
            ref = T.dense_stats(x, post)
            assert (post.astype(np.float64).T @ (x.astype(np.float64) ** 2)).max() * 2.0 ** 10 < 2.0 ** 53
            acc = P.DgmmAccumulator(G, D, "mvw")
            acc.accumulate_dense_post(x, post)
            same_bits(acc.get(), ref, (G, rows))


# ------------------------------------------------------------------------------------------------------------------- scores
@functools.lru_cache(maxsize=None)
def integer_model(G, D):
    """small integers and powers of two; gconst_g carries g * 2^-12, which makes every score of a frame different from every other"""
    rng = np.random.default_rng(1000 * G + D)
    return dict(gconsts=(rng.integers(-8, 9, G) + np.arange(G) * 2.0 ** -12).astype(F), means_invvars=rng.integers(-3, 4, (G, D)).astype(F),
                inv_vars=(2.0 ** rng.integers(0, 3, (G, D))).astype(F))


@functools.lru_cache(maxsize=None)
def random_model(G, D, rows=512):
    """a random diagonal model (the diagonal image of ubm_ref's full one), frames around its means, the float64 scores and their bound"""
    w, means, b, ic = R.random_full_model(77 + G + D, G, D, spread=1.0)
    gc, mi, iv = (a.astype(F) for a in R.fgmm_to_gmm(w, b, ic))
    x = R.frames_around(5 + D, means, rows, noise=1.0)
    model = dict(gconsts=gc, means_invvars=mi, inv_vars=iv)
    return x, model, R.diag_loglikes(x, **model), T.score_bound(x, **model)


@pytest.mark.parametrize("G,n,D", [(7, 7, 1), (65, 20, 33), (130, 64, 60), (300, 30, 96)])
def test_selected_scores_are_the_selection_kernels_bit_for_bit(G, n, D):
    rng = np.random.default_rng(G + D)
    cases = [(integer_model(G, D), rng.integers(-4, 5, (131, D)).astype(F))]
    x, model, _, _ = random_model(G, D)
    cases.append((model, x))
    for model, x in cases:
        dm = P.Ubm.diag(**model)
        (sel,), (ll,) = dm.gselect([x], n, return_loglikes=True)
        acc = P.DgmmAccumulator(G, D, "mvw")
        _, got = acc.accumulate_gselect(dm, x, sel, return_loglikes=True)
        assert np.array_equal(got.view(np.uint32), ll.view(np.uint32))
        # any order inside a frame and repeats across frames: every (frame, slot) its own Gaussian's
        perm = np.stack([rng.permutation(n) for _ in range(len(x))])
        _, got = acc.accumulate_gselect(dm, x, np.take_along_axis(sel, perm, 1), return_loglikes=True)
        assert np.array_equal(got.view(np.uint32), np.take_along_axis(ll, perm, 1).view(np.uint32))


@pytest.mark.parametrize("G,D", [(1, 33), (17, 33), (64, 33), (64, 60)])
def test_dense_logsum_on_the_devices_own_scores(G, D):
    """G <= 64: xv_ubm_gselect(n = G) returns every score of the frame, the bits the dense kernel recomputes.  Their float64
    log-sum-exp against the device's: within 8 * 2^-24 (|L| + log G + 1), the bound test_gpu_ubm uses for ubm_post (expf and logf at 2
    ulp each, the subtraction, the final rounding)."""
    x, model, _, _ = random_model(G, D)
    dm = P.Ubm.diag(**model)
    (_,), (ll,) = dm.gselect([x], G, return_loglikes=True)
    _, want = R.posteriors(ll.astype(np.float64))
    got = P.DgmmAccumulator(G, D, "mvw").accumulate_dense(dm, x)
    err, bound = np.abs(got - want), 8 * U * (np.abs(want) + np.log(G) + 1.0)
    print("G = %d  D = %d  worst error / bound = %.4f" % (G, D, float((err / bound).max())))
    assert np.all(err <= bound)


@pytest.mark.parametrize("G", [130, 2048])
def test_dense_logsum_against_the_float64_scores(G):
    """the bound above plus the scores' own: gamma(2 D + 4) sum |terms|, the largest of the frame"""
    D = 60
    x, model, ll, eps = random_model(G, D)
    assert len(x) == 512
    _, want = R.posteriors(ll)
    got = P.DgmmAccumulator(G, D, "mvw").accumulate_dense(P.Ubm.diag(**model), x)
    err, bound = np.abs(got - want), eps.max(1) + 8 * U * (np.abs(want) + np.log(G) + 1.0)
    print("G = %d  worst error / bound = %.4f" % (G, float((err / bound).max())))
    assert np.all(err <= bound)


# ------------------------------------------------------------------------------------------------------------------- fused statistics
def check_stats(got, x, post64, e, what):
    """every element within the bound of dubm_train_ref.weighted_error_bound of the float64 restatement's statistics"""
    x64 = x.astype(np.float64)
    want = (post64.sum(0), post64.T @ x64, post64.T @ (x64 * x64))
    worst = 0.0
    for name, a, b, bound in zip(("occ", "mean", "var"), got, want, T.weighted_error_bound(x, post64, e)):
        err = np.abs(a - b)
        ratio = float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), 0.0)))
        print("%s  %-4s  worst error / bound = %.4f" % (what, name, ratio))
        worst = max(worst, ratio)
        assert np.all(err <= bound), (what, name, ratio)
    assert worst > 0.0   # the comparison is not one of a thing with itself


@pytest.mark.parametrize("G", [17, 130])
@pytest.mark.parametrize("D", [33, 60])
def test_fused_dense_statistics_are_within_the_derived_bound(G, D):
    x, model, ll, eps = random_model(G, D)
    post64, _ = R.posteriors(ll)
    acc = P.DgmmAccumulator(G, D, "mvw")
    acc.accumulate_dense(P.Ubm.diag(**model), x)
    check_stats(acc.get(), x, post64, eps.max(1), "dense G = %d D = %d" % (G, D))


@pytest.mark.parametrize("n", [1, 20, 64])
@pytest.mark.parametrize("D", [33, 60])
def test_fused_sparse_statistics_are_within_the_derived_bound(n, D):
    G = 130
    x, model, ll, eps = random_model(G, D)
    dm = P.Ubm.diag(**model)
    (sel,) = dm.gselect([x], n)
    p_sel, want_logsum = R.posteriors(np.take_along_axis(ll, sel, 1))
    post64 = np.zeros((len(x), G))
    np.put_along_axis(post64, sel, p_sel, 1)
    e = np.take_along_axis(eps, sel, 1).max(1)
    acc = P.DgmmAccumulator(G, D, "mvw")
    logsum = acc.accumulate_gselect(dm, x, sel)
    assert np.all(np.abs(logsum - want_logsum) <= e + 8 * U * (np.abs(want_logsum) + np.log(n) + 1.0))
    if n > 1:
        check_stats(acc.get(), x, post64, e, "sparse n = %d D = %d" % (n, D))
    else:   # one Gaussian per frame: the posterior is exactly 1 and the sums are those of the frames
        frame = np.arange(len(x))
        want = T.acc_stats(x, frame, sel[:, 0], np.ones(len(x), F), G)
        n_g = np.bincount(sel[:, 0], minlength=G)
        for a, b, s in zip(acc.get(), want, T.abs_terms(x, frame, sel[:, 0], np.ones(len(x), F), G)[:3]):
            assert np.all(np.abs(a - b) <= (n_g.reshape((-1,) + (1,) * (s.ndim - 1)) * 2.0 ** -52) * s)


# ------------------------------------------------------------------------------------------------------------------- batch independence
def test_a_frame_has_the_same_bits_in_any_batch_and_a_call_repeats_itself():
    G, n, D = 130, 20, 60
    x, model, _, _ = random_model(G, D)
    dm = P.Ubm.diag(**model)
    (sel,) = dm.gselect([x], n)
    one = P.DgmmAccumulator(G, D, "mvw")
    logsum, ll = one.accumulate_gselect(dm, x, sel, return_loglikes=True)
    dense_one = P.DgmmAccumulator(G, D, "mvw")
    dense_logsum = dense_one.accumulate_dense(dm, x)
    cuts = [0, 37, 300, len(x)]
    pieces, dense_pieces = P.DgmmAccumulator(G, D, "mvw"), P.DgmmAccumulator(G, D, "mvw")
    for a, b in zip(cuts[:-1], cuts[1:]):
        ls, l = pieces.accumulate_gselect(dm, x[a:b], sel[a:b], return_loglikes=True)
        assert np.array_equal(ls.view(np.uint32), logsum[a:b].view(np.uint32)) and np.array_equal(l.view(np.uint32), ll[a:b].view(np.uint32))
        assert np.array_equal(dense_pieces.accumulate_dense(dm, x[a:b]).view(np.uint32), dense_logsum[a:b].view(np.uint32))
    again, dense_again = P.DgmmAccumulator(G, D, "mvw"), P.DgmmAccumulator(G, D, "mvw")
    again.accumulate_gselect(dm, x, sel)
    dense_again.accumulate_dense(dm, x)
    same_bits(again.get(), one.get(), "sparse, twice")
    same_bits(dense_again.get(), dense_one.get(), "dense, twice")
    # a frame's posteriors add up to 1 in both E-steps
    assert np.allclose(dense_one.get()[0].sum(), len(x), rtol=1e-5) and np.allclose(one.get()[0].sum(), len(x), rtol=1e-5)


def test_limits_are_errors_that_name_them():
    model = integer_model(70, 6)
    dm = P.Ubm.diag(**model)
    acc = P.DgmmAccumulator(70, 6, "mvw")
    x = np.zeros((3, 6), F)
    with pytest.raises(P.XvError, match="take 1 to 64"):
        acc.accumulate_gselect(dm, x, np.zeros((3, 65), np.int32))
    with pytest.raises(P.XvError, match="limit of 96"):
        P.DgmmAccumulator(2, 97, "mvw")
    with pytest.raises(P.XvError, match="name Gaussian 70; the accumulators have 70"):
        acc.accumulate(x, [(np.array([70], np.int32), np.ones(1, F))] * 3)
    with pytest.raises(P.XvError, match="names Gaussian 70; the model has 70"):
        acc.accumulate_gselect(dm, x, np.full((3, 2), 70, np.int32))
    with pytest.raises(P.XvError, match="the model has 7 components"):
        acc.accumulate_dense(P.Ubm.diag(**integer_model(7, 6)), x)
    assert not acc.get()[0].any()   # nothing was accumulated on the way


# ------------------------------------------------------------------------------------------------------------------- the recipe
def _sh(line, cwd=None):
    env = dict(os.environ, PATH=BIN + os.pathsep + os.environ.get("PATH", ""))
    return subprocess.run(["/bin/sh", "-c", line], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, cwd=cwd, timeout=300)


@pytest.fixture(scope="module")
def recipe(tmp_path_factory):
    """data/ with 12 utterances of about 500 frames of 2 columns drawn from 8 separated clusters, split in two jobs, and the feature
    strings of sid/train_diag_ubm.sh:94-95; add-deltas makes 6 columns of the 2"""
    root = tmp_path_factory.mktemp("diag_ubm")
    data, dirr = root / "data", root / "exp"
    nj, subsample = 2, 2
    for d in (data / "split2" / "1", data / "split2" / "2", dirr):
        d.mkdir(parents=True)
    rng = np.random.default_rng(42)
    centres = np.array([[-9, -9], [-9, 0], [-9, 9], [0, -6], [0, 6], [9, -9], [9, 0], [9, 9]], np.float64)
    utts = []
    for i in range(12):
        T_ = 440 + 20 * i
        lab = np.repeat(rng.integers(0, 8, T_ // 20 + 1), 20)[:T_]   # 20 frames on a cluster at a time: the deltas stay small
        utts.append(("spk%02d-a" % i, (centres[lab] + rng.normal(0, 0.7, size=(T_, 2))).astype(F)))
    vads = [(k, (rng.uniform(size=len(u)) < 0.95).astype(F)) for k, u in utts]
    kio.write_ark_matrices(str(data / "raw.ark"), utts, scp_path=str(data / "feats.scp"))
    kio.write_ark_vectors(str(data / "vad.ark"), vads, scp_path=str(data / "vad.scp"))
    for job in (1, 2):
        part = slice(6 * (job - 1), 6 * job)
        sd = data / "split2" / str(job)
        kio.write_ark_matrices(str(sd / "raw.ark"), utts[part], scp_path=str(sd / "feats.scp"))
        kio.write_ark_vectors(str(sd / "vad.ark"), vads[part], scp_path=str(sd / "vad.scp"))
    delta_opts = "--delta-window=3 --delta-order=2"
    sdata = data / "split2"
    all_feats = ("ark,s,cs:add-deltas %s scp:%s/feats.scp ark:- | apply-cmvn-sliding --norm-vars=false --center=true --cmn-window=300 ark:- ark:- | "
                 "select-voiced-frames ark:- scp,s,cs:%s/vad.scp ark:- |" % (delta_opts, data, data))
    feats = ("ark,s,cs:add-deltas %s scp:%s/JOB/feats.scp ark:- | apply-cmvn-sliding --norm-vars=false --center=true --cmn-window=300 ark:- ark:- | "
             "select-voiced-frames ark:- scp,s,cs:%s/JOB/vad.scp ark:- | subsample-feats --n=%d ark:- ark:- |" % (delta_opts, sdata, sdata, subsample))
    r = _sh(all_feats[len("ark,s,cs:"):] + " cat > %s/prepared.ark" % root)
    assert r.returncode == 0, r.stderr
    prepared = np.concatenate([m for _, m in kio.read_ark(str(root / "prepared.ark"))])
    assert prepared.shape[1] == 6 and 5500 < len(prepared) < 6500
    return dict(root=root, data=data, dir=dirr, nj=nj, all_feats=all_feats, feats=feats, prepared=prepared)


def _init(recipe, out, extra):
    # sid/train_diag_ubm.sh:105-109
    line = ('gmm-global-init-from-feats --num-threads=32 --num-frames=4096 --min-gaussian-weight=0.0001 %s "%s" %s/%s'
            % (extra, recipe["all_feats"], recipe["dir"], out))
    r = _sh(line)
    assert r.returncode == 0, r.stderr.decode()
    return r.stderr.decode(), (recipe["dir"] / out).read_bytes()


def test_init_from_feats_is_keyed_by_the_seed_matches_the_restatement_and_climbs(recipe):
    """(b): one iteration from the bit-replicated initialisation, against the restatement's float64 E-step and M-step.  The cap of
    1e-4 (of a standard deviation for the means, relative for variances and weights) is a condition, not a tuned tolerance: a numpy
    emulation of the float32 chain stayed within 6e-6 of float64 at G = 16, D = 60, T = 4096 and at G = 64, D = 24, T = 8192, and a
    wrong posterior moves these values by orders of magnitude more.  Seen on the MI355X: means 2.4e-07 of a standard deviation,
    variances 1.9e-07 and weights 6.0e-08 relative."""
    opts = "--num-gauss=8 --num-gauss-init=4 --num-iters=6"
    log, a = _init(recipe, "0.dubm", opts)
    _, b = _init(recipe, "0b.dubm", opts)
    _, c = _init(recipe, "0c.dubm", opts + " --seed=3")
    assert a == b and a != c   # (a)
    kept_line = re.search(r"Kept 4096 out of (\d+) input frames = (\S+)%\.", log)
    assert kept_line and int(kept_line.group(1)) == len(recipe["prepared"]), log
    assert [int(g) for g in re.findall(r"Splitting to (\d+) Gaussians\.", log)] == [5, 6, 7, 8] and "Wrote model to" in log
    likes = [(int(i), float(l), int(t)) for i, l, t in re.findall(r"Likelihood per frame on iteration (\d+) was (\S+) over (\d+) frames\.", log)]
    assert [i for i, _, _ in likes] == list(range(6)) and all(t == 4096 for _, _, t in likes)
    assert len(re.findall(r"Objective-function change on iteration \d+ was \S+ over \S+ frames\.", log)) == 6
    # (c): the last split follows iteration 3; from iteration 4 on the model has 8 Gaussians and EM does not lose likelihood,
    # beyond what the device's log-sums may be off by (the bound of test_dense_logsum_against_the_float64_scores, per frame)
    final = R.read_diag_gmm(a)
    kept, _ = T.sample_frames(recipe["prepared"], 4096, 0)
    model = dict(gconsts=final["gconsts"], means_invvars=final["means_invvars"], inv_vars=final["inv_vars"])
    tol = float(T.score_bound(kept, **model).max()) + 8 * U * (abs(likes[5][1]) + np.log(8) + 1.0)
    print("likelihood per frame, iteration by iteration: %s (tolerance %.3g)" % ([l for _, l, _ in likes], tol))
    assert likes[5][1] >= likes[4][1] - 2 * tol
    # (b)
    _, one = _init(recipe, "one.dubm", "--num-gauss=8 --num-gauss-init=8 --num-iters=1")
    got = R.read_diag_gmm(one)
    w0, mi0, iv0, _ = T.init_from_frames(kept, 8, 0)
    want, _ = T.em_iteration(kept, w0, mi0, iv0, min_gaussian_weight=0.0001)
    assert want["removed"] == [] and len(got["weights"]) == 8
    sd = 1.0 / np.sqrt(want["inv_vars"].astype(np.float64))
    mean_err = np.abs(got["means_invvars"] / got["inv_vars"] - want["means_invvars"].astype(np.float64) / want["inv_vars"]) / sd
    var_err = np.abs(got["inv_vars"] / want["inv_vars"].astype(np.float64) - 1.0)
    w_err = np.abs(got["weights"] / want["weights"].astype(np.float64) - 1.0)
    print("one iteration against the restatement: means %.3g sd, variances %.3g, weights %.3g (relative)" % (mean_err.max(), var_err.max(), w_err.max()))
    assert mean_err.max() <= 1e-4 and var_err.max() <= 1e-4 and w_err.max() <= 1e-4


def test_train_diag_ubm_lines_run_with_the_scripts_argv(recipe):
    dirr, feats, nj = recipe["dir"], recipe["feats"], recipe["nj"]
    if not (dirr / "0.dubm").exists():
        _init(recipe, "0.dubm", "--num-gauss=8 --num-gauss-init=4 --num-iters=6")

    def jobs(line):
        for job in range(1, nj + 1):
            r = _sh(line.replace("JOB", str(job)))
            assert r.returncode == 0, r.stderr.decode()
            yield r.stderr.decode()

    # :116-118
    for log in jobs('gmm-gselect --n=4 %s/0.dubm "%s" "ark:|gzip -c >%s/gselect.JOB.gz"' % (dirr, feats, dirr)):
        assert "Done 6 files, 0 with errors" in log
    assert gzip.open(str(dirr / "gselect.1.gz")).read(7) == b"spk00-a"
    likes, num_iters = [], 2
    for x in range(num_iters):
        tot, frames = 0.0, 0
        # :128-129
        for log in jobs('gmm-global-acc-stats "--gselect=ark,s,cs:gunzip -c %s/gselect.JOB.gz|" %s/%d.dubm "%s" %s/%d.JOB.acc' % (dirr, dirr, x, feats, dirr, x)):
            assert "Done 6 files; 0 with errors." in log
            m = re.search(r"Overall likelihood per frame = (\S+) over (\d+) \(weighted\) frames\.", log)
            assert m, log
            tot += float(m.group(1)) * int(m.group(2))
            frames += int(m.group(2))
        assert 2700 < frames < 3300
        likes.append(tot / frames)
        # :131-137
        opt = "--remove-low-count-gaussians=%s" % ("true" if x + 1 == num_iters else "false")
        r = _sh('gmm-global-est %s --min-gaussian-weight=0.0001 %s/%d.dubm "gmm-global-sum-accs - %s/%d.*.acc|" %s/%d.dubm' % (opt, dirr, x, dirr, x, dirr, x + 1))
        assert r.returncode == 0, r.stderr.decode()
        log = r.stderr.decode()
        assert "Summed 2 stats" in log and re.search(r"Overall objective function improvement is \S+ per frame over \S+ frames", log), log
    print("likelihood per frame, pass by pass: %s" % likes)
    assert likes[1] >= likes[0] - 1e-3, likes
    # (d): the same first pass unsplit.  The .acc files differ by their float roundings (each part once, the sum once more: a few
    # 2^-24 relative), which var = var_acc / occ - mean^2 amplifies by (mean^2 + var) / var and the mean by nothing.
    whole = ("ark,s,cs:" + recipe["all_feats"][len("ark,s,cs:"):] + " subsample-feats --n=2 ark:- ark:- |")
    r = _sh('gmm-gselect --n=4 %s/0.dubm "%s" "ark:|gzip -c >%s/gselect.all.gz"' % (dirr, whole, dirr))
    assert r.returncode == 0, r.stderr.decode()
    r = _sh('gmm-global-acc-stats "--gselect=ark,s,cs:gunzip -c %s/gselect.all.gz|" %s/0.dubm "%s" %s/whole.acc' % (dirr, dirr, whole, dirr))
    assert r.returncode == 0 and b"Done 12 files; 0 with errors." in r.stderr, r.stderr.decode()
    r = _sh("gmm-global-est --remove-low-count-gaussians=false --min-gaussian-weight=0.0001 %s/0.dubm %s/whole.acc %s/1w.dubm" % (dirr, dirr, dirr))
    assert r.returncode == 0, r.stderr.decode()
    a, b = R.read_diag_gmm((dirr / "1.dubm").read_bytes()), R.read_diag_gmm((dirr / "1w.dubm").read_bytes())
    mean = a["means_invvars"].astype(np.float64) / a["inv_vars"]
    var = 1.0 / a["inv_vars"].astype(np.float64)
    amp = (mean * mean + var) / var
    assert np.all(np.abs(b["inv_vars"] / a["inv_vars"].astype(np.float64) - 1.0) <= 8 * U * amp)
    assert np.all(np.abs(b["means_invvars"] / b["inv_vars"].astype(np.float64) - mean) <= 8 * U * (np.abs(mean) + np.sqrt(var)))
    assert np.all(np.abs(b["weights"] / a["weights"].astype(np.float64) - 1.0) <= 8 * U)
    # :142, and (e): the model feeds the next stage
    os.rename(str(dirr / ("%d.dubm" % num_iters)), str(dirr / "final.dubm"))
    r = _sh("gmm-global-to-fgmm %s/final.dubm %s/0.ubm" % (dirr, dirr))
    assert r.returncode == 0 and b"Written full GMM to" in r.stderr, r.stderr
    r = _sh('gmm-gselect --n=4 %s/final.dubm "%s" ark:/dev/null' % (dirr, feats.replace("JOB", "1")))
    assert r.returncode == 0 and b"Done 6 files, 0 with errors" in r.stderr, r.stderr.decode()
    final = R.read_diag_gmm((dirr / "final.dubm").read_bytes())
    assert 1 <= len(final["weights"]) <= 8 and abs(float(final["weights"].sum()) - 1.0) < 1e-6 and np.all(np.isfinite(final["gconsts"]))


def test_acc_stats_words_and_counts_what_it_skips(tmp_path):
    """gmm-global-acc-stats on five utterances, one usable: a key the --gselect table does not have, a selection a frame short
    and one of another width are warned and counted; a matrix without rows is warned and not counted."""
    Gm, D = 4, 6
    m = integer_model(Gm, D)
    (tmp_path / "0.dubm").write_bytes(R.diag_gmm_bytes(np.full(Gm, 1.0 / Gm, F), m["means_invvars"], m["inv_vars"], True))
    x = np.random.default_rng(61).integers(-4, 5, (12, D)).astype(F)
    kio.write_ark_matrices(str(tmp_path / "f.ark"), [("a", x[0:3]), ("b", x[3:5]), ("c", x[5:8]), ("d", x[8:12]), ("e", x[:0])])
    (tmp_path / "f.gs").write_bytes(R.gselect_table_bytes([("a", [[0, 1]] * 3), ("c", [[1, 2]] * 2), ("d", [[3]] * 4)], True))
    r = _sh("gmm-global-acc-stats --gselect=ark,s,cs:f.gs 0.dubm ark,s,cs:f.ark f.acc", cwd=str(tmp_path))
    log = r.stderr.decode()
    assert r.returncode == 0, log
    for text in (") No gselect information for utterance b\n", ") gselect information for utterance c has wrong size 2 vs. 3\n",
                 ") The Gaussian selection of utterance d does not have the 2 indices per frame of the utterances before it (skipping utterance)\n",
                 ") Empty feature matrix for utterance e\n", ") Done 1 files; 3 with errors.\n"):
        assert log.count(text) == 1, log
    assert re.search(r"Overall likelihood per frame = \S+ over 3 \(weighted\) frames\.", log), log


def test_init_from_feats_stops_at_an_entry_it_cannot_read(tmp_path):
    x = np.random.default_rng(62).normal(size=(8, 3)).astype(F)
    offs = kio.write_ark_matrices(str(tmp_path / "f.ark"), [("a", x[:4]), ("c", x[4:])])
    (tmp_path / "f.scp").write_text("a f.ark:%d\nb gone.ark:7\nc f.ark:%d\n" % (offs["a"], offs["c"]))
    r = _sh("gmm-global-init-from-feats --num-gauss=2 --num-iters=1 scp:f.scp out.dubm", cwd=str(tmp_path))
    log = r.stderr.decode()
    assert r.returncode == 255, log
    assert log.count("ERROR (gmm-global-init-from-feats) Failed to read features for key b: cannot open gone.ark for reading") == 1, log
    assert not (tmp_path / "out.dubm").exists()
