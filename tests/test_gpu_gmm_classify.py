"""GPU tests of the GMM classifiers (csrc/gmm_classify_kernels.hip, csrc/gmm_classify.cc): the second-stage selection against the
float64 restatement (tests/gmm_classify_ref.py) exactly on integer models, its ties, random models within the summation bound,
the frame likelihoods against the posteriors' log-sum bit for bit, batch independence, the limits, and the command lines of
sid/gender_id.sh:88-118, sid/music_id.sh:73-104 and sid/compute_vad_decision_gmm.sh:91-127 through real pipes."""
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import gmm_classify_ref as C
import helpers as H
import ubm_ref as R
from oracle import kaldi_io as kio

pytestmark = pytest.mark.gpu
P = H.pkg()
BIN = os.path.join(H.ROOT, H.PKG_NAME, "bin")

_HDR = open(os.path.join(H.ROOT, H.PKG_NAME, "csrc", "gmm_classify_kernels.h")).read()
W = int(re.search(r"kRerankFramesPerBlock = (\d+);", _HDR).group(1))
FRAMES = [1, W - 1, W, W + 1, 2 * W + 3]
# (Gaussians, n_in, n_out, D)
EXACT = [(1, 1, 1, 1), (20, 20, 3, 23), (21, 20, 20, 60), (65, 64, 1, 23), (65, 64, 64, 60), (65, 63, 50, 69), (30, 10, 50, 60)]
U = 2.0 ** -24


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ------------------------------------------------------------------------------------------------------------------- exact
@pytest.mark.parametrize("G,n_in,n_out,D", EXACT)
def test_integer_models_rerank_exactly(G, n_in, n_out, D):
    full = C.integer_full_model(G, D)
    fm = P.Ubm.full(**full)
    rng = np.random.default_rng(G + n_in + n_out + D)
    for T in FRAMES:
        x = rng.integers(-2, 3, (T, D)).astype(np.float32)
        pre = np.stack([rng.permutation(G)[:n_in] for _ in range(T)]).astype(np.int32)   # any order inside a frame, no repeats
        # every product and every partial sum is a multiple of 2^-10 below 2^14 in magnitude: 24 bits, whatever the order
        assert R.full_loglikes(x, sel=pre, absolute=True, **full).max() * 2.0 ** 10 < 2.0 ** 24
        scores = R.full_loglikes(x, sel=pre, **full)
        assert all(len(np.unique(row)) == n_in for row in scores), "the restatement has a tie"
        want_idx, want_ll = C.rerank(scores, pre, n_out)
        (idx,), (ll,) = fm.rerank([x], [pre], n_out, return_loglikes=True)
        assert idx.shape == (T, min(n_out, n_in)) and idx.dtype == np.int32
        assert np.array_equal(idx, want_idx), (T, "indices")
        assert np.array_equal(ll.astype(np.float64), want_ll), (T, "log-likelihoods")
        (only_idx,) = fm.rerank([x], [pre], n_out)
        assert np.array_equal(only_idx, idx)


# ------------------------------------------------------------------------------------------------------------------- ties
def test_equal_scores_go_by_index_then_slot():
    """Gaussians 1 and 4 are one Gaussian twice, and the preselection names 2 and 4 twice: equal scores come out with the lower index
    first, and a repeated index as often as it was named."""
    G, D = 6, 5
    full = C.integer_full_model(G, D)
    for k in full:
        full[k] = full[k].copy()
        full[k][4] = full[k][1]
    fm = P.Ubm.full(**full)
    rng = np.random.default_rng(1)
    for T in FRAMES:
        x = rng.integers(-2, 3, (T, D)).astype(np.float32)
        pre = np.tile(np.array([4, 2, 1, 2, 0, 4], np.int32), (T, 1))
        scores = R.full_loglikes(x, sel=pre, **full)
        assert np.array_equal(scores[:, 0], scores[:, 2]) and np.array_equal(scores[:, 0], scores[:, 5])
        for n_out in (6, 4, 1):
            want_idx, want_ll = C.rerank(scores, pre, n_out)
            (idx,), (ll,) = fm.rerank([x], [pre], n_out, return_loglikes=True)
            assert np.array_equal(idx, want_idx) and np.array_equal(ll.astype(np.float64), want_ll), (T, n_out)
        (idx,) = fm.rerank([x], [pre], 6)
        for row in idx.tolist():
            assert sorted(row) == [0, 1, 2, 2, 4, 4]
            assert row.index(1) + 1 == row.index(4) and row[row.index(4) + 1] == 4, "1, then 4 twice"
            assert row[row.index(2) + 1] == 2


def test_a_minus_infinite_gconst_is_ranked_last():
    G, D = 8, 5
    full = C.integer_full_model(G, D)
    full["gconsts"] = full["gconsts"].copy()
    full["gconsts"][[3, 5]] = -np.inf
    fm = P.Ubm.full(**full)
    rng = np.random.default_rng(2)
    for T in FRAMES:
        x = rng.integers(-2, 3, (T, D)).astype(np.float32)
        pre = np.tile(np.array([5, 0, 7, 3, 1, 6], np.int32), (T, 1))
        with np.errstate(invalid="ignore"):
            scores = R.full_loglikes(x, sel=pre, **full)
        assert np.all(np.isneginf(scores[:, [0, 3]]))
        want_idx, want_ll = C.rerank(scores, pre, 6)
        (idx,), (ll,) = fm.rerank([x], [pre], 6, return_loglikes=True)
        assert np.array_equal(idx, want_idx) and np.array_equal(ll.astype(np.float64), want_ll)
        assert np.all(idx[:, 4] == 3) and np.all(idx[:, 5] == 5) and np.all(np.isneginf(ll[:, 4:])) and np.all(np.isfinite(ll[:, :4]))
        (idx4,) = fm.rerank([x], [pre], 4)
        assert not np.isin(idx4, [3, 5]).any()


# ------------------------------------------------------------------------------------------------------------------- random
RANDOM = [(70, 20, 5, 23), (133, 30, 30, 60)]
T_RANDOM = 16 * W + 3


@functools.lru_cache(maxsize=None)
def random_case(G, n_in, D):
    """a random model, frames around its means, the first-stage selection of the restatement (the model's diagonal image), and for
    every (frame, slot): the float64 score and the summation bound gamma_m S, m - 3 = D^2 + D + 1 (test_gpu_ubm.py)"""
    w, means, b, ic = R.random_full_model(177 + G + D, G, D, spread=1.0)
    full = dict(gconsts=R.full_gconsts(w, b, ic).astype(np.float32), means_invcovars=b, inv_covars=ic)
    gc_d, mi, iv = R.fgmm_to_gmm(w, b, ic)
    x = R.frames_around(15 + D, means, T_RANDOM, noise=1.0)
    pre = R.gselect(R.diag_loglikes(x, gc_d, mi, iv), n_in)
    scores = R.full_loglikes(x, sel=pre, **full)
    eps = R.gamma(D * D + D + 1 + 3) * R.full_loglikes(x, sel=pre, absolute=True, **full)
    for a in (x, pre, scores, eps):
        a.setflags(write=False)
    return full, x, pre, scores, eps


@pytest.mark.parametrize("G,n_in,n_out,D", RANDOM)
def test_random_models_rank_their_own_scores(G, n_in, n_out, D):
    full, x, pre, scores, eps = random_case(G, n_in, D)
    fm = P.Ubm.full(**full)
    _, (dev_ll,), _ = fm.post([x], [pre], return_details=True)
    err = np.abs(dev_ll - scores)
    print("worst error / bound %.3g" % float((err / eps).max()))
    assert np.all(err <= eps)
    (idx,), (ll,) = fm.rerank([x], [pre], n_out, return_loglikes=True)
    want_idx, want_ll = C.rerank(dev_ll, pre, n_out)
    assert np.array_equal(idx, want_idx)
    assert np.array_equal(_bits(ll), _bits(want_ll)), "a (frame, slot) score is the one the posteriors are made from"


# ------------------------------------------------------------------------------------------------------------------- frame likes
@pytest.mark.parametrize("G,n_in,n_out,D", RANDOM)
def test_frame_likes_are_the_posteriors_logsum(G, n_in, n_out, D):
    full, x, pre, scores, eps = random_case(G, n_in, D)
    fm = P.Ubm.full(**full)
    _, _, (logsum,) = fm.post([x], [pre], min_post=0.0, return_details=True)
    (likes,) = fm.frame_likes([x], [pre])
    assert likes.dtype == np.float32 and likes.shape == (len(x),)
    assert np.array_equal(_bits(likes), _bits(logsum))
    want = C.logsumexp(scores)
    # log-sum-exp is 1-Lipschitz in the largest score error; then n rounded expf terms in [0, 1], one logf and one add
    bound = eps.max(1) + (n_in + 4) * U * (1.0 + np.abs(want))
    err = np.abs(likes.astype(np.float64) - want)
    print("worst error / bound %.3g" % float((err / bound).max()))
    assert np.all(err <= bound)
    (avg,) = fm.frame_likes([x], [pre], average=True)
    assert avg.dtype == np.float32 and _bits(avg) == _bits(C.average_like(likes))


def test_dense_frame_likes_are_the_identity_selection():
    D = 23
    w, means, b, ic = R.random_full_model(41, 20, D, spread=1.0)
    fm = P.Ubm.full(R.full_gconsts(w, b, ic).astype(np.float32), b, ic)
    for T in FRAMES:
        x = R.frames_around(T, means, T)
        ident = np.tile(np.arange(20, dtype=np.int32), (T, 1))
        (dense,) = fm.frame_likes([x])
        (sel,) = fm.frame_likes([x], [ident])
        assert np.array_equal(_bits(dense), _bits(sel)), T
    big = C.integer_full_model(65, 8)
    with pytest.raises(P.XvError, match="limit of 64"):
        P.Ubm.full(**big).frame_likes([np.zeros((3, 8), np.float32)])


# ------------------------------------------------------------------------------------------------------------------- batches
def test_an_utterance_has_the_same_bytes_alone_and_in_a_batch():
    G, n_in, n_out, D = RANDOM[0]
    full, x_all, pre_all, _, _ = random_case(G, n_in, D)
    fm = P.Ubm.full(**full)
    rng = np.random.default_rng(9)
    lens = [7, 3 * W + 1, 2, 2 * W, 19]
    for u, T in enumerate(FRAMES):
        x, pre = x_all[u:u + T], pre_all[u:u + T]
        k = u % 5
        xs, pres = [], []
        for j, r in enumerate(lens):
            if j == k:
                xs.append(x)
                pres.append(pre)
            else:
                xs.append(rng.normal(0.0, 3.0, size=(r, D)).astype(np.float32))
                pres.append(rng.integers(0, G, (r, n_in)).astype(np.int32))
        assert len({len(a) for a in xs}) == 5
        (idx,), (ll,) = fm.rerank([x], [pre], n_out, return_loglikes=True)
        idx_b, ll_b = fm.rerank(xs, pres, n_out, return_loglikes=True)
        assert idx.tobytes() == idx_b[k].tobytes() and ll.tobytes() == ll_b[k].tobytes(), T
        (likes,) = fm.frame_likes([x], [pre])
        assert likes.tobytes() == fm.frame_likes(xs, pres)[k].tobytes(), T
        assert fm.frame_likes([x], [pre], average=True)[0].tobytes() == fm.frame_likes(xs, pres, average=True)[k].tobytes(), T


# ------------------------------------------------------------------------------------------------------------------- limits
def test_limits_are_errors_that_name_them():
    G, D = 65, 8
    full = C.integer_full_model(G, D)
    fm = P.Ubm.full(**full)
    x = np.zeros((3, D), np.float32)
    with pytest.raises(P.XvError, match="limit of 64"):
        fm.rerank([x], [np.zeros((3, 65), np.int32)], 5)
    with pytest.raises(P.XvError, match="limit of 64"):
        fm.frame_likes([x], [np.zeros((3, 65), np.int32)])
    bad = np.zeros((3, 4), np.int32)
    bad[2, 3] = G
    with pytest.raises(P.XvError, match="names Gaussian 65; the model has 65"):
        fm.rerank([x], [bad], 2)
    with pytest.raises(P.XvError, match="names Gaussian 65; the model has 65"):
        fm.frame_likes([x], [bad])
    dm = P.Ubm.diag(np.zeros(G, np.float32), np.zeros((G, D), np.float32), np.ones((G, D), np.float32))
    with pytest.raises(P.XvError, match="full-covariance model is needed"):
        dm.rerank([x], [np.zeros((3, 4), np.int32)], 2)
    with pytest.raises(P.XvError, match="full-covariance model is needed"):
        dm.frame_likes([x], [np.zeros((3, 4), np.int32)])
    with pytest.raises(P.XvError, match="at least 1"):
        fm.rerank([x], [np.zeros((3, 4), np.int32)], 0)


# ------------------------------------------------------------------------------------------------------------------- the recipes
def _sh(line, cwd=None):
    env = dict(os.environ, PATH=BIN + os.pathsep + os.environ.get("PATH", ""))
    return subprocess.run(["/bin/sh", "-c", line], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, cwd=cwd, timeout=300)


G_R, D_R = 21, 12
KEYS = ["spk1-a", "spk2-a"]


@pytest.fixture(scope="module")
def recipe(tmp_path_factory):
    """data/split1/1 with two utterances of 4 static features (about 40 and 70 frames) and an energy VAD, and random full models of
    21 Gaussians on the 12 columns --delta-order=2 makes of them; the prepared features are the tools' own."""
    top = tmp_path_factory.mktemp("classify")
    sdata = top / "data" / "split1" / "1"
    sdata.mkdir(parents=True)
    rng = np.random.default_rng(6)
    lens = dict(zip(KEYS, (41, 70)))
    utts = [(k, rng.normal(0.0, 2.0, size=(lens[k], 4)).astype(np.float32)) for k in KEYS]
    vads = [(k, (rng.uniform(size=lens[k]) < 0.8).astype(np.float32)) for k in KEYS]
    kio.write_ark_matrices(str(sdata / "raw.ark"), utts, scp_path=str(sdata / "feats.scp"))
    kio.write_ark_vectors(str(sdata / "vad.ark"), vads, scp_path=str(sdata / "vad.scp"))
    models = {}
    for i, name in enumerate(("ubm", "male", "female", "speech", "music", "noise")):
        d = top / name
        d.mkdir()
        w, _, b, ic = R.random_full_model(50 + i, G_R, D_R, spread=1.0)
        (d / "final.ubm").write_bytes(R.full_gmm_bytes(w, b, ic, True))
        (d / "delta_opts").write_text("--delta-order=2\n")
        models[name] = dict(gconsts=P.fgmm_gconsts(w, b, ic), means_invcovars=b, inv_covars=ic)   # what a tool computes when it reads the file
    base = ("ark,s,cs:add-deltas --delta-order=2 scp:%s/feats.scp ark:- | apply-cmvn-sliding --norm-vars=false --center=true --cmn-window=300 ark:- ark:- |"
            % sdata)
    voiced = base + " select-voiced-frames ark:- scp,s,cs:%s/vad.scp ark:- |" % sdata
    prepared = {}
    for name, feats in (("voiced", voiced), ("all", base)):
        r = _sh(feats[len("ark,s,cs:"):] + " cat > %s/%s.ark" % (top, name))
        assert r.returncode == 0, r.stderr
        prepared[name] = dict(kio.read_ark(str(top / (name + ".ark"))))
        assert all(prepared[name][k].shape[1] == D_R for k in KEYS)
    assert [prepared["voiced"][k].shape[0] for k in KEYS] == [int(v.sum()) for _, v in vads]
    return dict(top=top, sdata=sdata, models=models, voiced=voiced, all=base, prepared=prepared, vads=dict(vads))


def _bound(x, model, sel):
    """per (frame, slot): the summation bound of the device's score"""
    return R.gamma(D_R * D_R + D_R + 1 + 3) * R.full_loglikes(x, sel=sel, absolute=True, **model)


def _check_gselect(got, first, x_by_key, model, n_out):
    """fgmm-gselect's table against the restatement's ranking of the first stage's selection; the float64 scores of a frame must be
    further apart than the device's error can bridge, which is a property of the data"""
    assert [k for k, _ in got] == KEYS and [k for k, _ in first] == KEYS
    for (k, sel), (_, pre) in zip(got, first):
        pre = np.array(pre, np.int32)
        scores = R.full_loglikes(x_by_key[k], sel=pre, **model)
        eps = _bound(x_by_key[k], model, pre).max(1)
        gaps = np.diff(np.sort(scores, axis=1), axis=1).min(1) if pre.shape[1] > 1 else np.full(len(pre), np.inf)
        assert np.all(gaps > 2 * eps), "the data has a near tie: choose another seed"
        want_idx, _ = C.rerank(scores, pre, n_out)
        assert np.array_equal(np.array(sel, np.int32), want_idx), k


def _check_likes(got, x, model, sel):
    """float32 frame likelihoods against the float64 restatement, within the bound of the frame-likes test"""
    sel = np.array(sel, np.int32)
    want = C.logsumexp(R.full_loglikes(x, sel=sel, **model))
    bound = _bound(x, model, sel).max(1) + (sel.shape[1] + 4) * U * (1.0 + np.abs(want))
    assert got.shape == want.shape and np.all(np.abs(got.astype(np.float64) - want) <= bound)
    return want, bound


def test_gender_id_lines_run_with_the_recipes_argv(recipe):
    top, feats, x = recipe["top"], recipe["voiced"], recipe["prepared"]["voiced"]
    d = top / "gender"
    d.mkdir()
    ubmdir, male, female = top / "ubm", top / "male", top / "female"
    # gender_id.sh:68-70
    for m in (ubmdir, male, female):
        r = _sh("fgmm-global-info --print-args=false %s/final.ubm | grep gaussians | awk '{print $NF}'" % m)
        assert r.stdout.strip() == b"21", r.stderr
    # gender_id.sh:83, 94-97 with num_gselect1 = 5, num_gselect2 = 3
    r = _sh('fgmm-global-to-gmm %s/final.ubm %s/final.dubm && gmm-gselect --n=5 %s/final.dubm "%s" ark:- | tee %s/first.ark | '
            'fgmm-gselect --gselect=ark,s,cs:- --n=3 %s/final.ubm "%s" "ark:|gzip -c >%s/gselect.1.gz"' % (ubmdir, d, d, feats, d, ubmdir, feats, d))
    assert r.returncode == 0, r.stderr
    log = r.stderr.decode()
    assert re.search(r"LOG \(fgmm-gselect.*Done 2 files, 0 with errors, average UBM log-likelihood is \S+ over \d+ frames\.", log), log
    assert "pointless" not in log
    r = _sh("gunzip -c %s/gselect.1.gz" % d)
    second = R.read_gselect_table(r.stdout)
    first = R.read_gselect_table((d / "first.ark").read_bytes())
    _check_gselect(second, first, x, recipe["models"]["ubm"], 3)
    # the log's average: the float64 mean of the log-sum-exp over the kept scores
    m = re.search(r"LOG \(fgmm-gselect.*average UBM log-likelihood is (\S+) over (\d+) frames", log)   # not gmm-gselect's line
    tot = np.concatenate([C.logsumexp(R.full_loglikes(x[k], sel=np.array(s, np.int32), **recipe["models"]["ubm"])) for k, s in second])
    eps = np.concatenate([_bound(x[k], recipe["models"]["ubm"], np.array(s, np.int32)).max(1) for k, s in second])
    # the device's scores are within eps of these, and the log line prints six significant digits
    assert int(m.group(2)) == len(tot) and abs(float(m.group(1)) - tot.mean()) <= eps.mean() + 5e-6 * abs(tot.mean())
    # gender_id.sh:107-116
    avg = {}
    for name, mdir in (("male", male), ("female", female)):
        r = _sh('fgmm-global-get-frame-likes --average=true "--gselect=ark,s,cs:gunzip -c %s/gselect.1.gz|" %s/final.ubm "%s" ark,t:%s/%s_logprob.1'
                % (d, mdir, feats, d, name))
        assert r.returncode == 0, r.stderr
        assert b"Done 2 files; 0 with errors." in r.stderr
        got = C.read_float_table((d / ("%s_logprob.1" % name)).read_bytes())
        assert [k for k, _ in got] == KEYS
        for (k, v), (_, sel) in zip(got, second):
            want = C.logsumexp(R.full_loglikes(x[k], sel=np.array(sel, np.int32), **recipe["models"][name]))
            bound = _bound(x[k], recipe["models"][name], np.array(sel, np.int32)).max(1) + (3 + 4) * U * (1.0 + np.abs(want))
            assert abs(float(v) - want.mean()) <= bound.mean() + U * abs(want.mean()), (name, k)
            # the same bits as the library gives for the utterance alone: the average does not depend on the batch
            fm = P.Ubm.full(**recipe["models"][name])
            assert _bits(v) == _bits(fm.frame_likes([x[k]], [np.array(sel, np.int32)], average=True)[0])
            avg[(name, k)] = (want.mean(), bound.mean())
    # gender_id.sh:121-140 on the two text tables
    r = _sh("for j in 1; do cat male_logprob.$j; done > male_logprob; for j in 1; do cat female_logprob.$j; done > female_logprob; "
            "paste male_logprob female_logprob | awk '{if ($1 != $3) { print >/dev/stderr \"Sorting mismatch\"; exit(1);  } print $1, $2, $4;}' >logprob && "
            "cat logprob | awk -v pmale=0.5 '{lratio = log(pmale/(1-pmale))+$2-$3; print $1, 1/(1+exp(-lratio));}' >ratio && "
            "cat ratio | awk '{if ($2 > 0.5) { print $1, \"m\"; } else { print $1, \"f\"; }}' > utt2gender", cwd=str(d))
    assert r.returncode == 0, r.stderr
    want = []
    for k in KEYS:
        lratio = avg[("male", k)][0] - avg[("female", k)][0]
        assert abs(lratio) > 2 * (avg[("male", k)][1] + avg[("female", k)][1]) + 1e-6, "the data does not decide: choose another seed"
        want.append("%s %s" % (k, "m" if lratio > 0 else "f"))
    assert (d / "utt2gender").read_text().splitlines() == want
    # the averages as a binary BaseFloat table, read back by scale-post
    r = _sh('fgmm-global-get-frame-likes --average=true "--gselect=ark,s,cs:gunzip -c %s/gselect.1.gz|" %s/final.ubm "%s" ark:%s/male.bin'
            % (d, male, feats, d))
    assert r.returncode == 0, r.stderr
    binary = C.read_float_table((d / "male.bin").read_bytes())
    assert binary == C.read_float_table((d / "male_logprob.1").read_bytes())
    post = [(k, [[(1, 1.0)]]) for k in KEYS]
    (d / "post.ark").write_bytes(R.post_table_bytes(post, True))
    r = _sh("scale-post ark:%s/post.ark ark:%s/male.bin ark,t:-" % (d, d))
    assert r.returncode == 0, r.stderr
    got = R.read_post_table(r.stdout)   # text: nine significant digits, which name one float32
    assert [(k, [[(i, np.float32(p)) for i, p in f] for f in fr]) for k, fr in got] == [(k, [[(1, s)]]) for k, s in binary]


def test_music_id_lines_run_with_the_recipes_argv(recipe):
    top, feats, x = recipe["top"], recipe["voiced"], recipe["prepared"]["voiced"]
    d = top / "music_id"
    d.mkdir()
    # music_id.sh:61-66, 74-84, 95-104 with num_gselect = 5: the second stage keeps what the first selected, sorted by the full model
    for name in ("music", "speech"):
        mdir = top / name
        r = _sh('fgmm-global-to-gmm %s/final.ubm %s/%s_final.dubm && gmm-gselect --n=5 %s/%s_final.dubm "%s" ark:- | tee %s/%s_first.ark | '
                'fgmm-gselect --gselect=ark,s,cs:- --n=5 %s/final.ubm "%s" "ark:|gzip -c >%s/%s_gselect.1.gz"'
                % (mdir, d, name, d, name, feats, d, name, mdir, feats, d, name))
        assert r.returncode == 0, r.stderr
        assert r.stderr.count(b"Gaussian selection is pointless") == 1, r.stderr   # fgmm-gselect, once for both utterances
        second = R.read_gselect_table(_sh("gunzip -c %s/%s_gselect.1.gz" % (d, name)).stdout)
        first = R.read_gselect_table((d / ("%s_first.ark" % name)).read_bytes())
        _check_gselect(second, first, x, recipe["models"][name], 5)
        assert all(sorted(a) == sorted(b) for (_, s), (_, f) in zip(second, first) for a, b in zip(s, f))
        r = _sh('fgmm-global-get-frame-likes --average=true "--gselect=ark,s,cs:gunzip -c %s/%s_gselect.1.gz|" %s/final.ubm "%s" ark,t:%s/%s_logprob.1'
                % (d, name, mdir, feats, d, name))
        assert r.returncode == 0, r.stderr
        got = C.read_float_table((d / ("%s_logprob.1" % name)).read_bytes())
        assert [k for k, _ in got] == KEYS
        for (k, v), (_, sel) in zip(got, second):
            want, bound = _check_likes(P.Ubm.full(**recipe["models"][name]).frame_likes([x[k]], [np.array(sel, np.int32)])[0], x[k],
                                       recipe["models"][name], sel)
            assert abs(float(v) - want.mean()) <= bound.mean() + U * abs(want.mean()), (name, k)
    # music_id.sh:109-126
    r = _sh("paste music_logprob.1 speech_logprob.1 | awk '{if ($1 != $3) { print >/dev/stderr \"Sorting mismatch\"; exit(1);  } print $1, $2, $4;}' >logprob && "
            "cat logprob | awk '{lratio = $2-$3; print $1, 1/(1+exp(-lratio));}' >ratio", cwd=str(d))
    assert r.returncode == 0 and [l.split()[0] for l in (d / "ratio").read_text().splitlines()] == KEYS


def test_compute_vad_decision_gmm_lines_run_with_the_recipes_argv(recipe):
    top, sdata, feats, x = recipe["top"], recipe["sdata"], recipe["all"], recipe["prepared"]["all"]
    d = top / "vad_gmm"
    d.mkdir()
    names = ("music", "speech", "noise")
    likes = {}
    # compute_vad_decision_gmm.sh:86, 95-98, 109-112 with num_gselect = 5, then 3 on the command line of the second stage
    for name in names:
        mdir = top / name
        r = _sh('fgmm-global-to-gmm %s/final.ubm %s/%s_final.dubm && gmm-gselect --n=5 %s/%s_final.dubm "%s" ark:- | '
                'fgmm-gselect --gselect=ark,s,cs:- --n=3 %s/final.ubm "%s" "ark:|gzip -c >%s/%s_gselect.1.gz" && '
                'fgmm-global-get-frame-likes --average=false "--gselect=ark,s,cs:gunzip -c %s/%s_gselect.1.gz|" %s/final.ubm "%s" ark:%s/%s_logprob.1.ark'
                % (mdir, d, name, d, name, feats, mdir, feats, d, name, d, name, mdir, feats, d, name))
        assert r.returncode == 0, r.stderr
        assert b"Done 2 files; 0 with errors." in r.stderr
        sel = R.read_gselect_table(_sh("gunzip -c %s/%s_gselect.1.gz" % (d, name)).stdout)
        got = C.read_vector_table((d / ("%s_logprob.1.ark" % name)).read_bytes())
        assert [k for k, _ in got] == KEYS
        for (k, v), (_, s) in zip(got, sel):
            assert len(s) == len(x[k]) and all(len(row) == 3 for row in s)
            _check_likes(v, x[k], recipe["models"][name], s)
            assert _bits(v).tolist() == _bits(P.Ubm.full(**recipe["models"][name]).frame_likes([x[k]], [np.array(s, np.int32)])[0]).tolist()
            likes[(name, k)] = v
    # compute_vad_decision_gmm.sh:116-119 with the script's defaults (no map, no priors), then with both
    frame_likes = " ".join("ark:%s/%s_logprob.1.ark" % (d, n) for n in names)
    r = _sh("compute-vad-from-frame-likes --map= --priors= %s ark,scp:%s/vad_gmm_data.1.ark,%s/vad_gmm_data.1.scp" % (frame_likes, d, d))
    assert r.returncode == 0, r.stderr
    got = C.read_vector_table((d / "vad_gmm_data.1.ark").read_bytes())
    for k, v in got:
        assert np.array_equal(v, C.vad_from_frame_likes([likes[(n, k)] for n in names]))
    assert [k for k, _ in got] == KEYS
    (d / "map").write_text("0 2\n1 1\n2 0\n")
    r = _sh("compute-vad-from-frame-likes --map=%s/map --priors=0.2,0.6,0.2 %s ark,scp:%s/vad_gmm_data.1.ark,%s/vad_gmm_data.1.scp" % (d, frame_likes, d, d))
    assert r.returncode == 0, r.stderr
    got = C.read_vector_table((d / "vad_gmm_data.1.ark").read_bytes())
    for k, v in got:
        assert np.array_equal(v, C.vad_from_frame_likes([likes[(n, k)] for n in names], [0.2, 0.6, 0.2], [2, 1, 0]))
    # compute_vad_decision_gmm.sh:123-127
    triples = [(0, 0, 0), (0, 1, 0), (0, 2, 0), (1, 0, 0), (1, 1, 1), (1, 2, 2)]
    (d / "merge_map").write_text("".join("%d %d %d\n" % t for t in triples))
    r = _sh("merge-vads --map=%s/merge_map scp:%s/vad.scp scp:%s/vad_gmm_data.1.scp ark,scp:%s/vad_merged_data.1.ark,%s/vad_merged_data.1.scp"
            % (d, sdata, d, d, d))
    assert r.returncode == 0, r.stderr
    merged = C.read_vector_table((d / "vad_merged_data.1.ark").read_bytes())
    for (k, v), (_, g) in zip(merged, got):
        assert np.array_equal(v, C.merge_vads(recipe["vads"][k], g, triples))


def test_the_tools_refuse_what_the_device_does_not_take(recipe, tmp_path):
    top, feats = recipe["top"], recipe["voiced"]
    w, _, b, ic = R.random_full_model(3, 65, D_R, spread=1.0)
    (tmp_path / "big.ubm").write_bytes(R.full_gmm_bytes(w, b, ic, True))
    for tool in ("fgmm-gselect", "fgmm-global-get-frame-likes"):
        r = _sh('%s %s/big.ubm "%s" ark:/dev/null' % (tool, tmp_path, feats))
        assert r.returncode == 255 and b"limit of 64" in r.stderr and b"--gselect" in r.stderr, r.stderr
    # without --gselect a model the device takes whole is ranked whole: every Gaussian, best first, and --n above it warns
    r = _sh('fgmm-gselect --n=50 %s/ubm/final.ubm "%s" ark,t:-' % (top, feats))
    assert r.returncode == 0, r.stderr
    assert r.stderr.count(b"Gaussian selection is pointless") == 1
    sel = R.read_gselect_table(r.stdout)
    assert [k for k, _ in sel] == KEYS and all(sorted(row) == list(range(G_R)) for _, s in sel for row in s)
    r1 = _sh('fgmm-global-get-frame-likes %s/ubm/final.ubm "%s" ark:-' % (top, feats))
    assert r1.returncode == 0, r1.stderr
    fm = P.Ubm.full(**recipe["models"]["ubm"])
    for k, v in C.read_vector_table(r1.stdout):
        assert np.array_equal(_bits(v), _bits(fm.frame_likes([recipe["prepared"]["voiced"][k]])[0]))
    # a missing selection, a wrong frame count, a ragged selection and a wrong dimension are that utterance's error
    first = R.read_gselect_table(_sh('fgmm-global-to-gmm %s/ubm/final.ubm - | gmm-gselect --n=5 - "%s" ark:-' % (top, feats)).stdout)
    (tmp_path / "missing.ark").write_bytes(R.gselect_table_bytes(first[:1], True))
    (tmp_path / "short.ark").write_bytes(R.gselect_table_bytes([(k, s[:-1] if k == KEYS[1] else s) for k, s in first], True))
    (tmp_path / "ragged.ark").write_bytes(R.gselect_table_bytes([(k, [s[0][:-1]] + s[1:] if k == KEYS[1] else s) for k, s in first], True))
    for table, words in (("missing", b"No Gaussian-selection info available for utterance spk2-a"), ("short", b"Mismatch in number of frames"),
                         ("ragged", b"does not have one length for every frame")):
        r = _sh('fgmm-gselect --n=3 --gselect=ark:%s/%s.ark %s/ubm/final.ubm "%s" ark:/dev/null' % (tmp_path, table, top, feats))
        assert r.returncode == 0 and words in r.stderr and b"Done 1 files, 1 with errors" in r.stderr, r.stderr
    r = _sh('fgmm-gselect --n=3 %s/ubm/final.ubm "%s" ark:/dev/null' % (top, feats.replace("--delta-order=2", "--delta-order=1")))
    assert r.returncode == 1 and r.stderr.count(b"Dimension mismatch for utterance") == 2 and b"Done 0 files, 2 with errors" in r.stderr
