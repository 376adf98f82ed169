"""GPU tests of the PLDA back-end (stage 7 of egs/sre/v2/run_sre10.sh:221-252): the device kernels through the C ABI
against tests/plda_ref.py, the stage itself with the recipe's own argv on a synthetic recipe, the model files, and the
errors of the five tools.  At most 5 processes of one pipe hold the GPU at a time; every subprocess has a time limit."""
import os
import re
import subprocess

import numpy as np
import pytest

import helpers as H
import plda_ref as R
from oracle import backend as B
from oracle import kaldi_io as kio

pytestmark = pytest.mark.gpu
BIN = os.path.join(H.ROOT, H.PKG_NAME, "bin")
GENDER = "female"


def _run(args, timeout=300, **kw):
    return subprocess.run(args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=timeout, **kw)


def _bash(cmd, timeout=600):
    env = dict(os.environ, PATH=BIN + os.pathsep + os.environ.get("PATH", ""))
    return subprocess.run(["bash", "-c", "set -o pipefail; " + cmd], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                          timeout=timeout, env=env)


# ------------------------------------------------------------------------------------------------ kernels, C ABI
def _ragged_segments(rng, n, n_seg):
    segs = []
    for s in range(n_seg):
        k = int(rng.integers(0, 6)) if s % 5 else 1                      # speakers of one utterance, and empty ones
        segs.append([int(i) for i in rng.integers(0, n, k)])
    return segs


@pytest.mark.parametrize("dim", [20, 150, 512, 3000])
@pytest.mark.parametrize("n", [1, 37, 5000])
def test_scatter_stats_match_the_oracle_and_are_deterministic(dim, n):
    P = H.pkg()
    rng = np.random.default_rng(dim + n)
    x = (rng.standard_normal((n, dim)) * 2 + 0.5).astype(np.float32)
    segs = [list(range(n))] if n == 1 else _ragged_segments(rng, n, max(1, n // 4))
    s_tot, sums, s_bet = P.scatter_stats(x, segs)
    r_tot, r_sums, r_bet = R.scatter_stats(x, segs)
    for got, ref in ((s_tot, r_tot), (sums, r_sums), (s_bet, r_bet)):
        assert got.shape == ref.shape
        assert np.abs(got - ref).max() <= 1e-12 * max(np.abs(ref).max(), 1e-300)
    np.testing.assert_array_equal(s_tot, s_tot.T)
    np.testing.assert_array_equal(s_bet, s_bet.T)
    again = P.scatter_stats(x, segs)
    for a, b in zip(again, (s_tot, sums, s_bet)):
        np.testing.assert_array_equal(a, b)                                 # same input, same bits
    if len(segs) > 2:
        alone = P.scatter_stats(x, [segs[1]])[1][0]
        np.testing.assert_array_equal(alone, sums[1])                      # a speaker's sum ignores the rest of the batch


def _plda_model(rng, dim):
    mean = rng.standard_normal(dim)
    t = np.linalg.qr(rng.standard_normal((dim, dim)))[0] * rng.uniform(0.5, 2.0, dim)[:, None]
    psi = np.sort(rng.uniform(0.0, 6.0, dim))[::-1]
    return mean, t, psi


@pytest.mark.parametrize("simple", [False, True])
@pytest.mark.parametrize("dim", [7, 150, 512])
def test_plda_transform_matches_the_oracle(dim, simple):
    P = H.pkg()
    rng = np.random.default_rng(dim)
    mean, t, psi = _plda_model(rng, dim)
    x = (rng.standard_normal((70, dim)) * 3).astype(np.float32)
    num = np.array([(1, 3, 17)[i % 3] for i in range(70)], np.float64)
    off = -(t @ mean)
    for normalize in (True, False):
        y, scale = P.plda_transform(x, t, off, psi, num, normalize=normalize, simple=simple)
        ry, rscale = R.transform_ivector(x, mean, t, psi, num, normalize=normalize, simple=simple)
        ulp = np.spacing(np.abs(ry).astype(np.float32))
        assert np.all(np.abs(y.astype(np.float64) - ry.astype(np.float64)) <= ulp), np.abs(y - ry).max()
        np.testing.assert_allclose(scale, rscale, rtol=1e-12)


@pytest.mark.parametrize("n_trials", [1, 255, 256, 257, 200000])
def test_plda_score_matches_the_oracle(n_trials):
    P = H.pkg()
    rng = np.random.default_rng(n_trials)
    dim = 150
    psi = np.sort(rng.uniform(0.0, 5.0, dim))[::-1]
    n_u, n_v = 40, 300
    u = rng.standard_normal((n_u, dim)).astype(np.float32)
    v = rng.standard_normal((n_v, dim)).astype(np.float32)
    num = rng.integers(1, 9, n_u).astype(np.float64)
    ks = rng.integers(0, n_u - 2, n_trials)                               # the last two speakers: no trials
    ks[: min(n_trials, 1)] = n_u - 3
    tr = np.stack([ks, rng.integers(0, n_v, n_trials)], 1)
    got = P.plda_score(u, num, v, psi, tr)
    sample = np.arange(n_trials) if n_trials <= 2000 else rng.integers(0, n_trials, 2000)
    ref = np.array([R.llr(u[tr[i, 0]], num[tr[i, 0]], v[tr[i, 1]], psi) for i in sample])
    assert np.all(np.abs(got[sample] - ref) <= 1e-9 * (1 + np.abs(ref)))
    np.testing.assert_array_equal(P.plda_score(u, num, v, psi, tr[::-1])[::-1], got)   # order-independent bits
    with pytest.raises(P.XvError, match="indexes a row that does not exist"):
        P.plda_score(u, num, v, psi, [[0, n_v]])


# ------------------------------------------------------------------------------------------------ a synthetic recipe
D_IN, LDA_DIM = 512, 150


def _speaker_model(rng):
    a = np.linalg.qr(rng.standard_normal((D_IN, D_IN)))[0]
    lb = a[:, :200] * np.sqrt(np.geomspace(1.2, 0.05, 200))[None, :]       # between-class variance in 200 directions
    c = np.linalg.qr(rng.standard_normal((D_IN, D_IN)))[0]
    lw = c * np.linspace(0.6, 1.4, D_IN)[None, :]                          # within-class noise, anisotropic
    return lb, lw, rng.standard_normal(D_IN) * 0.5


def _speaker(rng, model, n):
    lb, lw, mu = model
    y = mu + lb @ rng.standard_normal(lb.shape[1])
    return [(y + lw @ rng.standard_normal(D_IN)).astype(np.float32) for _ in range(n)]


@pytest.fixture(scope="module")
def recipe(tmp_path_factory):
    root = tmp_path_factory.mktemp("sre")
    exp, data = root / "exp", root / "data"
    rng = np.random.default_rng(2024)
    model = _speaker_model(rng)
    train, train_spk2utt = [], []
    for s in range(300):
        utts = ["tr%03d-u%d" % (s, i) for i in range(int(rng.integers(2, 11)))]
        train.extend(zip(utts, _speaker(rng, model, len(utts))))
        train_spk2utt.append(("tr%03d" % s, utts))
    enroll, enroll_spk2utt, test, trials = [], [], [], []
    for s in range(60):
        k = int(rng.integers(1, 6))
        vecs = _speaker(rng, model, k + 2)
        utts = ["en%02d-u%d" % (s, i) for i in range(k)]
        enroll.extend(zip(utts, vecs[:k]))
        enroll_spk2utt.append(("en%02d" % s, utts))
        test.extend(("te%02d-%d" % (s, i), v) for i, v in enumerate(vecs[k:]))
    for s in range(80):
        test.append(("imp%02d" % s, _speaker(rng, model, 1)[0]))
    test_keys = [k for k, _ in test]
    for s in range(60):
        for key in sorted(set(["te%02d-0" % s, "te%02d-1" % s] + list(rng.choice(test_keys, 25, replace=False)))):
            trials.append(("en%02d" % s, key, "target" if key.startswith("te%02d-" % s) else "nontarget"))
    order = rng.permutation(len(trials))
    trials = [trials[i] for i in order]
    missing = [("en99", "te00-0", "target"), ("en03", "nosuchutt", "nontarget")]
    trials_with_missing = trials[:100] + [missing[0]] + trials[100:500] + [missing[1]] + trials[500:]

    d_comb, d_enr, d_test = exp / "xvectors_sre_combined", exp / ("xvectors_sre10_enroll_coreext_c5_" + GENDER), \
        exp / ("xvectors_sre10_test_coreext_c5_" + GENDER)
    for d in (d_comb, d_enr, d_test, exp / "xvector_scores", data / "sre_combined", data / ("sre10_enroll_coreext_c5_" + GENDER),
              data / ("sre10_test_coreext_c5_" + GENDER)):
        d.mkdir(parents=True, exist_ok=True)
    kio.write_ark_vectors(str(d_comb / "xvector_sre_combined.ark"), train, scp_path=str(d_comb / "xvector_sre_combined.scp"))
    kio.write_ark_vectors(str(d_enr / "xvector.ark"), enroll, scp_path=str(d_enr / ("xvector_sre10_enroll_coreext_c5_%s.scp" % GENDER)))
    kio.write_ark_vectors(str(d_test / "xvector.ark"), test, scp_path=str(d_test / ("xvector_sre10_test_coreext_c5_%s.scp" % GENDER)))
    (data / "sre_combined" / "spk2utt").write_text("".join("%s %s\n" % (s, " ".join(u)) for s, u in train_spk2utt))
    (data / "sre_combined" / "utt2spk").write_text("".join("%s %s\n" % (u, s) for s, us in train_spk2utt for u in us))
    (data / ("sre10_enroll_coreext_c5_" + GENDER) / "spk2utt").write_text(
        "".join("%s %s\n" % (s, " ".join(u)) for s, u in enroll_spk2utt))
    (d_enr / "num_utts.ark").write_text("".join("%s %d \n" % (s, len(u)) for s, u in enroll_spk2utt))   # ivector-mean's ark,t
    (data / ("sre10_test_coreext_c5_" + GENDER) / "trials").write_text("".join("%s %s %s\n" % t for t in trials_with_missing))
    return dict(root=root, exp=str(exp), data=str(data), train=train, train_spk2utt=train_spk2utt, enroll=enroll,
                enroll_spk2utt=enroll_spk2utt, test=test, trials=trials, missing=missing)


def _oracle_stage7(r):
    """The same stage in numpy: ivector-mean, ivector-compute-lda, the PLDA training pipe, and the scoring pipes."""
    x = np.stack([v for _, v in r["train"]])
    mean_vec = B.global_mean(x)
    row = {k: i for i, (k, _) in enumerate(r["train"])}
    spk = np.empty(len(x), np.int64)
    for s, (_, utts) in enumerate(r["train_spk2utt"]):
        spk[[row[u] for u in utts]] = s
    lda = R.lda(B.subtract_global_mean(x), spk, LDA_DIM)          # the recipe's LDA reads mean-subtracted vectors
    y, _ = B.backend_chain(x, B.global_mean(x), lda, normalize=True)
    segs = [[row[u] for u in utts] for _, utts in r["train_spk2utt"]]
    pmean, pt, psi = R.plda(y.astype(np.float32), segs)
    means, counts, _, _ = B.speaker_means(r["enroll_spk2utt"], dict(r["enroll"]))
    e, _ = B.backend_chain(np.stack([m for _, m in means]), mean_vec, lda, normalize=True)
    t, _ = B.backend_chain(np.stack([v for _, v in r["test"]]), mean_vec, lda, normalize=True)
    n = np.array([counts[k] for k, _ in means], np.float64)
    u, _ = R.transform_ivector(e.astype(np.float32), pmean, pt, psi, n)
    v, _ = R.transform_ivector(t.astype(np.float32), pmean, pt, psi)
    ei = {k: i for i, (k, _) in enumerate(means)}
    ti = {k: i for i, (k, _) in enumerate(r["test"])}
    return np.array([R.llr(u[ei[a]], n[ei[a]], v[ti[b]], psi) for a, b, _ in r["trials"]])


def _stage7_commands(exp, data, gender):
    """egs/sre/v2/run_sre10.sh:224-246 without the `$train_cmd <log>` prefix, $exp / $data / $gender substituted."""
    lda_dim = LDA_DIM
    return [
        "ivector-mean scp:%(exp)s/xvectors_sre_combined/xvector_sre_combined.scp \\\n"
        "    %(exp)s/xvectors_sre_combined/mean.vec",
        "ivector-compute-lda --total-covariance-factor=0.0 --dim=%(lda_dim)d \\\n"
        "    \"ark:ivector-subtract-global-mean scp:%(exp)s/xvectors_sre_combined/xvector_sre_combined.scp ark:- |\" \\\n"
        "    ark:%(data)s/sre_combined/utt2spk %(exp)s/xvectors_sre_combined/transform.mat",
        "ivector-compute-plda ark:%(data)s/sre_combined/spk2utt \\\n"
        "    \"ark:ivector-subtract-global-mean scp:%(exp)s/xvectors_sre_combined/xvector_sre_combined.scp ark:- | transform-vec "
        "%(exp)s/xvectors_sre_combined/transform.mat ark:- ark:- | ivector-normalize-length ark:-  ark:- |\" \\\n"
        "    %(exp)s/xvectors_sre_combined/plda_lda%(lda_dim)d",
        "ivector-plda-scoring --normalize-length=true \\\n"
        "    --num-utts=ark:%(exp)s/xvectors_sre10_enroll_coreext_c5_%(gender)s/num_utts.ark \\\n"
        "    \"ivector-copy-plda --smoothing=0.0 %(exp)s/xvectors_sre_combined/plda_lda%(lda_dim)d - |\" \\\n"
        "    \"ark:ivector-mean ark:%(data)s/sre10_enroll_coreext_c5_%(gender)s/spk2utt scp:%(exp)s/xvectors_sre10_enroll_coreext_c5_%(gender)s/"
        "xvector_sre10_enroll_coreext_c5_%(gender)s.scp ark:- | ivector-subtract-global-mean %(exp)s/xvectors_sre_combined/mean.vec "
        "ark:- ark:- | transform-vec %(exp)s/xvectors_sre_combined/transform.mat ark:- ark:- | ivector-normalize-length ark:- ark:- |\" \\\n"
        "    \"ark:ivector-subtract-global-mean %(exp)s/xvectors_sre_combined/mean.vec scp:%(exp)s/xvectors_sre10_test_coreext_c5_%(gender)s/"
        "xvector_sre10_test_coreext_c5_%(gender)s.scp ark:- | transform-vec %(exp)s/xvectors_sre_combined/transform.mat ark:- ark:- | "
        "ivector-normalize-length ark:- ark:- |\" \\\n"
        "    \"cat '%(data)s/sre10_test_coreext_c5_%(gender)s/trials' | cut -d\\  --fields=1,2 |\" "
        "%(exp)s/xvector_scores/sre10_coreext_c5_scores_%(gender)s",
    ], ("paste %(data)s/sre10_test_coreext_c5_%(gender)s/trials %(exp)s/xvector_scores/sre10_coreext_c5_scores_%(gender)s | "
        "awk '{print $6, $3}' | compute-eer - 2>/dev/null")


@pytest.fixture(scope="module")
def stage7(recipe):
    subst = dict(exp=recipe["exp"], data=recipe["data"], gender=GENDER, lda_dim=LDA_DIM)
    cmds, eer_cmd = _stage7_commands(recipe["exp"], recipe["data"], GENDER)
    logs = []
    for c in cmds:
        r = _bash(c % subst)
        logs.append(r.stderr.decode())
        assert r.returncode == 0, logs[-1]
    return recipe, logs, eer_cmd % subst


def _read_scores(path):
    rows = [line.split() for line in open(path)]
    assert all(len(r) == 3 for r in rows)
    return [(a, b) for a, b, _ in rows], np.array([float(s) for _, _, s in rows])


def test_stage7_of_run_sre10_runs_with_the_recipes_argv(stage7):
    r, logs, eer_cmd = stage7
    lda_log, plda_log, score_log = logs[1], logs[2], logs[3]
    assert "2-norm of iVector mean is" in lda_log and "Read %d utterances, 0 with errors." % len(r["train"]) in lda_log
    assert ("Accumulated stats from 300 speakers (0 with no utterances), consisting of %d utterances (0 absent from input)."
            % len(r["train"])) in plda_log
    assert "Read 60 training iVectors, errors on 0" in score_log
    assert "Average renormalization scale on training iVectors was" in score_log
    assert "Read %d test iVectors." % len(r["test"]) in score_log
    assert "Mean score was" in score_log and ", standard deviation was" in score_log
    assert "Processed %d trials, 2 had errors." % len(r["trials"]) in score_log
    assert "Key en99 not present in training iVectors." in score_log
    assert "Key nosuchutt not present in test iVectors." in score_log
    keys, scores = _read_scores(os.path.join(r["exp"], "xvector_scores", "sre10_coreext_c5_scores_" + GENDER))
    assert keys == [(a, b) for a, b, _ in r["trials"]]                        # the trial file's order, minus the missing keys
    with open(os.path.join(r["exp"], "xvectors_sre_combined", "transform.mat"), "rb") as f:
        assert f.read(2) == b"\0B" and kio.read_matrix(f).shape == (LDA_DIM, D_IN + 1)
    ref = _oracle_stage7(r)
    assert np.all(np.abs(scores - ref) <= 1e-4 * (1 + np.abs(ref))), np.abs(scores - ref).max()


def test_pooled_eer_of_stage7(stage7, tmp_path):
    """run_sre10.sh:252: paste trials scores | awk '{print $6, $3}' | compute-eer - - on the trial lines that were scored
    (the recipe's trials have no missing keys; this file's lines with missing keys would shift the paste)."""
    r, _, eer_cmd = stage7
    tdir = os.path.join(r["data"], "sre10_test_coreext_c5_" + GENDER)
    os.rename(os.path.join(tdir, "trials"), os.path.join(tdir, "trials.with_missing"))
    try:
        with open(os.path.join(tdir, "trials"), "w") as f:
            f.write("".join("%s %s %s\n" % t for t in r["trials"]))
        res = _bash(eer_cmd)
    finally:
        os.replace(os.path.join(tdir, "trials.with_missing"), os.path.join(tdir, "trials"))
    assert res.returncode == 0, res.stderr.decode()
    _, scores = _read_scores(os.path.join(r["exp"], "xvector_scores", "sre10_coreext_c5_scores_" + GENDER))
    labels = [lab for _, _, lab in r["trials"]]
    tgt = [s for s, lab in zip(scores, labels) if lab == "target"]
    non = [s for s, lab in zip(scores, labels) if lab == "nontarget"]
    e, _ = R.eer(tgt, non)
    assert res.stdout.decode() == "%.4g\n" % (100.0 * e)
    assert 0.0 < e < 0.4
    ref = _oracle_stage7(r)
    e_ref, _ = R.eer([s for s, lab in zip(ref, labels) if lab == "target"], [s for s, lab in zip(ref, labels) if lab == "nontarget"])
    assert abs(e - e_ref) <= 1.0 / len(tgt) + 1e-12


# ------------------------------------------------------------------------------------------------ model files
def _score_with(stage, plda_rx, out):
    r = stage[0]
    exp, data = r["exp"], r["data"]
    cmd = ("ivector-plda-scoring --num-utts=ark:%(exp)s/xvectors_sre10_enroll_coreext_c5_%(g)s/num_utts.ark \"%(plda)s\" "
           "\"ark:ivector-mean ark:%(data)s/sre10_enroll_coreext_c5_%(g)s/spk2utt scp:%(exp)s/xvectors_sre10_enroll_coreext_c5_%(g)s/"
           "xvector_sre10_enroll_coreext_c5_%(g)s.scp ark:- | ivector-subtract-global-mean %(exp)s/xvectors_sre_combined/mean.vec "
           "ark:- ark:- | transform-vec %(exp)s/xvectors_sre_combined/transform.mat ark:- ark:- | ivector-normalize-length ark:- ark:- |\" "
           "\"ark:ivector-subtract-global-mean %(exp)s/xvectors_sre_combined/mean.vec scp:%(exp)s/xvectors_sre10_test_coreext_c5_%(g)s/"
           "xvector_sre10_test_coreext_c5_%(g)s.scp ark:- | transform-vec %(exp)s/xvectors_sre_combined/transform.mat ark:- ark:- | "
           "ivector-normalize-length ark:- ark:- |\" \"cut -d' ' -f1,2 %(data)s/sre10_test_coreext_c5_%(g)s/trials |\" %(out)s") % \
        dict(exp=exp, data=data, g=GENDER, plda=plda_rx, out=out)
    res = _bash(cmd)
    return res


def test_model_files(stage7, tmp_path):
    r = stage7[0]
    plda = os.path.join(r["exp"], "xvectors_sre_combined", "plda_lda%d" % LDA_DIM)
    base = os.path.join(r["exp"], "xvector_scores", "sre10_coreext_c5_scores_" + GENDER)
    # text model -> identical scores
    assert _run([os.path.join(BIN, "ivector-copy-plda"), "--binary=false", plda, str(tmp_path / "plda.txt")]).returncode == 0
    res = _score_with(stage7, str(tmp_path / "plda.txt"), tmp_path / "s_text")
    assert res.returncode == 0, res.stderr.decode()
    assert (tmp_path / "s_text").read_bytes() == open(base, "rb").read()
    # a model with float vectors
    mean, t, psi = R.read_plda(plda)
    R.write_plda(str(tmp_path / "plda.f"), mean, t, psi, double=False)
    res = _score_with(stage7, str(tmp_path / "plda.f"), tmp_path / "s_float")
    assert res.returncode == 0, res.stderr.decode()
    _, s_float = _read_scores(str(tmp_path / "s_float"))
    _, s_base = _read_scores(base)
    assert np.all(np.abs(s_float - s_base) <= 1e-3 * (1 + np.abs(s_base)))
    # smoothing as the oracle's, and it is what the scorer uses through the model pipe
    res = _run([os.path.join(BIN, "ivector-copy-plda"), "--smoothing=0.1", plda, str(tmp_path / "plda.s")])
    assert res.returncode == 0, res.stderr.decode()
    m2, t2, p2 = R.read_plda(str(tmp_path / "plda.s"))
    rt, rp = R.smooth(t, psi, 0.1)
    np.testing.assert_array_equal(m2, mean)
    np.testing.assert_allclose(t2, rt, rtol=1e-14)
    np.testing.assert_allclose(p2, rp, rtol=1e-14)
    res = _score_with(stage7, "ivector-copy-plda --smoothing=0.1 %s - |" % plda, tmp_path / "s_smooth")
    assert res.returncode == 0, res.stderr.decode()
    assert not np.array_equal(_read_scores(str(tmp_path / "s_smooth"))[1], s_base)
    # a truncated model: an error line and 255, not a crash
    whole = open(plda, "rb").read()
    (tmp_path / "cut").write_bytes(whole[: len(whole) * 2 // 3])
    res = _score_with(stage7, str(tmp_path / "cut"), tmp_path / "s_cut")
    assert res.returncode == 255 and b"ERROR (ivector-plda-scoring)" in res.stderr, res.stderr.decode()


# ------------------------------------------------------------------------------------------------ errors
def test_tool_errors(stage7, tmp_path):
    r = stage7[0]
    exp, data = r["exp"], r["data"]
    plda = os.path.join(exp, "xvectors_sre_combined", "plda_lda%d" % LDA_DIM)
    lda_in = "ark:%s/xvectors_sre_combined/xvector_sre_combined.ark" % exp
    vecs = "ark:transform-vec %s/xvectors_sre_combined/transform.mat %s ark:- |" % (exp, lda_in)
    (tmp_path / "three").write_text("tr000 tr000-u0 extra\n")
    res = _run([os.path.join(BIN, "ivector-plda-scoring"), plda, "ark:ivector-mean ark:%s/sre_combined/spk2utt %s ark:- | transform-vec "
                "%s/xvectors_sre_combined/transform.mat ark:- ark:- |" % (data, lda_in, exp), vecs, str(tmp_path / "three"),
                str(tmp_path / "out")], env=dict(os.environ, PATH=BIN + os.pathsep + os.environ["PATH"]))
    assert res.returncode == 255 and b"expected two fields: key1 key2" in res.stderr, res.stderr.decode()
    (tmp_path / "none").write_text("nobody tr000-u0\ntr000 nothing\n")
    res = _run([os.path.join(BIN, "ivector-plda-scoring"), plda, "ark:ivector-mean ark:%s/sre_combined/spk2utt %s ark:- | transform-vec "
                "%s/xvectors_sre_combined/transform.mat ark:- ark:- |" % (data, lda_in, exp), vecs, str(tmp_path / "none"),
                str(tmp_path / "out")], env=dict(os.environ, PATH=BIN + os.pathsep + os.environ["PATH"]))
    assert res.returncode == 1 and b"Processed 0 trials, 2 had errors." in res.stderr, res.stderr.decode()
    res = _run([os.path.join(BIN, "ivector-compute-lda"), "--dim=600", lda_in, "ark:%s/sre_combined/utt2spk" % data, str(tmp_path / "t")])
    assert res.returncode != 0 and re.search(rb"--dim=600 is out of range: the iVectors have dimension 512", res.stderr)
    assert not (tmp_path / "t").exists()
    res = _run([os.path.join(BIN, "compute-eer"), "-"], input=b"1.5 target\n0.5 target\n")
    assert res.returncode != 0 and b"No non-target scores seen." in res.stderr
