"""GPU tests of ivector-adapt-plda (stage 2 of egs/sre/v2/run_sre16.sh:76-175): the statistics pass (one segment that
lists every row of xv_scatter_stats), the tool against tests/plda_adapt_ref.py on binary, text and piped models, its
errors, and the whole stage on a synthetic SRE16 recipe with the recipe's own argv.  Every subprocess has a time limit."""
import os
import subprocess
import time

import numpy as np
import pytest

import helpers as H
import plda_adapt_ref as A
import plda_ref as R
from oracle import backend as B
from oracle import kaldi_io as kio

pytestmark = pytest.mark.gpu
BIN = os.path.join(H.ROOT, H.PKG_NAME, "bin")


def _bash(cmd, timeout=600):
    env = dict(os.environ, PATH=BIN + os.pathsep + os.environ.get("PATH", ""))
    return subprocess.run(["bash", "-c", "set -o pipefail; " + cmd], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                          timeout=timeout, env=env)


def _close(a, b, rtol):
    assert np.abs(a - b).max() <= rtol * np.abs(b).max(), np.abs(a - b).max() / np.abs(b).max()


# ------------------------------------------------------------------------------------------------ the statistics pass
@pytest.mark.parametrize("dim", [7, 150, 512])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 3001])
def test_one_segment_of_every_row_is_the_sum_in_row_order(n, dim):
    P = H.pkg()
    rng = np.random.default_rng(n * 1000 + dim)
    x = (rng.standard_normal((n, dim)) * 3 + 1).astype(np.float32)
    s_tot, sums, _ = P.scatter_stats(x, [list(range(n))])
    seq = np.zeros(dim)
    for row in x.astype(np.float64):                      # one fp64 add per row, in list order
        seq = seq + row
    np.testing.assert_array_equal(sums[0], seq)
    x64 = x.astype(np.float64)
    assert np.abs(s_tot - x64.T @ x64).max() <= 1e-12 * np.abs(x64.T @ x64).max()


# ------------------------------------------------------------------------------------------------ the tool
def _model(rng, dim):
    mean = rng.standard_normal(dim) * 0.2
    t = np.linalg.qr(rng.standard_normal((dim, dim)))[0] * rng.uniform(0.5, 2.0, dim)[:, None]
    psi = np.sort(rng.uniform(0.05, 6.0, dim))[::-1]
    return mean, t, psi


def _adaptation_vectors(rng, mean, t, psi, n):
    dim = len(mean)
    tm = t / np.sqrt(1.0 + psi)[:, None]
    r = np.linalg.qr(rng.standard_normal((dim, dim)))[0]
    scale = np.sqrt(np.where(np.arange(dim) < dim // 5, 2.5, np.where(np.arange(dim) >= dim - dim // 5, 0.4, 1.0)))
    z = rng.standard_normal((n, dim)) * scale
    return (np.linalg.solve(tm, (z @ r.T).T).T + mean + 0.5 * np.linalg.solve(tm, r[:, 0])).astype(np.float32)


@pytest.fixture(scope="module")
def tool_case(tmp_path_factory):
    d = tmp_path_factory.mktemp("adapt")
    rng = np.random.default_rng(11)
    dim = 150
    mean, t, psi = _model(rng, dim)
    x = _adaptation_vectors(rng, mean, t, psi, 5000)
    R.write_plda(str(d / "plda"), mean, t, psi)
    kio.write_ark_vectors(str(d / "x.ark"), [("utt%05d" % i, v) for i, v in enumerate(x)], scp_path=str(d / "x.scp"))
    return d, mean, t, psi, x


def _check_model(path, ref):
    mean, t, psi = R.read_plda(path)
    np.testing.assert_allclose(mean, ref[0], rtol=1e-12, atol=1e-15)
    np.testing.assert_allclose(psi, ref[2], rtol=1e-9)
    for a, b in zip(A.implied_covariances(t, psi), A.implied_covariances(ref[1], ref[2])):
        _close(a, b, 1e-9)


def test_tool_matches_the_restatement(tool_case):
    d, mean, t, psi, x = tool_case
    n, m, v = A.stats(x)
    ref = A.adapt(n, m, v, mean, t, psi, 1.0, 0.75, 0.25)
    assert ref[3].max() > 1.0 and ref[3].min() < 1.0
    r = _bash("ivector-adapt-plda --within-covar-scale=0.75 --between-covar-scale=0.25 %s scp:%s %s"
              % (d / "plda", d / "x.scp", d / "adapted"))
    assert r.returncode == 0, r.stderr.decode()
    log = r.stderr.decode()
    assert "Accumulated stats from 5000 iVectors." in log
    assert "Mean differs from old mean with norm" in log
    assert "Eigenvalues of adaptation-data total-covariance in space where out-of-domain PLDA total-covariance is unit" in log
    assert "Old diagonal of between-class covar was:" in log and ", new diagonal is" in log
    assert (d / "adapted").read_bytes()[:2] == b"\0B"
    _check_model(str(d / "adapted"), ref)
    # a text model in, a text model out (--binary=false), and the model through ivector-copy-plda's pipe: the same model
    assert _bash("ivector-copy-plda --binary=false %s %s" % (d / "plda", d / "plda.txt")).returncode == 0
    r = _bash("ivector-adapt-plda --binary=false --within-covar-scale=0.75 --between-covar-scale=0.25 %s ark:%s %s"
              % (d / "plda.txt", d / "x.ark", d / "adapted.txt"))
    assert r.returncode == 0, r.stderr.decode()
    assert (d / "adapted.txt").read_bytes().startswith(b"<Plda>  [ ")
    _check_model(str(d / "adapted.txt"), ref)
    r = _bash("ivector-adapt-plda --within-covar-scale=0.75 --between-covar-scale=0.25 \"ivector-copy-plda --smoothing=0.0 %s - |\" "
              "\"ark:copy-vector scp:%s ark:- |\" %s" % (d / "plda", d / "x.scp", d / "adapted.pipe"))
    assert r.returncode == 0, r.stderr.decode()
    assert (d / "adapted.pipe").read_bytes() == (d / "adapted").read_bytes()
    r = _bash("ivector-copy-plda %s %s" % (d / "adapted.txt", d / "adapted.txt.bin"))
    assert r.returncode == 0 and (d / "adapted.txt.bin").read_bytes() == (d / "adapted").read_bytes()
    # Kaldi's defaults (0.3 / 0.7) and the mean-diff scale are what the tool uses
    r = _bash("ivector-adapt-plda --mean-diff-scale=0.0 %s scp:%s %s" % (d / "plda", d / "x.scp", d / "adapted.default"))
    assert r.returncode == 0, r.stderr.decode()
    _check_model(str(d / "adapted.default"), A.adapt(n, m, v, mean, t, psi, 0.0, 0.3, 0.7))


def test_tool_errors(tool_case, tmp_path):
    d, mean, t, psi, x = tool_case
    out = tmp_path / "out"
    (tmp_path / "empty.ark").write_bytes(b"")
    r = _bash("ivector-adapt-plda %s ark:%s %s" % (d / "plda", tmp_path / "empty.ark", out))
    assert r.returncode == 255 and b"Accumulated stats from 0 iVectors." in r.stderr, r.stderr.decode()
    assert not out.exists()
    kio.write_ark_vectors(str(tmp_path / "short.ark"), [("u%d" % i, v[:100]) for i, v in enumerate(x[:50])])
    r = _bash("ivector-adapt-plda %s ark:%s %s" % (d / "plda", tmp_path / "short.ark", out))
    assert r.returncode == 255 and b"iVector dimension 100 does not match the PLDA dimension 150" in r.stderr, r.stderr.decode()
    assert not out.exists()
    r = _bash("ivector-adapt-plda --within-covar-scale=0.75 --between-covar=0.25 %s scp:%s %s" % (d / "plda", d / "x.scp", out))
    assert r.returncode == 255 and b"Invalid option --between-covar=0.25" in r.stderr, r.stderr.decode()
    assert not out.exists()


# ------------------------------------------------------------------------------------------------ a synthetic SRE16 recipe
D_IN, LDA_DIM = 512, 150
LANGS = ("tgl", "yue")


def _domain_models(rng):
    """The out-of-domain speaker model, and the in-domain one: the same speaker subspace, a shifted mean, more within-class
    variance in 30 directions and less in 60 others."""
    a = np.linalg.qr(rng.standard_normal((D_IN, D_IN)))[0]
    lb = a[:, :200] * np.sqrt(np.geomspace(1.2, 0.05, 200))[None, :]
    c = np.linalg.qr(rng.standard_normal((D_IN, D_IN)))[0]
    lw = c * np.linspace(0.6, 1.4, D_IN)[None, :]
    mu = rng.standard_normal(D_IN) * 0.5
    g = np.ones(D_IN)
    g[:30] = 2.2
    g[-60:] = 0.45
    return (lb, lw, mu), (lb, lw * g[None, :], mu + rng.standard_normal(D_IN) * 0.35)


def _speaker(rng, model, n):
    lb, lw, mu = model
    y = mu + lb @ rng.standard_normal(lb.shape[1])
    return [(y + lw @ rng.standard_normal(D_IN)).astype(np.float32) for _ in range(n)]


@pytest.fixture(scope="module")
def recipe(tmp_path_factory):
    root = tmp_path_factory.mktemp("sre16")
    exp, data = root / "exp", root / "data"
    rng = np.random.default_rng(2016)
    ood, ind = _domain_models(rng)
    train, train_spk2utt = [], []
    for s in range(300):
        utts = ["tr%03d-u%d" % (s, i) for i in range(int(rng.integers(2, 11)))]
        train.extend(zip(utts, _speaker(rng, ood, len(utts))))
        train_spk2utt.append(("tr%03d" % s, utts))
    major = []
    for s in range(500):                                                   # unlabelled in-domain data
        major.extend(("maj%04d-%d" % (s, i), v) for i, v in enumerate(_speaker(rng, ind, int(rng.integers(1, 6)))))
    enroll, enroll_spk2utt, test, lang = [], [], [], {}
    for s in range(40):
        k = int(rng.integers(1, 4))
        vecs = _speaker(rng, ind, k + 2)
        spk = "en%02d" % s
        lang[spk] = LANGS[s % 2]
        utts = ["%s-u%d" % (spk, i) for i in range(k)]
        enroll.extend(zip(utts, vecs[:k]))
        enroll_spk2utt.append((spk, utts))
        test.extend(("te%02d-%d" % (s, i), v) for i, v in enumerate(vecs[k:]))
    for s in range(80):
        test.append(("imp%02d" % s, _speaker(rng, ind, 1)[0]))
    test_keys = [k for k, _ in test]
    trials = []
    for s in range(40):
        for key in sorted(set(["te%02d-0" % s, "te%02d-1" % s] + list(rng.choice(test_keys, 25, replace=False)))):
            trials.append(("en%02d" % s, key, "target" if key.startswith("te%02d-" % s) else "nontarget"))
    trials = [trials[i] for i in rng.permutation(len(trials))]

    d_comb, d_major, d_enr, d_test = (exp / "xvectors_sre_combined", exp / "xvectors_sre16_major",
                                      exp / "xvectors_sre16_eval_enroll", exp / "xvectors_sre16_eval_test")
    for d in (d_comb, d_major, d_enr, d_test, exp / "xvector_scores", data / "sre_combined", data / "sre16_eval_enroll",
              data / "sre16_eval_test"):
        d.mkdir(parents=True, exist_ok=True)
    kio.write_ark_vectors(str(d_comb / "xvector.ark"), train, scp_path=str(d_comb / "xvector_sre_combined.scp"))
    kio.write_ark_vectors(str(d_major / "xvector.ark"), major, scp_path=str(d_major / "xvector_sre16_major.scp"))
    kio.write_ark_vectors(str(d_enr / "xvector.ark"), enroll, scp_path=str(d_enr / "xvector_sre16_eval_enroll.scp"))
    kio.write_ark_vectors(str(d_test / "xvector.ark"), test, scp_path=str(d_test / "xvector_sre16_eval_test.scp"))
    (data / "sre_combined" / "spk2utt").write_text("".join("%s %s\n" % (s, " ".join(u)) for s, u in train_spk2utt))
    (data / "sre_combined" / "utt2spk").write_text("".join("%s %s\n" % (u, s) for s, us in train_spk2utt for u in us))
    (data / "sre16_eval_enroll" / "spk2utt").write_text("".join("%s %s\n" % (s, " ".join(u)) for s, u in enroll_spk2utt))
    (d_enr / "num_utts.ark").write_text("".join("%s %d \n" % (s, len(u)) for s, u in enroll_spk2utt))
    lines = ["%s %s %s\n" % t for t in trials]
    (data / "sre16_eval_test" / "trials").write_text("".join(lines))
    for lg in LANGS:
        (data / "sre16_eval_test" / ("trials_" + lg)).write_text("".join(ln for ln in lines if lang[ln.split()[0]] == lg))
    return dict(root=root, exp=str(exp), data=str(data), train=train, train_spk2utt=train_spk2utt, major=major,
                enroll=enroll, enroll_spk2utt=enroll_spk2utt, test=test, trials=trials, lang=lang)


def _stage2_commands():
    """egs/sre/v2/run_sre16.sh:78-161 without the `$train_cmd <log>` prefix and the MATLAB blocks, with $exp / $data /
    $lda_dim / $sre16_trials substituted; `utils/filter_scp.pl` is restated in the test."""
    scoring = ("ivector-plda-scoring --normalize-length=true \\\n"
               "    --num-utts=ark:%(exp)s/xvectors_sre16_eval_enroll/num_utts.ark \\\n"
               "    \"ivector-copy-plda --smoothing=0.0 %(exp)s/%(plda)s - |\" \\\n"
               "    \"ark:ivector-mean ark:%(data)s/sre16_eval_enroll/spk2utt scp:%(exp)s/xvectors_sre16_eval_enroll/"
               "xvector_sre16_eval_enroll.scp ark:- | ivector-subtract-global-mean %(exp)s/xvectors_sre16_major/mean.vec ark:- ark:- | "
               "transform-vec %(exp)s/xvectors_sre_combined/transform.mat ark:- ark:- | ivector-normalize-length ark:- ark:- |\" \\\n"
               "    \"ark:ivector-subtract-global-mean %(exp)s/xvectors_sre16_major/mean.vec scp:%(exp)s/xvectors_sre16_eval_test/"
               "xvector_sre16_eval_test.scp ark:- | transform-vec %(exp)s/xvectors_sre_combined/transform.mat ark:- ark:- | "
               "ivector-normalize-length ark:- ark:- |\" \\\n"
               "    \"cat '%(sre16_trials)s' | cut -d\\  --fields=1,2 |\" %(exp)s/xvector_scores/%(scores)s")
    return [
        "ivector-mean scp:%(exp)s/xvectors_sre16_major/xvector_sre16_major.scp \\\n"
        "    %(exp)s/xvectors_sre16_major/mean.vec",
        "ivector-compute-lda --total-covariance-factor=0.0 --dim=%(lda_dim)d \\\n"
        "    \"ark:ivector-subtract-global-mean scp:%(exp)s/xvectors_sre_combined/xvector_sre_combined.scp ark:- |\" \\\n"
        "    ark:%(data)s/sre_combined/utt2spk %(exp)s/xvectors_sre_combined/transform.mat",
        "ivector-compute-plda ark:%(data)s/sre_combined/spk2utt \\\n"
        "    \"ark:ivector-subtract-global-mean scp:%(exp)s/xvectors_sre_combined/xvector_sre_combined.scp ark:- | transform-vec "
        "%(exp)s/xvectors_sre_combined/transform.mat ark:- ark:- | ivector-normalize-length ark:-  ark:- |\" \\\n"
        "    %(exp)s/xvectors_sre_combined/plda_lda%(lda_dim)d",
        "ivector-adapt-plda --within-covar-scale=0.75 --between-covar-scale=0.25 \\\n"
        "    %(exp)s/xvectors_sre_combined/plda_lda%(lda_dim)d \\\n"
        "    \"ark:ivector-subtract-global-mean scp:%(exp)s/xvectors_sre16_major/xvector_sre16_major.scp ark:- | transform-vec "
        "%(exp)s/xvectors_sre_combined/transform.mat ark:- ark:- | ivector-normalize-length ark:- ark:- |\" \\\n"
        "    %(exp)s/xvectors_sre16_major/plda_lda%(lda_dim)d_sre16_adapt",
        scoring.replace("%(plda)s", "xvectors_sre_combined/plda_lda%(lda_dim)d").replace("%(scores)s", "sre16_eval_scores"),
        scoring.replace("%(plda)s", "xvectors_sre16_major/plda_lda%(lda_dim)d_sre16_adapt")
               .replace("%(scores)s", "sre16_eval_scores_adapt"),
    ], "paste %(trials)s %(scores)s | awk '{print $6, $3}' | compute-eer - 2>/dev/null"


@pytest.fixture(scope="module")
def stage2(recipe):
    subst = dict(exp=recipe["exp"], data=recipe["data"], lda_dim=LDA_DIM,
                 sre16_trials=os.path.join(recipe["data"], "sre16_eval_test", "trials"))
    cmds, eer_cmd = _stage2_commands()
    logs, secs = [], []
    for c in cmds:
        t0 = time.perf_counter()
        r = _bash(c % subst)
        secs.append(time.perf_counter() - t0)
        logs.append(r.stderr.decode())
        assert r.returncode == 0, logs[-1]
    print("stage 2 wall times (s): " + ", ".join("%s %.2f" % (c.split()[0], s) for c, s in zip(cmds, secs)))
    return recipe, logs, eer_cmd


def _oracle_stage2(r):
    """The same stage in numpy: (out-of-domain scores, adapted scores, the adaptation eigenvalues)."""
    x = np.stack([v for _, v in r["train"]])
    row = {k: i for i, (k, _) in enumerate(r["train"])}
    spk = np.empty(len(x), np.int64)
    for s, (_, utts) in enumerate(r["train_spk2utt"]):
        spk[[row[u] for u in utts]] = s
    lda = R.lda(B.subtract_global_mean(x), spk, LDA_DIM)
    y, _ = B.backend_chain(x, B.global_mean(x), lda, normalize=True)
    segs = [[row[u] for u in utts] for _, utts in r["train_spk2utt"]]
    pmean, pt, psi = R.plda(y.astype(np.float32), segs)
    xm = np.stack([v for _, v in r["major"]])
    ym, _ = B.backend_chain(xm, B.global_mean(xm), lda, normalize=True)
    n, m, v = A.stats(ym.astype(np.float32))
    amean, at, apsi, s = A.adapt(n, m, v, pmean, pt, psi, 1.0, 0.75, 0.25)
    major_mean = B.global_mean(xm)
    means, counts, _, _ = B.speaker_means(r["enroll_spk2utt"], dict(r["enroll"]))
    e, _ = B.backend_chain(np.stack([mv for _, mv in means]), major_mean, lda, normalize=True)
    t, _ = B.backend_chain(np.stack([tv for _, tv in r["test"]]), major_mean, lda, normalize=True)
    cnt = np.array([counts[k] for k, _ in means], np.float64)
    ei = {k: i for i, (k, _) in enumerate(means)}
    ti = {k: i for i, (k, _) in enumerate(r["test"])}
    out = []
    for mean_, t_, psi_ in ((pmean, pt, psi), (amean, at, apsi)):
        u, _ = R.transform_ivector(e.astype(np.float32), mean_, t_, psi_, cnt)
        w, _ = R.transform_ivector(t.astype(np.float32), mean_, t_, psi_)
        out.append(np.array([R.llr(u[ei[a]], cnt[ei[a]], w[ti[b]], psi_) for a, b, _ in r["trials"]]))
    return out[0], out[1], s


def _read_scores(path):
    rows = [line.split() for line in open(path)]
    assert all(len(r) == 3 for r in rows)
    return [(a, b) for a, b, _ in rows], np.array([float(s) for _, _, s in rows])


def test_stage2_of_run_sre16_runs_with_the_recipes_argv(stage2):
    r, logs, _ = stage2
    adapt_log = logs[3]
    assert "Accumulated stats from %d iVectors." % len(r["major"]) in adapt_log
    assert "Mean differs from old mean with norm" in adapt_log
    assert "Eigenvalues of adaptation-data total-covariance" in adapt_log
    assert "Old diagonal of between-class covar was:" in adapt_log
    for score_log in logs[4:]:
        assert "Read 40 training iVectors, errors on 0" in score_log
        assert "Processed %d trials, 0 had errors." % len(r["trials"]) in score_log
    ref_ood, ref_adapt, s = _oracle_stage2(r)
    assert s.max() > 1.0 and s.min() < 1.0                                 # some directions grow, some shrink
    scores_dir = os.path.join(r["exp"], "xvector_scores")
    for name, ref in (("sre16_eval_scores", ref_ood), ("sre16_eval_scores_adapt", ref_adapt)):
        keys, scores = _read_scores(os.path.join(scores_dir, name))
        assert keys == [(a, b) for a, b, _ in r["trials"]]
        assert np.all(np.abs(scores - ref) <= 1e-4 * (1 + np.abs(ref))), (name, np.abs(scores - ref).max())
    # the adapted model is a different model, and the one the restatement predicts
    _, _, psi = R.read_plda(os.path.join(r["exp"], "xvectors_sre16_major", "plda_lda%d_sre16_adapt" % LDA_DIM))
    _, _, psi0 = R.read_plda(os.path.join(r["exp"], "xvectors_sre_combined", "plda_lda%d" % LDA_DIM))
    assert not np.allclose(psi, psi0)
    assert np.all(np.diff(psi) <= 0) and psi.min() >= 0


def test_eers_of_stage2_pooled_and_per_language(stage2):
    """run_sre16.sh:112-116 and :157-161: filter_scp.pl splits the scores by the enrolment speakers of each language's
    trial list (restated here), then paste | awk | compute-eer, for both models."""
    r, _, eer_cmd = stage2
    tdir = os.path.join(r["data"], "sre16_eval_test")
    sdir = os.path.join(r["exp"], "xvector_scores")
    for scores in ("sre16_eval_scores", "sre16_eval_scores_adapt"):
        lines = open(os.path.join(sdir, scores)).readlines()
        pairs = [("trials", scores)]
        for lg in LANGS:
            keep = A.filter_scp(open(os.path.join(tdir, "trials_" + lg)).readlines(), lines)
            name = scores.replace("sre16_eval_", "sre16_eval_%s_" % lg)
            with open(os.path.join(sdir, name), "w") as f:
                f.write("".join(keep))
            pairs.append(("trials_" + lg, name))
        for trials, sc in pairs:
            res = _bash(eer_cmd % dict(trials=os.path.join(tdir, trials), scores=os.path.join(sdir, sc)))
            assert res.returncode == 0, res.stderr.decode()
            tl = [ln.split() for ln in open(os.path.join(tdir, trials))]
            _, s = _read_scores(os.path.join(sdir, sc))
            assert len(tl) == len(s)
            tgt = [v for v, t in zip(s, tl) if t[2] == "target"]
            non = [v for v, t in zip(s, tl) if t[2] == "nontarget"]
            e, _ = R.eer(tgt, non)
            assert res.stdout.decode() == "%.4g\n" % (100.0 * e)
            assert 0.0 <= e < 0.5
