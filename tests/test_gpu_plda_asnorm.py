"""GPU tests of adaptive score normalisation end to end: xv_plda_cohort_stats (the fused path: a score matrix that exists one
chunk at a time) against xv_topn_stats of xv_plda_score_dense bit for bit, and the tool ivector-plda-scoring-asnorm on synthetic
tables against tests/asnorm_ref.py."""
import os
import re
import subprocess

import numpy as np
import pytest

import asnorm_ref as A
import helpers as H
import plda_ref as R
from oracle import kaldi_io as kio
from test_gpu_plda_dense import TILE_M, U53, dense_units

pytestmark = pytest.mark.gpu

BIN = os.path.join(H.ROOT, H.PKG_NAME, "bin")
LD = np.longdouble
N_TRAIN, N_TEST, N_COHORT = 20, 40, 30


# ------------------------------------------------------------------------------------------------ the fused path
@pytest.mark.parametrize("rows_per_chunk", [5, TILE_M])
def test_the_fused_statistics_are_those_of_the_dense_matrix_across_chunk_edges(rows_per_chunk, monkeypatch):
    P = H.pkg()
    dim, cols = 24, 70
    for rows in (rows_per_chunk - 1, rows_per_chunk, rows_per_chunk + 1, 2 * rows_per_chunk + 3):
        u, num_u, v, psi = R.scoring_case(rows, dim, rows, cols)
        monkeypatch.delenv("XVEC_PLDA_DENSE_WORKSPACE", raising=False)
        full = P.asnorm.plda_score_dense(u, num_u, v, psi)
        want = {n: P.asnorm.topn_stats(full, n) for n in (2, 9, cols)}
        want_t = {n: P.asnorm.topn_stats(np.ascontiguousarray(full.T), n) for n in (2, rows)} if rows >= 2 else {}
        assert P.asnorm.plda_dense_plan(rows, cols, dim)[1] == 1
        # a workspace of rows_per_chunk rows of the matrix: `rows` sits on the chunk edge
        monkeypatch.setenv("XVEC_PLDA_DENSE_WORKSPACE", str(8 * cols * rows_per_chunk))
        assert np.array_equal(P.asnorm.plda_score_dense(u, num_u, v, psi), full)          # the dense entry passes through chunks too
        for n, w in want.items():
            got = P.asnorm.plda_cohort_stats(u, num_u, v, psi, n)
            assert np.array_equal(got[0], w[0]) and np.array_equal(got[1], w[1]), (rows, n)
        # and of rows_per_chunk rows of its transpose (`cols` rows of `rows` scores): several chunks whatever `rows` is
        monkeypatch.setenv("XVEC_PLDA_DENSE_WORKSPACE", str(8 * rows * rows_per_chunk))
        for n, w in want_t.items():
            got = P.asnorm.plda_cohort_stats(u, num_u, v, psi, n, by_column=True)
            assert np.array_equal(got[0], w[0]) and np.array_equal(got[1], w[1]), (rows, n, "by column")
    chunks = P.asnorm.plda_dense_plan(2 * rows_per_chunk + 3, cols, dim, 8 * cols * rows_per_chunk)
    assert chunks[:2] == (rows_per_chunk, 3)


# ------------------------------------------------------------------------------------------------ the tool
def _run(args, cwd):
    r = subprocess.run(args, cwd=cwd, stdin=subprocess.DEVNULL, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    return r.returncode, r.stderr.decode()


def _fmt(x):
    """a score as the tools print it: BaseFloat through a stream of six significant digits"""
    return float("%g" % np.float32(x))


class Case:
    """Tables on which the model's transform is the identity and length normalisation is off: the vectors of
    plda_ref.scoring_case are what the kernels see."""

    def __init__(self, d, dim, seed):
        self.d, self.dim = str(d), dim
        u, _, v, self.psi = R.scoring_case(seed, dim, N_TRAIN, N_TEST + N_COHORT)
        self.train, self.test, self.cohort = u, v[:N_TEST], v[N_TEST:]
        self.num = np.array([(1, 2, 3)[k % 3] for k in range(N_TRAIN)], np.float64)
        self.tk = ["spk%02d" % k for k in range(N_TRAIN)]
        self.sk = ["utt%02d" % k for k in range(N_TEST)]
        self.ck = ["coh%02d" % k for k in range(N_COHORT)]
        R.write_plda(self.path("plda"), np.zeros(dim), np.eye(dim), self.psi)
        self.write("train", self.tk, self.train)
        self.write("test", self.sk, self.test)
        self.write("cohort", self.ck, self.cohort)
        with open(self.path("num_utts"), "w") as f:
            f.writelines("%s %d\n" % (k, n) for k, n in zip(self.tk, self.num))
        rng = np.random.default_rng(seed)
        # not every row is in a trial: train row 3 and test rows 5 and 6 are in none
        self.pairs = [(e, t) for e in range(N_TRAIN) for t in rng.choice(N_TEST, 4, replace=False) if e != 3 and t not in (5, 6)]
        self.write_trials("trials", self.pairs)

    def path(self, name):
        return os.path.join(self.d, name)

    def write(self, name, keys, rows):
        kio.write_ark_vectors(self.path(name + ".ark"), list(zip(keys, np.asarray(rows, np.float32))))

    def write_trials(self, name, pairs, extra=()):
        with open(self.path(name), "w") as f:
            f.writelines("%s %s\n" % (self.tk[e], self.sk[t]) for e, t in pairs)
            f.writelines(extra)

    def tool(self, out, *options, cohort="cohort", trials="trials", tool="ivector-plda-scoring-asnorm"):
        args = [os.path.join(BIN, tool), "--normalize-length=false", "--num-utts=ark:" + self.path("num_utts")] + list(options)
        args += [self.path("plda"), "ark:" + self.path("train.ark"), "ark:" + self.path("test.ark")]
        if tool.endswith("asnorm"):
            args.append("ark:" + self.path(cohort + ".ark"))
        return _run(args + [self.path(trials), self.path(out)], self.d)

    def scores(self, name):
        out = {}
        for line in open(self.path(name)):
            a, b, s = line.split()
            out[(self.tk.index(a), self.sk.index(b))] = (float(s), s)
        return out

    def stats(self, name):
        return [(k, float(m), float(s)) for k, m, s in (line.split() for line in open(self.path(name)))]

    def bound(self, P, cohort, top_n, pairs):
        """The reference's normalised scores from the RAW scores of xv_plda_score (the tool's own bits: no error of theirs to
        propagate) and a bound on the tool's distance from them.  Each cohort score of the device is within b = dense_units u
        size of the reference's (tests/test_gpu_plda_dense.py); the top-N mean and deviation as functions of a row move by at
        most the largest such b of the row (the sorted values move by no more, and the deviation of a vector by no more than its
        largest change), to which the sums' own bounds are added (tests/test_gpu_topn_stats.py):
          dmu <= b + (N + 1) u sum |x| / N,   dsigma <= b + (N / 2 + 4) u sigma + (N + 1) u sum |x| / N
        and z = (s - mu) / sigma moves by (dmu + |z| dsigma) / sigma plus three roundings; the result by half the sum of the two
        sides' and two more roundings."""
        raw = P.plda_score(self.train, self.num, self.test, self.psi, pairs)
        n = min(top_n, len(cohort))
        ref, (mu_e, sd_e), (mu_t, sd_t) = A.asnorm(raw, pairs, self.train, self.num, self.test, cohort, self.psi, top_n)
        s_e, s_t = A.cohort_scores(self.train, self.num, self.test, cohort, self.psi)
        b_e = (dense_units(self.dim) * U53 * A.expanded_size(self.train, self.num, cohort, self.psi)).max(1)
        b_t = (dense_units(self.dim) * U53 * A.expanded_size(cohort, np.ones(len(cohort)), self.test, self.psi)).max(0)
        bound = np.zeros(len(pairs), LD)
        for (mu, sd, b, s, col) in ((mu_e, sd_e, b_e, s_e, 0), (mu_t, sd_t, b_t, s_t, 1)):
            mag = A.topn_stats(s, n)[2]
            dmu = b + (n + 1) * U53 * mag / n
            dsd = b + (n / 2 + 4) * U53 * sd + (n + 1) * U53 * mag / n
            i = np.asarray(pairs)[:, col]
            with np.errstate(divide="ignore", invalid="ignore"):
                z = np.abs((raw.astype(LD) - mu[i]) / sd[i])
                bound += ((dmu[i] + z * dsd[i]) / sd[i] + 3 * U53 * z) / 2 + 2 * U53 * z / 2
        return raw, ref, bound, (mu_e, sd_e, mu_t, sd_t)


def _check_lines(case, got, pairs, ref, bound):
    """every line is the reference's after the same rounding: rounding is monotone, so the printed number lies between the
    printed ends of [ref - bound, ref + bound]"""
    assert sorted(got) == sorted(set(pairs))
    worst = 0
    for p, r, b in zip(pairs, ref, bound):
        lo, hi = _fmt(r - b), _fmt(r + b)
        assert lo <= got[p][0] <= hi, (p, got[p], float(r), float(b))
        worst = max(worst, float(b / max(abs(r), LD(1e-30))))
    return worst


@pytest.fixture(scope="module", params=[10, 150])
def case(request, tmp_path_factory):
    return Case(tmp_path_factory.mktemp("asnorm%d" % request.param), request.param, 40 + request.param)


def test_the_tool_matches_the_restatement_and_its_statistics_are_the_library_s(case):
    P = H.pkg()
    top_n = 7
    rc, err = case.tool("scores", "--top-n=%d" % top_n, "--train-stats=" + case.path("train_stats"), "--test-stats=" + case.path("test_stats"))
    assert rc == 0, err
    raw, ref, bound, _ = case.bound(P, case.cohort, top_n, case.pairs)
    worst = _check_lines(case, case.scores("scores"), case.pairs, ref, bound)
    print("ivector-plda-scoring-asnorm, dim %d: largest bound relative to its score %.3g" % (case.dim, worst))
    assert "Processed %d trials, 0 had errors." % len(case.pairs) in err and "Reading cohort iVectors" in err
    assert not re.search(r"top-n=\d+ is more than the cohort holds", err)
    # the statistics of the rows that are in a trial, in table order, as the C ABI gives them for those rows
    e_rows, t_rows = sorted({e for e, _ in case.pairs}), sorted({t for _, t in case.pairs})
    assert 3 not in e_rows and 5 not in t_rows and len(e_rows) == N_TRAIN - 1
    mu, sd = P.asnorm.plda_cohort_stats(case.train[e_rows], case.num[e_rows], case.cohort, case.psi, top_n)
    assert case.stats("train_stats") == [(case.tk[r], m, s) for r, m, s in zip(e_rows, mu, sd)]
    mu, sd = P.asnorm.plda_cohort_stats(case.cohort, np.ones(N_COHORT), case.test[t_rows], case.psi, top_n, by_column=True)
    assert case.stats("test_stats") == [(case.sk[r], m, s) for r, m, s in zip(t_rows, mu, sd)]
    # the sibling prints the raw scores this test fed the restatement with
    rc, err = case.tool("raw_scores", tool="ivector-plda-scoring")
    assert rc == 0, err
    got = case.scores("raw_scores")
    assert sorted(got) == sorted(case.pairs) and all(got[p][0] == _fmt(s) for p, s in zip(case.pairs, raw))


def test_a_top_n_above_the_cohort_size_is_plain_s_norm(case):
    P = H.pkg()
    rc, err = case.tool("scores_snorm", "--top-n=1000")
    assert rc == 0, err
    assert err.count("--top-n=1000 is more than the cohort holds: using all %d cohort scores (S-norm)." % N_COHORT) == 1
    raw, ref, bound, _ = case.bound(P, case.cohort, 1000, case.pairs)
    s_e, s_t = A.cohort_scores(case.train, case.num, case.test, case.cohort, case.psi)
    direct = A.snorm_direct(raw, case.pairs, s_e, s_t)
    assert np.all(np.abs(direct - ref) <= 1e-15 * (1 + np.abs(ref)))
    _check_lines(case, case.scores("scores_snorm"), case.pairs, direct, bound)
    rc, err = case.tool("scores_all", "--top-n=%d" % N_COHORT)
    assert rc == 0 and "is more than the cohort holds" not in err
    assert open(case.path("scores_all")).read() == open(case.path("scores_snorm")).read()


def test_a_trial_with_a_missing_key_is_skipped_and_counted(case):
    case.write_trials("trials_missing", case.pairs[:5], ["nobody utt00\n", "spk00 nothing\n"])
    rc, err = case.tool("scores_missing", "--top-n=7", trials="trials_missing")
    assert rc == 0 and "Processed 5 trials, 2 had errors." in err
    assert "Key nobody not present in training iVectors." in err and "Key nothing not present in test iVectors." in err
    raw, ref, bound, _ = case.bound(H.pkg(), case.cohort, 7, case.pairs[:5])
    _check_lines(case, case.scores("scores_missing"), case.pairs[:5], ref, bound)


def test_equal_top_scores_give_no_deviation_and_the_trial_is_skipped(case):
    """Three copies of train row 0's own vector in the cohort: with --top-n=3 the three highest cohort scores of every row that
    likes that vector best are one number."""
    P = H.pkg()
    cohort = np.concatenate([case.cohort, np.repeat(case.train[:1], 3, 0)])
    case.write("cohort_dup", case.ck + ["dup0", "dup1", "dup2"], cohort)
    rc, err = case.tool("scores_dup", "--top-n=3", cohort="cohort_dup")
    raw, ref, bound, (mu_e, sd_e, mu_t, sd_t) = case.bound(P, cohort, 3, case.pairs)
    dead = [(sd_e[e] == 0) or (sd_t[t] == 0) for e, t in case.pairs]
    assert sd_e[0] == 0 and any(dead) and not all(dead)
    assert rc == 0 and "Processed %d trials, %d had errors." % (len(dead) - sum(dead), sum(dead)) in err
    assert err.count("have standard deviation 0: not normalising trial") == sum(dead)
    keep = [i for i, d in enumerate(dead) if not d]
    _check_lines(case, case.scores("scores_dup"), [case.pairs[i] for i in keep], ref[keep], bound[keep])


def test_every_error_exits_255_and_writes_no_file(tmp_path):
    case = Case(tmp_path, 10, 3)
    bad = {"cohort_one": (case.ck[:1], case.cohort[:1]), "cohort_none": ([], case.cohort[:0]),
           "cohort_dim": (case.ck, np.concatenate([case.cohort, case.cohort[:, :1]], 1)),
           "cohort_inf": (case.ck, np.where(np.arange(case.dim) == 3, np.inf, case.cohort).astype(np.float32)),
           "cohort_nan": (case.ck, np.where(np.arange(case.dim) == 0, np.nan, case.cohort).astype(np.float32))}
    messages = {"cohort_one": "The cohort has 1 iVectors: score normalisation needs at least two.",
                "cohort_none": "The cohort has 0 iVectors: score normalisation needs at least two.",
                "cohort_dim": "iVector dimension 11 does not match the PLDA dimension 10",
                "cohort_inf": "has a value that is not finite", "cohort_nan": "has a value that is not finite"}
    for name, (keys, rows) in bad.items():
        case.write(name, keys, rows)
        rc, err = case.tool("never_" + name, "--top-n=3", "--train-stats=" + case.path("never_stats_" + name), cohort=name)
        assert rc == 255 and messages[name] in err, (name, rc, err)
    rc, err = case.tool("never_top_n", "--top-n=1")
    assert rc == 255 and "--top-n=1 is out of range" in err
    assert not [f for f in os.listdir(case.d) if f.startswith("never_")]
