"""GPU tests of i-vector extraction (csrc/ivex_kernels.hip): the derived variables, the statistics and the two fp64 MFMA GEMMs
against the float64 restatement (tests/ivector_ref.py) for equality on integer models, the solve and the objective change within
bounds computed from the restatement's own Q, a Q that is not positive definite, batch independence, the options, and
sid/extract_ivectors.sh:65-70 through real pipes."""
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import helpers as H
import ivector_cases as C
import ivector_ref as R
import ubm_ref as UR
from oracle import kaldi_io as kio

pytestmark = pytest.mark.gpu
P = H.pkg()
BIN = os.path.join(H.ROOT, H.PKG_NAME, "bin")

RT, NB, MAX_S, MAX_B = C.RT, C.NB, C.MAX_S, C.MAX_B   # read from csrc/ivex_kernels.h (tests/ivector_cases.py)
U53 = C.U53
CASES = C.CASES
eps_of = C.eps_of


@functools.lru_cache(maxsize=None)
def integer_case(G, D, S):
    m = R.integer_model(C.integer_seed(G, D, S), G, D, S)
    return m, R.derived(m["M"], m["sigma_inv"])


_utterances = C.integer_utterances


def _reference(m, sim_U, utts, **kw):
    return [R.extract(x, post, m["M"], m["sigma_inv"], m["prior_offset"], sim_U=sim_U, **kw) for x, post in utts]


def check_solve(ref, iv, auxf, l_gpu, Q_gpu, p):
    """the i-vector, the residual and the objective change of one utterance; ref is the restatement's"""
    Q, l, x_ref = ref["quadratic"], ref["linear"], ref["x"]
    S = len(l)
    eps = eps_of(Q)
    assert eps < 1e-6, "a precondition of the test's inputs"
    want = x_ref.copy()
    want[0] -= p
    norm_x = np.linalg.norm(x_ref)
    err = np.abs(iv.astype(np.float64) - want.astype(np.float32).astype(np.float64))
    bound = eps * norm_x + np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
    print("S = %d: eps %.3g, worst |x - ref| / bound %.3g" % (S, eps, float((err / bound).max())))
    assert np.all(err <= bound)
    # the residual against the terms the device itself formed, in extended precision.  The first term is the backward error of
    # the solve, on the solution x; the second is the float32 rounding of the output, and what is rounded is x - p e_0 (the
    # offset leaves element 0 before the rounding), so that is the vector whose norm it carries.
    xq = iv.astype(np.longdouble)
    xq[0] += np.longdouble(p)
    res = np.linalg.norm((Q_gpu.astype(np.longdouble) @ xq - l_gpu.astype(np.longdouble)).astype(np.float64))
    nq, nx = np.linalg.norm(Q_gpu, 2), float(np.linalg.norm(xq.astype(np.float64)))
    res_bound = 4 * S * (3 * S + 1) * U53 * nq * nx + nq * 2.0 ** -24 * float(np.linalg.norm(iv.astype(np.float64)))
    print("residual %.3g, bound %.3g" % (res, res_bound))
    assert res <= res_bound
    # the objective change: both evaluation points, any order of the S^2 + 2 S terms, plus what the solution's error moves F by
    e0 = np.zeros(S)
    e0[0] = p
    terms = sum(np.abs(l * v).sum() + 0.5 * np.abs(v[:, None] * Q * v[None, :]).sum() for v in (x_ref, e0))
    d_bound = (S * S + 2 * S) * U53 * terms + np.linalg.norm(Q, 2) * (eps * norm_x) ** 2
    xl = x_ref.astype(np.longdouble)
    F = lambda v: float(l.astype(np.longdouble) @ v - 0.5 * (v @ Q.astype(np.longdouble) @ v))
    d_ref = F(xl) - F(e0.astype(np.longdouble))
    print("auxf change %.17g, reference %.17g, bound %.3g" % (auxf, d_ref, d_bound))
    assert abs(auxf - d_ref) <= d_bound
    assert auxf >= -d_bound


# ------------------------------------------------------------------------------------------------------------------- exact
@pytest.mark.parametrize("G,D,S,T,B", CASES)
def test_integer_models_give_the_restatements_terms_bit_for_bit(G, D, S, T, B):
    m, (sim, U) = integer_case(G, D, S)
    ie = P.IvectorExtractor(**m)
    got_sim, got_U = ie.derived()
    assert np.array_equal(got_sim, sim) and np.array_equal(got_U, U)
    utts = _utterances(G + D + S, B, T, G, D, empty_every=7)
    ref = _reference(m, (sim, U), utts)
    # every absolute partial sum of l and Q stays below 2^53: float64 holds every one exactly, whatever the order
    for (x, post), r in zip(utts, ref):
        abs_X = R.stats(np.abs(x), post, G)[1].reshape(-1)
        assert (np.abs(sim).T @ abs_X).max() + abs(m["prior_offset"]) < 2.0 ** 53
        assert (r["gamma"] @ np.abs(U)).max() + 1.0 < 2.0 ** 53
    iv, status, auxf, det = ie.extract([x for x, _ in utts], [p for _, p in utts], return_details=True)
    assert not status.any()
    for u, r in enumerate(ref):
        for name in ("gamma", "X", "linear", "quadratic"):
            assert np.array_equal(det[name][u], r[name]), (u, name)
        check_solve(r, iv[u], auxf[u], det["linear"][u], det["quadratic"][u], m["prior_offset"])
    if G > 1 and T < G:
        assert any((r["gamma"] == 0).any() for r in ref), "no Gaussian went without a frame"


def _assert_terms(det, ref):
    for u, r in enumerate(ref):
        for name in ("gamma", "X", "linear", "quadratic"):
            assert np.array_equal(det[name][u], r[name]), (u, name)


@pytest.mark.parametrize("G,D,S,T,B", C.LARGE_S_TERM_CASES)
def test_integer_models_give_the_restatements_terms_bit_for_bit_at_large_s(G, D, S, T, B):
    """The quadratic GEMM at N = P columns and the packed-index recovery of ivex_derive up to e = P - 1, P = S (S + 1) / 2, at
    S = kIvexThreads + 1 and kIvexMaxS.  The terms only: an integer model's Q is too ill-conditioned at this size for check_solve's
    precondition, and test_random_models_solve_within_the_bound covers the solve at these S."""
    m, (sim, U) = integer_case(G, D, S)
    ie = P.IvectorExtractor(**m)
    got_sim, got_U = ie.derived()
    assert np.array_equal(got_sim, sim) and np.array_equal(got_U, U)
    utts = C.case_utterances(G, D, S, T, B)
    ref = _reference(m, (sim, U), utts)
    for (x, post), r in zip(utts, ref):
        assert C.exact_preconditions(m, sim, U, x, post, r["gamma"])
    iv, status, auxf, det = ie.extract([x for x, _ in utts], [p for _, p in utts], return_details=True)
    assert not status.any() and np.isfinite(iv).all() and np.isfinite(auxf).all()
    _assert_terms(det, ref)


def test_a_launch_group_closed_by_its_frames_gives_the_restatements_terms_bit_for_bit():
    """IvexExtract closes a launch group at kIvexMaxBatch utterances or at kBatchFrames frames.  Three utterances of about 30000
    frames: the third would take the first group past kBatchFrames, so the call makes the groups {0, 1}, {2} and {3}, the last one an
    utterance that is past the limit on its own; the frame and pair offsets of the later groups start beyond 2^16."""
    G, D, S = C.FRAMES_SHAPE
    m, (sim, U) = integer_case(G, D, S)
    ie = P.IvectorExtractor(**m)
    utts = C.frames_utterances()
    ref = _reference(m, (sim, U), utts)
    for (x, post), r in zip(utts, ref):
        assert C.exact_preconditions(m, sim, U, x, post, r["gamma"])
    iv, status, auxf, det = ie.extract([x for x, _ in utts], [p for _, p in utts], return_details=True)
    assert not status.any()
    _assert_terms(det, ref)


# ------------------------------------------------------------------------------------------------------------------- the solve
@pytest.mark.parametrize("G,D,S", C.SOLVE_CASES)
def test_random_models_solve_within_the_bound(G, D, S):
    """Sigma^-1 = A A' / D + I; (1, 2, 17) is the rank-poor case: Q is the identity plus a term of rank 2.  The S above
    2 kIvexPanel + 3 are the edges of ivex_solve_kernel's loops, each from below and from above, the recipes' 400 and 600 and the
    limit kIvexMaxS (tests/ivector_cases.py's SOLVE_EDGES says which loop each one is for)."""
    m = C.solve_model(G, D, S)
    ie = P.IvectorExtractor(**m)
    sim_U = R.derived(m["M"], m["sigma_inv"])
    utts = C.solve_utterances(G, D, S, C.solve_utts_count(S))
    ref = _reference(m, sim_U, utts)
    iv, status, auxf, det = ie.extract([x for x, _ in utts], [p for _, p in utts], return_details=True)
    assert not status.any()
    for u, r in enumerate(ref):
        if G == 1:
            assert np.linalg.matrix_rank(r["quadratic"] - np.eye(S)) == 2
        check_solve(r, iv[u], auxf[u], det["linear"][u], det["quadratic"][u], m["prior_offset"])


def _not_positive_definite(S, s0):
    G, D = 2, 3
    m = C.not_pd_model(G, D, S, s0)
    ie = P.IvectorExtractor(**m)
    sim_U = R.derived(m["M"], m["sigma_inv"])
    utts = C.not_pd_utterances(D)
    bad = utts[1]
    bad_Q = R.extract(*bad, m["M"], m["sigma_inv"], m["prior_offset"], sim_U=sim_U)["quadratic"]
    assert np.linalg.eigvalsh(bad_Q).min() < 0
    assert np.array_equal(bad_Q[:s0, :s0], np.eye(s0)) and s0 <= C.first_bad_pivot(bad_Q) < S
    iv, status, auxf, det = ie.extract([x for x, _ in utts], [p for _, p in utts], return_details=True)
    assert status.tolist() == [0, 1, 0]
    assert np.isfinite(iv).all() and np.isfinite(auxf).all() and not iv[1].any() and auxf[1] == 0.0
    for u in (0, 2):
        r = R.extract(*utts[u], m["M"], m["sigma_inv"], m["prior_offset"], sim_U=sim_U)
        check_solve(r, iv[u], auxf[u], det["linear"][u], det["quadratic"][u], m["prior_offset"])


def test_a_q_that_is_not_positive_definite_is_flagged_and_its_neighbours_are_right():
    """Sigma^-1 of Gaussian 0 has a negative diagonal, on purpose: an utterance that lands on it gets Q = I - 8 gamma M'M, which
    has a negative pivot.  An arithmetic flag for that utterance, not a fault; the others of the batch are untouched."""
    _not_positive_definite(NB + 5, 0)


def test_a_bad_pivot_in_a_late_panel_is_flagged_too():
    """With s0 = 2 kIvexPanel + 1 leading columns of every M_g zero the leading s0 x s0 block of Q is the identity: the bad pivot
    comes in the third panel of the factorisation or later, after block-column updates that have earlier panels to subtract."""
    _not_positive_definite(C.LATE_S, C.LATE_S0)


# ------------------------------------------------------------------------------------------------------------------- batches
def test_an_utterance_has_the_same_bits_alone_and_anywhere_in_a_batch():
    G, D, S = 37, 23, 40
    m = R.random_model(11, G, D, S)
    ie = P.IvectorExtractor(**m)
    rng = np.random.default_rng(2)

    def utt(T):
        x = rng.normal(0.0, 2.0, (T, D)).astype(np.float32)
        return x, [(rng.permutation(G)[:4].astype(np.int32), rng.dirichlet(np.ones(4)).astype(np.float32)) for _ in range(T)]

    mine = utt(100)
    others = [utt(int(T)) for T in rng.integers(1, 250, RT)]   # longer and shorter ones
    iv0, st0, ax0, det0 = ie.extract([mine[0]], [mine[1]], return_details=True)
    assert st0[0] == 0
    more = [utt(int(T)) for T in rng.integers(1, 250, MAX_B - RT)]
    # first, middle and last of RT + 1; the last of the first launch group and the only one of the second, of kIvexMaxBatch + 1
    for k, rest in [(0, others), (RT // 2, others), (RT, others), (MAX_B - 1, others + more), (MAX_B, others + more)]:
        batch = rest[:k] + [mine] + rest[k:]
        assert len(batch) == (RT + 1 if k <= RT else MAX_B + 1)
        iv, st, ax, det = ie.extract([x for x, _ in batch], [p for _, p in batch], return_details=True)
        assert np.array_equal(iv[k].view(np.uint32), iv0[0].view(np.uint32)), k
        assert np.array_equal(ax[k:k + 1].view(np.uint64), ax0.view(np.uint64)), k
        for name in ("gamma", "X", "linear", "quadratic"):
            assert np.array_equal(det[name][k].view(np.uint64), det0[name][0].view(np.uint64)), (k, name)


# ------------------------------------------------------------------------------------------------------------------- options
def test_acoustic_weight_and_max_count_follow_the_restatement():
    G, D, S = 5, 60, 17
    m, sim_U = integer_case(G, D, S)
    ie = P.IvectorExtractor(**m)
    utts = [R.integer_utterance(1, 64, G, D, empty_every=5), R.integer_utterance(2, 9, G, D)]
    feats, posts = [x for x, _ in utts], [p for _, p in utts]
    # 0.5 is a power of two: the statistics stay exact
    ref = _reference(m, sim_U, utts, acoustic_weight=0.5)
    iv, status, auxf, det = ie.extract(feats, posts, return_details=True, acoustic_weight=0.5)
    for u, r in enumerate(ref):
        for name in ("gamma", "X", "linear", "quadratic"):
            assert np.array_equal(det[name][u], r[name]), (u, name)
        check_solve(r, iv[u], auxf[u], det["linear"][u], det["quadratic"][u], m["prior_offset"])
    # a max_count between the two utterances' totals bites on the first one only
    tots = [sum(float(w.sum()) for _, w in p) for p in posts]
    max_count = 0.5 * (tots[0] + tots[1])
    assert tots[1] < max_count < tots[0]
    assert [R.scale_posteriors(p, 1.0, max_count)[2] for p in posts] == [True, False]
    ref = _reference(m, sim_U, utts, max_count=max_count)
    iv, status, auxf, det = ie.extract(feats, posts, return_details=True, max_count=max_count)
    for u, r in enumerate(ref):
        # float32 products of float32 posteriors and a float32 scale, then sums of under 2^9 values of 24 + 3 bits within 2^4 of
        # one another: float64 holds gamma and X exactly in any order
        assert np.array_equal(det["gamma"][u], r["gamma"]) and np.array_equal(det["X"][u], r["X"]), u
        check_solve(r, iv[u], auxf[u], det["linear"][u], det["quadratic"][u], m["prior_offset"])
    assert abs(det["gamma"][0].sum() - max_count) < 1e-5 * max_count


def test_a_gaussian_index_outside_the_model_is_an_error_before_any_launch():
    m, _ = integer_case(4, 1, 1)
    ie = P.IvectorExtractor(**m)
    x = np.zeros((2, 1), np.float32)
    for bad in (4, -1):
        with pytest.raises(P.XvError, match="name Gaussian"):
            ie.extract([x], [[(np.array([0], np.int32), np.array([1.0], np.float32)), (np.array([bad], np.int32), np.array([1.0], np.float32))]])
    with pytest.raises(P.XvError, match="limit of 1024"):
        P.IvectorExtractor(np.ones(1), np.zeros((1, 1, 1025)), np.ones((1, 1)), 1.0)


# ------------------------------------------------------------------------------------------------------------------- the recipe
def _sh(line, cwd=None):
    env = dict(os.environ, PATH=BIN + os.pathsep + os.environ.get("PATH", ""))
    return subprocess.run(["/bin/sh", "-c", line], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, cwd=cwd, timeout=300)


def _read_text_vectors(data):
    out = []
    for line in data.decode().splitlines():
        key, rest = line.split(None, 1)
        assert rest.strip().startswith("[") and rest.strip().endswith("]"), line
        out.append((key, np.array(rest.strip()[1:-1].split(), dtype=np.float32)))
    return out


def test_extract_ivectors_lines_run_with_the_recipes_argv(tmp_path):
    srcdir, sdata, out = tmp_path / "extractor", tmp_path / "split1" / "1", tmp_path / "ivectors"
    for d in (srcdir, sdata, out):
        d.mkdir(parents=True)
    G, D, S = 21, 60, 17
    w, means, b, ic = UR.random_full_model(31, G, D, spread=1.0)
    (srcdir / "final.ubm").write_bytes(UR.full_gmm_bytes(w, b, ic, True))
    (srcdir / "delta_opts").write_text("--delta-window=3 --delta-order=2\n")
    m = R.random_model(8, G, D, S)
    (srcdir / "final.ie").write_bytes(R.ie_bytes(**m))
    rng = np.random.default_rng(4)
    lens = {"spk1-a": 150, "spk1-b": 41, "spk2-a": 97, "spk2-b": 60, "spk3-a": 33}
    keys = sorted(lens)
    utts = [(k, rng.normal(0.0, 4.0, size=(lens[k], 20)).astype(np.float32)) for k in keys]
    # spk2-b has no voiced frame: select-voiced-frames drops it;  spk1-b is missing from the posteriors
    vads = [(k, np.zeros(lens[k], np.float32) if k == "spk2-b" else (rng.uniform(size=lens[k]) < 0.8).astype(np.float32)) for k in keys]
    kio.write_ark_matrices(str(sdata / "raw.ark"), utts, scp_path=str(sdata / "feats.scp"))
    kio.write_ark_vectors(str(sdata / "vad.ark"), vads, scp_path=str(sdata / "vad.scp"))
    with open(sdata / "feats.scp") as f:
        (sdata / "feats4.scp").write_text("".join(l for l in f if not l.startswith("spk1-b")))

    # extract_ivectors.sh:55-70, the strings as the script builds them (JOB = 1)
    delta_opts = (srcdir / "delta_opts").read_text().strip()
    feats = ("ark,s,cs:add-deltas %s scp:%s/feats.scp ark:- | apply-cmvn-sliding --norm-vars=false --center=true --cmn-window=300 ark:- ark:- | "
             "select-voiced-frames ark:- scp,s,cs:%s/vad.scp ark:- |" % (delta_opts, sdata, sdata))
    dubm = "fgmm-global-to-gmm %s/final.ubm -|" % srcdir
    upstream = ('gmm-gselect --n=20 "%s" "%s" ark:- | fgmm-global-gselect-to-post --min-post=0.025 %s/final.ubm "%s" ark,s,cs:- ark:- | '
                'scale-post ark:- 1.0 ark:-' % (dubm, feats, srcdir, feats))
    extract = 'ivector-extract --verbose=2 %s/final.ie "%s" ark,s,cs:- ark,scp,t:%s/ivector.1.ark,%s/ivector.1.scp' % (srcdir, feats, out, out)
    r = _sh(upstream.replace("feats.scp", "feats4.scp") + " | " + extract)
    log = r.stderr.decode()
    assert r.returncode == 0, log
    done = [k for k in keys if k not in ("spk1-b", "spk2-b")]
    assert "No posteriors for utterance spk1-b" in log
    assert re.search(r"LOG \(ivector-extract.*Done 3 files, 1 with errors\.  Total \(weighted\) frames \S+", log), log
    assert re.search(r"Overall average objective-function change from estimating ivector was \S+ per frame", log), log
    for k in done:
        assert re.search(r"Auxf change for utterance %s was \S+ per frame over \S+ frames \(weighted\)" % k, log), log
        assert re.search(r"Ivector norm for utterance %s was \S+" % k, log), log
    got = _read_text_vectors((out / "ivector.1.ark").read_bytes())
    assert [k for k, _ in got] == done
    assert [l.split()[0] for l in (out / "ivector.1.scp").read_text().splitlines()] == done

    # the same through the C ABI, on the features and the posteriors the tools themselves make
    r2 = _sh(feats[len("ark,s,cs:"):] + " cat > %s/prepared.ark" % tmp_path)
    assert r2.returncode == 0, r2.stderr
    prepared = dict(kio.read_ark(str(tmp_path / "prepared.ark")))
    assert sorted(prepared) == [k for k in keys if k != "spk2-b"]
    r3 = _sh(upstream)
    assert r3.returncode == 0, r3.stderr
    post = dict(UR.read_post_table(r3.stdout))
    ie = P.IvectorExtractor.load(str(srcdir / "final.ie"))
    as_arrays = lambda frames: [(np.array([i for i, _ in f], np.int32), np.array([q for _, q in f], np.float32)) for f in frames]
    iv, status, auxf = ie.extract([prepared[k] for k in done], [as_arrays(post[k]) for k in done])
    assert not status.any()
    for (k, v), want in zip(got, iv):
        assert np.array_equal(v.view(np.uint32), want.view(np.uint32)), k

    # extract_ivectors.sh:75 and 83-85 on the result
    (out / "ivector.scp").write_text((out / "ivector.1.scp").read_text())
    (tmp_path / "spk2utt").write_text("spk1 spk1-a spk1-b\nspk2 spk2-a spk2-b\nspk3 spk3-a\n")
    r = _sh("ivector-normalize-length scp:%s/ivector.scp  ark:- | ivector-mean ark:%s/spk2utt ark:- ark:- ark,t:%s/num_utts.ark | "
            "ivector-normalize-length ark:- ark,scp:%s/spk_ivector.ark,%s/spk_ivector.scp" % (out, tmp_path, out, out, out))
    assert r.returncode == 0, r.stderr
    assert [l.split()[0] for l in (out / "spk_ivector.scp").read_text().splitlines()] == ["spk1", "spk2", "spk3"]
    assert (out / "num_utts.ark").read_text().split() == ["spk1", "1", "spk2", "1", "spk3", "1"]

    # a posterior that names a Gaussian the model does not have is fatal
    bad = [(k, [[(G, q) if j == 0 and t == 3 else (i, q) for j, (i, q) in enumerate(f)] for t, f in enumerate(post[k])]) for k in done]
    (tmp_path / "bad.ark").write_bytes(UR.post_table_bytes(bad, True))
    r = _sh('ivector-extract %s/final.ie "%s" ark:%s/bad.ark ark:/dev/null' % (srcdir, feats, tmp_path))
    assert r.returncode == 255 and b"ERROR (ivector-extract" in r.stderr and b"name Gaussian 21" in r.stderr


def test_a_posterior_a_frame_short_is_warned_about_and_counted(tmp_path):
    G, D, S = 4, 6, 5
    (tmp_path / "final.ie").write_bytes(R.ie_bytes(**R.random_model(9, G, D, S)))
    rng = np.random.default_rng(10)
    lens = {"a": 5, "b": 4, "c": 6}
    kio.write_ark_matrices(str(tmp_path / "f.ark"), [(k, rng.normal(size=(n, D)).astype(np.float32)) for k, n in lens.items()])
    post = {k: [[(int(rng.integers(0, G)), 1.0)] for _ in range(n)] for k, n in lens.items()}
    post["b"] = post["b"][:-1]
    (tmp_path / "p.post").write_bytes(UR.post_table_bytes(sorted(post.items()), True))
    r = _sh("timeout -k 10 120 ivector-extract final.ie ark,s,cs:f.ark ark,s,cs:p.post ark,t:iv.ark", cwd=str(tmp_path))
    log = r.stderr.decode()
    assert r.returncode == 0, log
    assert log.count(") Size mismatch between posterior 3 and features 4 for utterance b\n") == 1, log
    assert re.search(r"LOG \(ivector-extract\S* Done 2 files, 1 with errors\.  Total \(weighted\) frames \S+\n", log), log
    assert [k for k, _ in _read_text_vectors((tmp_path / "iv.ark").read_bytes())] == ["a", "c"]
