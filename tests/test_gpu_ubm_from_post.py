"""The supervised UBM of the phonetic i-vector path: fgmm-global-acc-stats-post against the numpy restatement of the accumulation
(tests/ubm_train_ref.py), and sid/init_full_ubm_from_nnet3.sh:118-136, sid/extract_post_nnet3.sh:85-91 and the i-vector tools that
read their results, with the scripts' argv."""
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
U = 2.0 ** -24
LIMIT = "timeout -k 10 120 "

_HDR = open(os.path.join(H.ROOT, H.PKG_NAME, "csrc", "ubm_train_kernels.h")).read()
C = int(re.search(r"kFgmmAccPairChunk = (\d+);", _HDR).group(1))
FB = int(re.search(r"kFgmmAccFrameBlock = (\d+);", _HDR).group(1))
LENGTHS = [0, 1, 3, 4, 5, C - 1, C, C + 1, 2 * C + 3]   # the bucket lengths of tests/test_gpu_ubm_train.py's integer case
G = len(LENGTHS)
D = 17


def _sh(line, cwd=None):
    env = dict(os.environ, PATH=BIN + os.pathsep + os.environ.get("PATH", ""))
    return subprocess.run(["/bin/sh", "-c", line], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, cwd=cwd, timeout=300)


@functools.lru_cache(maxsize=None)
def integer_case(copies):
    """the integer case of tests/test_gpu_ubm_train.py, rebuilt from ubm_train_ref and laid end to end `copies` times: integer frames
    in [-4, 4], posteriors that are multiples of 2^-10, pairs dealt over frames of 0 to 4 pairs, frame 0 naming Gaussian 8 twice.
    -> (x, post per frame, the restatement's sums, which are exact in any order)"""
    rng = np.random.default_rng(0)
    gauss = rng.permutation(np.repeat(np.arange(G), LENGTHS))
    first = np.nonzero(gauss == 8)[0][:2]
    gauss = np.concatenate([gauss[first], gauss[np.delete(np.arange(len(gauss)), first)]])
    counts = [2]
    while sum(counts) < len(gauss):
        counts.append(min(int(rng.integers(0, 5)), len(gauss) - sum(counts)))
    gauss = np.tile(gauss, copies).astype(np.int32)
    counts = np.tile(counts, copies)
    off = np.concatenate([[0], np.cumsum(counts)])
    frame = np.repeat(np.arange(len(counts)), counts)
    rng = np.random.default_rng(1 + D)
    x = rng.integers(-4, 5, size=(len(counts), D)).astype(F)
    p = (rng.integers(1, 1025, size=len(gauss)) / 1024.0).astype(F)
    ref = T.acc_stats(x, frame, gauss, p, G, 7)
    assert T.abs_terms(x, frame, gauss, p, G)[2].max() * 2.0 ** 10 < 2.0 ** 53   # every partial sum is an exact double
    post = [list(zip(gauss[off[t]:off[t + 1]].tolist(), p[off[t]:off[t + 1]].tolist())) for t in range(len(counts))]
    return x, post, ref


def write_case(d, name, x, post, cuts, keys=None):
    keys = keys or ["utt%03d" % i for i in range(len(cuts) - 1)]
    kio.write_ark_matrices(str(d / (name + ".ark")), [(k, x[cuts[i]:cuts[i + 1]]) for i, k in enumerate(keys)])
    (d / (name + ".post")).write_bytes(R.post_table_bytes([(k, post[cuts[i]:cuts[i + 1]]) for i, k in enumerate(keys)], True))
    return keys


def test_the_integer_case_gives_the_restatements_sums_bit_for_bit(tmp_path):
    x, post, ref = integer_case(1)
    assert post[0][0][0] == post[0][1][0] == 8   # a Gaussian named twice in one frame adds twice
    write_case(tmp_path, "one", x, post, [0, len(x)])
    for flags in ("mw", "mvw"):   # one.acc ends up with all three
        r = _sh(LIMIT + "fgmm-global-acc-stats-post --update-flags=%s ark:one.post %d ark:one.ark one.acc" % (flags, G), cwd=str(tmp_path))
        assert r.returncode == 0, r.stderr
        assert b"Done 1 files; 0 with errors." in r.stderr and b"Written accs to one.acc" in r.stderr
        want = ref if flags == "mvw" else (ref[0], ref[1], np.zeros_like(ref[2]))
        assert (tmp_path / "one.acc").read_bytes() == T.accs_bytes(*want, T.augment_flags(T.parse_flags(flags)), True)
    # text out, and fgmm-global-sum-accs reads it
    r = _sh(LIMIT + "fgmm-global-acc-stats-post --binary=false ark,s,cs:one.post %d ark,s,cs:one.ark one.txt && fgmm-global-sum-accs sum.acc one.txt one.acc" % G, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr
    assert (tmp_path / "one.txt").read_bytes()[:9] == b"<GMMACCS>"
    assert (tmp_path / "sum.acc").read_bytes() == T.accs_bytes(*[2.0 * a for a in ref], 7, True)   # doubling is exact


def test_the_statistics_do_not_depend_on_how_the_frames_are_cut_into_utterances(tmp_path):
    """more than one block of kFgmmAccFrameBlock frames, as 1, 3 and 7 utterances: the second of three and the sixth of seven straddle
    the block boundary, the posteriors once sorted and merged, once loaded"""
    copies = FB // len(integer_case(1)[0]) + 1
    x, post, ref = integer_case(copies)
    rows = len(x)
    assert FB < rows < 2 * FB
    want = T.accs_bytes(*ref, 7, True)
    for name, cuts, spec in (("one", [0, rows], "ark,s,cs"), ("three", [0, 9001, FB + 300, rows], "ark"),
                             ("seven", [0, 1, 2000, 2003, 9000, FB - 1, FB + 1, rows], "ark,s,cs")):
        assert any(a < FB < b for a, b in zip(cuts[:-1], cuts[1:]))
        write_case(tmp_path, name, x, post, cuts)
        r = _sh(LIMIT + "fgmm-global-acc-stats-post %s:%s.post %d ark:%s.ark %s.acc" % (spec, name, G, name, name), cwd=str(tmp_path))
        assert r.returncode == 0, r.stderr
        assert ("Done %d files; 0 with errors." % (len(cuts) - 1)).encode() in r.stderr
        assert (tmp_path / (name + ".acc")).read_bytes() == want, name


def test_missing_and_wrong_posteriors_are_warned_about_and_counted(tmp_path):
    x, post, _ = integer_case(1)
    cuts = [0, 100, 250, 400, 600]
    keys = ["a", "b", "c", "d"]
    write_case(tmp_path, "f", x, post, cuts, keys)
    # no posterior for b, one frame too few for c
    table = [("a", post[0:100]), ("c", post[250:399]), ("d", post[400:600])]
    (tmp_path / "p.post").write_bytes(R.post_table_bytes(table, True))
    r = _sh(LIMIT + "fgmm-global-acc-stats-post ark,s,cs:p.post %d ark,s,cs:f.ark f.acc" % G, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr
    log = r.stderr.decode()
    assert "WARNING (fgmm-global-acc-stats-post" in log and "No posterior for utterance b" in log
    assert "The posterior of utterance c has wrong size 149 vs. 150" in log and "Done 2 files; 2 with errors." in log
    # what was accumulated: a and d
    keep = list(range(0, 100)) + list(range(400, 600))
    frame, gauss, p = T.post_pairs([(np.array([g for g, _ in post[t]], np.int64), np.array([q for _, q in post[t]], F)) for t in keep])
    assert (tmp_path / "f.acc").read_bytes() == T.accs_bytes(*T.acc_stats(x[keep], frame, gauss, p, G, 7), 7, True)
    # nothing accepted: status 1
    (tmp_path / "none.post").write_bytes(R.post_table_bytes([("zzz", post[0:3])], True))
    r = _sh(LIMIT + "fgmm-global-acc-stats-post ark:none.post %d ark:f.ark none.acc" % G, cwd=str(tmp_path))
    assert r.returncode == 1 and b"Done 0 files; 4 with errors." in r.stderr
    # an index outside [0, num-components) is an error that names it
    r = _sh(LIMIT + "fgmm-global-acc-stats-post ark:p.post %d ark:f.ark bad.acc" % (G - 1), cwd=str(tmp_path))
    assert r.returncode == 255 and re.search(rb"the posterior of utterance \S+ names Gaussian 8 at frame \d+; <num-components> is 8", r.stderr), r.stderr
    assert not (tmp_path / "bad.acc").exists()


# ------------------------------------------------------------------------------------------------------------------- the recipes
def test_the_phonetic_baseline_runs_with_the_recipes_argv(tmp_path):
    nj, senones, S = 2, 40, 6
    nnet, data, data_dnn, dir_, post_dir, ie_dir = (tmp_path / n for n in ("nnet", "sid", "dnn", "full_ubm", "post", "extractor"))
    sdata, sdata_dnn = data / "split2", data_dnn / "split2"
    for p in (nnet, dir_, post_dir, ie_dir, sdata / "1", sdata / "2", sdata_dnn / "1", sdata_dnn / "2"):
        p.mkdir(parents=True)
    # an acoustic model with 40 senones, in the final.mdl container.  The head is small enough for flat posteriors: most are above
    # min_post, the others are pruned at random, and every senone keeps hundreds of frames, so that every Gaussian can be initialised
    net = H.nm.synthesize([H.config_text("am").replace("5139", str(senones))], seed=5, head_stddev=0.02)
    raw = net.to_bytes(True)
    (nnet / "final.mdl").write_bytes(b"\x00B<TransitionModel> " + bytes(range(256)) + b"</TransitionModel> " + raw[2:] +
                                     b"<LeftContext> \x04\x0d\x00\x00\x00<RightContext> \x04\x07\x00\x00\x00<Priors> FV \x04\x00\x00\x00\x00")
    rng = np.random.default_rng(6)
    jobs = {1: ["spkA-u1", "spkA-u2"], 2: ["spkB-u1"]}
    lens = {"spkA-u1": 260, "spkA-u2": 180, "spkB-u1": 310}
    voiced = {}
    for j, keys in jobs.items():
        dnn = [(k, H.features(300 + i + 10 * j, lens[k])) for i, k in enumerate(keys)]                      # 23-dimensional, for the network
        sid = [(k, rng.normal(0.0, 3.0, size=(lens[k], 4)).astype(F)) for k in keys]                        # 4 + deltas = 12, for the UBM
        vads = [(k, (rng.uniform(size=lens[k]) < 0.9).astype(F)) for k in keys]
        voiced.update({k: int(v.sum()) for k, v in vads})
        kio.write_ark_matrices(str(sdata_dnn / str(j) / "raw.ark"), dnn, scp_path=str(sdata_dnn / str(j) / "feats.scp"))
        kio.write_ark_matrices(str(sdata / str(j) / "raw.ark"), sid, scp_path=str(sdata / str(j) / "feats.scp"))
        kio.write_ark_vectors(str(sdata / str(j) / "vad.ark"), vads, scp_path=str(sdata / str(j) / "vad.scp"))
        (sdata_dnn / str(j) / "utt2spk").write_text("".join("%s %s\n" % (k, k.split("-")[0]) for k in keys))
        (sdata_dnn / str(j) / "spk2utt").write_text("".join("%s %s\n" % (s, " ".join(k for k in keys if k.startswith(s))) for s in sorted({k.split("-")[0] for k in keys})))
        r = _sh("compute-cmvn-stats --spk2utt=ark:%s/spk2utt scp:%s/feats.scp ark,scp:%s/cmvn.ark,%s/cmvn.scp" % ((sdata_dnn / str(j),) * 4))
        assert r.returncode == 0, r.stderr

    def run_jobs(line):
        for j in range(1, nj + 1):
            r = _sh(line.replace("JOB", str(j)))
            assert r.returncode == 0, r.stderr.decode()
            yield j, r.stderr.decode()

    # init_full_ubm_from_nnet3.sh:54, 71-79, 91
    nnet_raw = "nnet3-am-copy --raw=true %s/final.mdl - |" % nnet
    delta_opts = "--delta-window=3 --delta-order=2"
    feats = ("ark,s,cs:add-deltas %s scp:%s/JOB/feats.scp ark:- | apply-cmvn-sliding --norm-vars=false --center=true --cmn-window=300 ark:- ark:- | "
             "select-voiced-frames ark:- scp,s,cs:%s/JOB/vad.scp ark:- |" % (delta_opts, sdata, sdata))
    nnet_feats = "ark,s,cs:apply-cmvn  --utt2spk=ark:%s/JOB/utt2spk scp:%s/JOB/cmvn.scp scp:%s/JOB/feats.scp ark:- |" % ((sdata_dnn,) * 3)
    r = _sh("nnet3-info \"%s\" | grep 'output-node' | grep -oP 'dim=\\K[0-9]+'" % nnet_raw)
    assert r.returncode == 0 and r.stdout == b"40\n", r.stderr
    num_components = int(r.stdout)
    # :118-126
    to_post = ('%snnet3-compute --use-gpu=no "%s" "%s" ark:- | select-voiced-frames ark:- "scp,s,cs:%s/JOB/vad.scp" ark:- | %slogprob-to-post ark:- ark:- | '
               % (LIMIT, nnet_raw, nnet_feats, sdata, LIMIT))
    # (a tee between the two tools keeps the posteriors for the restatement below; every tool's argv is the script's)
    for j, log in run_jobs(to_post + 'tee %s/post.JOB.ark | %sfgmm-global-acc-stats-post ark:- %d "%s" "%s/stats.JOB.acc"' % (tmp_path, LIMIT, num_components, feats, dir_)):
        assert "Done %d files; 0 with errors." % len(jobs[j]) in log and "Done %d utterances; 0 with errors." % len(jobs[j]) in log
        assert re.search(r"%d frames in, \d+ pairs out, \S+ pairs per frame\." % sum(voiced[k] for k in jobs[j]), log), log
    # :133-136
    r = _sh('fgmm-global-init-from-accs --verbose=2 "fgmm-global-sum-accs - %s/stats.*.acc |" %d %s/final.ubm' % (dir_, num_components, dir_))
    assert r.returncode == 0, r.stderr
    assert b"Summed 2 stats" in r.stderr and b"Written model to" in r.stderr

    # the same from the restatement: the posteriors that went through the pipe, and the frames of the feature pipeline
    stats, tool_stats = [], []
    for j in range(1, nj + 1):
        r = _sh(feats[len("ark,s,cs:"):].replace("JOB", str(j)) + " cat > %s/feats.%d.ark" % (tmp_path, j))
        assert r.returncode == 0, r.stderr
        x = np.concatenate([m for _, m in kio.read_ark(str(tmp_path / ("feats.%d.ark" % j)))])
        posts = R.read_post_table((tmp_path / ("post.%d.ark" % j)).read_bytes())
        assert [k for k, _ in posts] == jobs[j] and [len(p) for _, p in posts] == [voiced[k] for k in jobs[j]]
        per_frame = [(np.array([g for g, _ in f], np.int64), np.array([q for _, q in f], F)) for _, p in posts for f in p]
        assert len(per_frame) == len(x) and x.shape[1] == 12
        frame, gauss, p = T.post_pairs(per_frame)
        assert gauss.min() >= 0 and gauss.max() < senones and 1.0 < len(gauss) / len(x) <= senones
        ref = T.acc_stats(x, frame, gauss, p, senones, 7)
        got = T.read_accs((dir_ / ("stats.%d.acc" % j)).read_bytes())
        # the bound of test_random_sums_are_within_the_summation_bound (n_g 2^-52 sum |terms|: any order, exact products), plus the
        # one rounding to float32 of the file
        a_occ, a_mean, a_cov, n_g = T.abs_terms(x, frame, gauss, p, senones)
        for name, want, s in zip(("occ", "mean", "cov"), ref, (a_occ, a_mean, a_cov)):
            bound = (n_g.reshape((-1,) + (1,) * (s.ndim - 1)) * 2.0 ** -52) * s + U * np.abs(want)
            assert np.all(np.abs(got[name].astype(np.float64) - want) <= bound), (j, name)
        stats.append([np.asarray(a, F).astype(np.float64) for a in ref])          # as the file holds them
        tool_stats.append([got[n].astype(np.float64) for n in ("occ", "mean", "cov")])
    final = R.read_full_gmm((dir_ / "final.ubm").read_bytes())
    # fgmm-global-sum-accs adds in fp64 and rounds once; the model of the tool's own sums is the binding's, bit for bit
    tool_sum = [(a + b).astype(F).astype(np.float64) for a, b in zip(*tool_stats)]
    own = P.fgmm_init_from_accs(*tool_sum)
    assert len(final["weights"]) == senones - len(own["removed"])
    for name in ("weights", "means_invcovars", "inv_covars"):
        assert np.array_equal(final[name], own[name]), name
    # and the restatement's sums give the same Gaussians, within what the float32 statistics allow: an element of cov / occ is off by at
    # most 3 2^-24 |S| (S = the second moment: one rounding per file, one of the sum, one of occ), and (C + E)^-1 - C^-1 is, to first
    # order, at most ||C^-1||^2 ||E|| in norm; ||E|| <= D max |E_ij|.  The mean term has the same shape.  8 instead of 3 for the rest.
    ref_sum = [(a + b).astype(F).astype(np.float64) for a, b in zip(*stats)]
    want = P.fgmm_init_from_accs(*ref_sum)
    assert want["removed"] == own["removed"] == [] and len(final["weights"]) == senones
    assert np.all(np.abs(final["weights"] - want["weights"]) <= 8 * U * want["weights"])   # occ_g and the total: 3 roundings each, and the weight's
    keep = [g for g in range(senones) if g not in want["removed"]]
    worst = 0.0
    for i, g in enumerate(keep):
        inv = R.unpack(want["inv_covars_f64"][i], 12)
        second = R.unpack(ref_sum[2][g], 12) / ref_sum[0][g]
        bound = 8 * U * 12 * np.abs(second).max() * np.linalg.norm(inv, 2) ** 2
        err = np.abs(R.unpack(final["inv_covars"][i].astype(np.float64), 12) - inv).max()
        worst = max(worst, err / bound)
        assert err <= bound, (g, err, bound)
    print("final.ubm against the restatement's statistics: worst error / bound = %.3g" % worst)
    assert np.all(np.isfinite(final["gconsts"]))

    # extract_post_nnet3.sh:85-91
    min_post, posterior_scale = 0.025, 1.0
    line = ('%snnet3-compute --use-gpu=no "%s" "%s" ark:- | select-voiced-frames ark:- scp,s,cs:%s/JOB/vad.scp ark:- | %slogprob-to-post --min-post=%s ark:- ark:- | '
            'scale-post ark:- %s "ark:|gzip -c >%s/post.JOB.gz"' % (LIMIT, nnet_raw, nnet_feats, sdata, LIMIT, min_post, posterior_scale, post_dir))
    for j, log in run_jobs(line):
        assert "Done %d utterances; 0 with errors." % len(jobs[j]) in log
        table = R.read_post_table(gzip.open(str(post_dir / ("post.%d.gz" % j))).read())
        assert [k for k, _ in table] == jobs[j] and [len(p) for _, p in table] == [voiced[k] for k in jobs[j]]
        assert all(q >= F(min_post) for _, p in table for f in p for _, q in f)

    # train_ivector_extractor_nnet3.sh:110-113, one pass of :123-147, extract_ivectors_nnet3.sh:56-58
    (ie_dir / "final.ubm").write_bytes((dir_ / "final.ubm").read_bytes())
    r = _sh("fgmm-global-to-gmm %s/final.ubm %s/final.dubm && ivector-extractor-init --ivector-dim=%d --use-weights=false %s/final.ubm %s/0.ie" % (ie_dir, ie_dir, S, ie_dir, ie_dir))
    assert r.returncode == 0, r.stderr
    args = ["%sivector-extractor-acc-stats --num-threads=4 --num-samples-for-weights=3 %s/0.ie '%s' 'ark,s,cs:gunzip -c %s/post.JOB.gz|' -|"
            .replace("JOB", str(j)) % (LIMIT, ie_dir, feats.replace("JOB", str(j)), post_dir) for j in (1, 2)]
    r = _sh(LIMIT + 'ivector-extractor-sum-accs --parallel=true "%s" "%s" %s/acc.0.1' % (args[0], args[1], ie_dir))
    assert r.returncode == 0, r.stderr.decode()
    r = _sh("ivector-extractor-sum-accs %s/acc.0.1 %s/acc.0 && ivector-extractor-est --num-threads=4 %s/0.ie %s/acc.0 %s/1.ie" % ((ie_dir,) * 5))
    assert r.returncode == 0, r.stderr
    os.rename(str(ie_dir / "1.ie"), str(ie_dir / "final.ie"))
    r = _sh((LIMIT + 'ivector-extract --verbose=2 %s/final.ie "%s" "ark,s,cs:gunzip -c %s/post.1.gz|" ark,scp,t:%s/ivector.1.ark,%s/ivector.1.scp')
            % (ie_dir, feats.replace("JOB", "1"), post_dir, tmp_path, tmp_path))
    assert r.returncode == 0, r.stderr
    assert re.search(rb"Done 2 files, 0 with errors", r.stderr), r.stderr
    vecs = [l.split() for l in (tmp_path / "ivector.1.ark").read_text().splitlines() if l.strip()]
    assert [v[0] for v in vecs] == jobs[1] and all(len(v) == S + 3 for v in vecs)
    assert np.all(np.isfinite(np.array([[float(t) for t in v[2:-1]] for v in vecs])))


def test_a_short_posterior_is_counted_and_a_matrix_without_rows_is_not(tmp_path):
    x, post, _ = integer_case(1)
    write_case(tmp_path, "f", x, post, [0, 5, 9, 9, 15], ["a", "b", "c", "d"])   # c has no rows
    (tmp_path / "p.post").write_bytes(R.post_table_bytes([("a", post[0:5]), ("b", post[5:8]), ("c", []), ("d", post[9:15])], True))
    r = _sh(LIMIT + "fgmm-global-acc-stats-post ark,s,cs:p.post %d ark,s,cs:f.ark f.acc" % G, cwd=str(tmp_path))
    log = r.stderr.decode()
    assert r.returncode == 0, log
    for text in (") The posterior of utterance b has wrong size 3 vs. 4\n", ") Empty feature matrix for utterance c\n", ") Done 2 files; 1 with errors.\n"):
        assert log.count(text) == 1, log
