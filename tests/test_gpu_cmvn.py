"""GPU tests of per-speaker CMVN (csrc/cmvn_kernels.hip): the fp64 statistics against exactly rounded sums, the fp32 application
against the numpy restatement tests/cmvn_ref.py for equality, and compute-cmvn-stats / apply-cmvn with the recipes' command lines."""
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import cmvn_ref as R
import helpers as H
from oracle import kaldi_io as kio

pytestmark = pytest.mark.gpu
P = H.pkg()
BIN = os.path.join(H.ROOT, H.PKG_NAME, "bin")

# the kernel's row block, read from its header: the row counts below straddle it
B = int(re.search(r"kCmvnRowBlock = (\d+);", open(os.path.join(H.ROOT, H.PKG_NAME, "csrc", "cmvn_kernels.h")).read()).group(1))
ROWS = [1, 2, B - 1, B, B + 1, 2 * B + 3]
COLS = [1, 23, 40, 65, 200]


@functools.lru_cache(maxsize=None)
def matrices(cols):
    rng = np.random.default_rng(100 + cols)
    # a large common offset: a sum that cancelled, or squares formed in float32, would show
    return tuple(rng.normal(50.0, 1.0, size=(r, cols)).astype(np.float32) for r in ROWS)


@functools.lru_cache(maxsize=None)
def device_stats(cols):
    return P.cmvn_stats(list(matrices(cols)))


@pytest.mark.parametrize("cols", COLS)
def test_statistics_are_within_the_summation_bound_of_the_exact_sums(cols):
    """Every sum and sum of squares against math.fsum of the same fp64 terms (cmvn_ref.stats; x * x of a float32 is exact in fp64).
    Bound, derived and not measured: an fp64 summation of n terms in ANY order - recursive, blocked, pairwise - commits n - 1
    additions, each with a relative error of at most u = 2^-53 on a partial sum no larger than sum |term| (1 + u)^(n - 1); hence
    |got - exact| <= (n - 1) u (1 + u)^(n - 1) sum |term| < n 2^-53 sum |term| (cmvn_ref.stats_bound)."""
    got = device_stats(cols)
    assert got.shape == (len(ROWS), 2, cols + 1) and got.dtype == np.float64
    for u, x in enumerate(matrices(cols)):
        exact, bound = R.stats(x), R.stats_bound(x)
        err = np.abs(got[u] - exact)
        print("rows %d cols %d: worst error / bound %.3g" % (x.shape[0], cols, float(np.max(err[:, :cols] / bound[:, :cols]))))
        assert np.all(err[:, :cols] <= bound[:, :cols]), (x.shape, float(err.max()))
        assert got[u, 0, cols] == x.shape[0] and got[u, 1, cols] == 0.0


@pytest.mark.parametrize("cols", [23, 65])
def test_an_utterance_has_the_same_bits_alone_and_in_a_batch(cols):
    rng = np.random.default_rng(7)
    others = [rng.normal(-3.0, 5.0, size=(int(r), cols)).astype(np.float32) for r in rng.integers(1, 3 * B, size=37)]
    for u, x in enumerate(matrices(cols)):
        alone = P.cmvn_stats([x])[0]
        k = (5 * u + 3) % 38
        inside = P.cmvn_stats(others[:k] + [x] + others[k:])[k]
        assert np.array_equal(alone.view(np.uint64), inside.view(np.uint64)), x.shape
        assert np.array_equal(alone.view(np.uint64), device_stats(cols)[u].view(np.uint64)), x.shape


@pytest.mark.parametrize("norm_vars", [False, True])
@pytest.mark.parametrize("cols", COLS)
def test_apply_equals_the_restatement_bit_for_bit(cols, norm_vars):
    mats = list(matrices(cols))
    # four norms in the table, from statistics of several matrices added together; utt_norm is not sorted
    groups = [[0, 3], [5], [1, 2, 4], [4, 5]]
    norms = np.stack([R.cmvn_norm(sum(R.stats(mats[i]) for i in g), norm_vars=norm_vars, skip_dims=(0,) if k == 2 else ())
                      for k, g in enumerate(groups)])
    utt_norm = [2, 0, 3, 3, 1, 0]
    got = P.apply_cmvn(mats, norms, utt_norm)
    for u, x in enumerate(mats):
        want = R.apply(x, norms[utt_norm[u]])
        assert got[u].shape == x.shape
        assert np.array_equal(got[u].view(np.uint32), want.view(np.uint32)), (x.shape, utt_norm[u])


# ---- the command lines ------------------------------------------------------------------------------------------------------------
def _run(tool, *args):
    return subprocess.run([os.path.join(BIN, tool)] + list(args), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    """A data directory as the recipes leave it: compressed feats ("CM", as make_mfcc.sh writes them), spk2utt, utt2spk.  spkB has
    one utterance; spkC-u2 is listed in spk2utt but has no features; spkD has statistics for none of its utterances."""
    d = tmp_path_factory.mktemp("cmvn_data")
    rng = np.random.default_rng(21)
    rows = {"spkA-u1": 2 * B + 3, "spkA-u2": 90, "spkA-u3": B, "spkB-u1": 131, "spkC-u1": 57, "spkC-u3": 300}
    raw = {k: (rng.normal(0, 1, size=(r, 23)) * np.linspace(20, 1, 23) + np.linspace(-30, 30, 23)).astype(np.float32) for k, r in rows.items()}
    kio.write_ark_matrices(str(d / "raw.ark"), sorted(raw.items()), scp_path=str(d / "feats.scp"), compressed="CM")
    spk2utt = {"spkA": ["spkA-u1", "spkA-u2", "spkA-u3"], "spkB": ["spkB-u1"], "spkC": ["spkC-u1", "spkC-u2", "spkC-u3"], "spkD": ["spkD-u1"]}
    (d / "spk2utt").write_text("".join("%s %s\n" % (s, " ".join(us)) for s, us in spk2utt.items()))
    (d / "utt2spk").write_text("".join("%s %s\n" % (u, s) for s, us in sorted(spk2utt.items()) for u in us))
    # the floats the stored objects stand for, as the library's host reader expands them; every expected value below is computed
    # from these.  The tools under test expand the same objects on the device (cm_expand), which tests/test_gpu_frontend.py holds
    # to the host reader's bits: a bit-for-bit mismatch below that is not reproduced from uncompressed features would be a
    # difference between the two expansions, not a CMVN bug.
    r = _run("copy-feats", "scp:%s/feats.scp" % d, "ark:%s/expanded.ark" % d)
    assert r.returncode == 0, r.stderr
    feats = dict(kio.read_ark(str(d / "expanded.ark")))
    assert sorted(feats) == sorted(raw)
    return d, feats, spk2utt


def _check_stats(got, mats):
    # the statistics of several utterances added: the same bound with n the number of frames of all of them (the device's sums and
    # the host's additions of utterance statistics are together one fp64 summation of those n terms, in some order)
    allx = np.concatenate(mats, axis=0)
    exact, bound = R.stats(allx), R.stats_bound(allx)
    cols = exact.shape[1] - 1
    assert got.shape == exact.shape
    assert np.all(np.abs(got - exact)[:, :cols] <= bound[:, :cols])
    assert got[0, cols] == allx.shape[0] and got[1, cols] == 0.0


def test_compute_cmvn_stats_per_speaker_with_the_recipes_line(data):
    d, feats, spk2utt = data
    # steps/compute_cmvn_stats.sh:104
    r = _run("compute-cmvn-stats", "--spk2utt=ark:%s/spk2utt" % d, "scp:%s/feats.scp" % d, "ark,scp:%s/cmvn.ark,%s/cmvn.scp" % (d, d))
    assert r.returncode == 0, r.stderr
    assert re.search(r"WARNING \(compute-cmvn-stats.*Did not find features for utterance spkC-u2", r.stderr)
    assert re.search(r"WARNING \(compute-cmvn-stats.*Did not find features for utterance spkD-u1", r.stderr)
    assert re.search(r"WARNING \(compute-cmvn-stats.*No stats accumulated for speaker spkD", r.stderr)
    assert re.search(r"LOG \(compute-cmvn-stats.*Done accumulating CMVN stats for 6 utterances; 2 had errors\.", r.stderr)
    got = R.read_double_matrices(str(d / "cmvn.ark"))
    assert list(got) == ["spkA", "spkB", "spkC"]
    assert [l.split()[0] for l in open(d / "cmvn.scp")] == ["spkA", "spkB", "spkC"]
    for spk, st in got.items():
        _check_stats(st, [feats[u] for u in spk2utt[spk] if u in feats])
    # a speaker is its utterances' statistics added in list order, in fp64: the single-utterance speaker IS its utterance
    per_utt = P.cmvn_stats([feats[u] for u in spk2utt["spkA"]] + [feats["spkB-u1"]])
    assert np.array_equal(got["spkB"], per_utt[3])
    assert np.array_equal(got["spkA"], (per_utt[0] + per_utt[1]) + per_utt[2])


def test_compute_cmvn_stats_per_utterance_and_global(data):
    d, feats, _ = data
    r = _run("compute-cmvn-stats", "scp:%s/feats.scp" % d, "ark:%s/utt_cmvn.ark" % d)
    assert r.returncode == 0, r.stderr
    assert re.search(r"Done accumulating CMVN stats for 6 utterances; 0 had errors\.", r.stderr)
    got = R.read_double_matrices(str(d / "utt_cmvn.ark"))
    assert list(got) == sorted(feats)
    for k, st in got.items():
        _check_stats(st, [feats[k]])
    r = _run("compute-cmvn-stats", "scp:%s/feats.scp" % d, "%s/global.stats" % d)
    assert r.returncode == 0, r.stderr
    assert re.search(r"LOG \(compute-cmvn-stats.*Wrote global CMVN stats to %s/global.stats" % re.escape(str(d)), r.stderr)
    assert re.search(r"Done accumulating CMVN stats for 6 utterances; 0 had errors\.", r.stderr)
    _check_stats(R.read_double_matrix_file(str(d / "global.stats")), [feats[k] for k in sorted(feats)])
    # nothing read: exit 1
    (d / "empty.scp").write_text("")
    r = _run("compute-cmvn-stats", "scp:%s/empty.scp" % d, "ark:%s/none.ark" % d)
    assert r.returncode == 1 and "Done accumulating CMVN stats for 0 utterances; 0 had errors." in r.stderr


def _apply(d, *opts):
    out = "%s/normed_%d.ark" % (d, abs(hash(opts)) % 10 ** 8)
    r = _run("apply-cmvn", *opts, "--utt2spk=ark:%s/utt2spk" % d, "scp:%s/cmvn.scp" % d, "scp:%s/feats.scp" % d, "ark:" + out)
    return r, (dict(kio.read_ark(out)) if r.returncode == 0 else None)


@pytest.mark.parametrize("opts,kw", [((), {}), (("--norm-vars=true",), {"norm_vars": True}),
                                     (("--norm-vars=true", "--skip-dims=0:22"), {"norm_vars": True, "skip_dims": (0, 22)}),
                                     (("--reverse=true",), {"reverse": True})])
def test_apply_cmvn_equals_the_restatement_fed_the_tools_own_statistics(data, opts, kw):
    d, feats, spk2utt = data
    if not os.path.exists(d / "cmvn.scp"):
        assert _run("compute-cmvn-stats", "--spk2utt=ark:%s/spk2utt" % d, "scp:%s/feats.scp" % d, "ark,scp:%s/cmvn.ark,%s/cmvn.scp" % (d, d)).returncode == 0
    stats = R.read_double_matrices(str(d / "cmvn.ark"))
    r, got = _apply(d, *opts)
    assert r.returncode == 0, r.stderr
    what = "mean and variance" if kw.get("norm_vars") else "mean"
    assert re.search(r"LOG \(apply-cmvn.*Applied cepstral %s normalization to 6 utterances, errors on 0" % what, r.stderr)
    assert list(got) == sorted(feats)
    utt2spk = {u: s for s, us in spk2utt.items() for u in us}
    for k, y in got.items():
        want = R.apply(feats[k], R.cmvn_norm(stats[utt2spk[k]], **kw))
        assert np.array_equal(y.view(np.uint32), want.view(np.uint32)), k


def test_apply_cmvn_skips_a_key_without_statistics_and_copies_without_means(data):
    d, feats, spk2utt = data
    if not os.path.exists(d / "cmvn.scp"):
        assert _run("compute-cmvn-stats", "--spk2utt=ark:%s/spk2utt" % d, "scp:%s/feats.scp" % d, "ark,scp:%s/cmvn.ark,%s/cmvn.scp" % (d, d)).returncode == 0
    stats = R.read_double_matrices(str(d / "cmvn.ark"))
    # spkB's utterance is mapped to a speaker the statistics do not have
    (d / "utt2spk_b").write_text(open(d / "utt2spk").read().replace("spkB-u1 spkB", "spkB-u1 spkZ"))
    r = _run("apply-cmvn", "--utt2spk=ark:%s/utt2spk_b" % d, "scp:%s/cmvn.scp" % d, "scp:%s/feats.scp" % d, "ark:%s/skip.ark" % d)
    assert r.returncode == 0, r.stderr
    assert re.search(r"WARNING \(apply-cmvn.*No normalization statistics available for key spkB-u1, producing no output for this utterance", r.stderr)
    assert re.search(r"Applied cepstral mean normalization to 5 utterances, errors on 1", r.stderr)
    got = dict(kio.read_ark("%s/skip.ark" % d))
    assert list(got) == [k for k in sorted(feats) if k != "spkB-u1"]
    for k, y in got.items():
        want = R.apply(feats[k], R.cmvn_norm(stats[k.split("-")[0]]))
        assert np.array_equal(y.view(np.uint32), want.view(np.uint32)), k
    r = _run("apply-cmvn", "--norm-means=false", "--utt2spk=ark:%s/utt2spk" % d, "scp:%s/cmvn.scp" % d, "scp:%s/feats.scp" % d, "ark:%s/copy.ark" % d)
    assert r.returncode == 0, r.stderr
    got = dict(kio.read_ark("%s/copy.ark" % d))
    assert list(got) == sorted(feats) and all(np.array_equal(got[k].view(np.uint32), feats[k].view(np.uint32)) for k in got)
    # one global matrix for every utterance; statistics of another width are fatal
    assert _run("compute-cmvn-stats", "scp:%s/feats.scp" % d, "%s/g.stats" % d).returncode == 0
    r = _run("apply-cmvn", "--norm-vars=true", "%s/g.stats" % d, "scp:%s/feats.scp" % d, "ark:%s/glob.ark" % d)
    assert r.returncode == 0, r.stderr
    g = R.cmvn_norm(R.read_double_matrix_file("%s/g.stats" % d), norm_vars=True)
    for k, y in kio.read_ark("%s/glob.ark" % d):
        assert np.array_equal(y.view(np.uint32), R.apply(feats[k], g).view(np.uint32)), k
    kio.write_ark_matrices("%s/wide.ark" % d, [("w", np.ones((4, 30), np.float32))], scp_path="%s/wide.scp" % d)
    r = _run("apply-cmvn", "%s/g.stats" % d, "scp:%s/wide.scp" % d, "ark:%s/no.ark" % d)
    assert r.returncode == 255 and "ERROR (apply-cmvn" in r.stderr and "Dimension mismatch" in r.stderr
