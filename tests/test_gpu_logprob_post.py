"""logprob-to-post on the device (csrc/post_kernels.h) against the numpy restatement (tests/logprob_post_ref.py): the kept set entry for
entry and in order, the kept values, batch independence, and the tool byte for byte against the binding."""
import functools
import os
import subprocess

import numpy as np
import pytest

import helpers as H
import logprob_post_ref as LP
import ubm_ref as R
from oracle import kaldi_io as kio

pytestmark = pytest.mark.gpu
P = H.pkg()
BIN = os.path.join(H.ROOT, H.PKG_NAME, "bin")
F = np.float32
MIN_POST = 0.01
# every p is far from min_post, and p / min_post (0.4, 0.07; 0 for -inf) is compared with multiples of 2^-24
VALUES = np.concatenate([np.log(np.array([0.5, 0.2, 0.03, 0.004, 0.0007])), [-np.inf]]).astype(F)
COLS = [1, 63, 64, 65, 257, 4099]   # around the wave (64) and the tile (256) edges, and many tiles
ROWS = [0, 1, 130]                  # 130: more than one workgroup of 4 rows, and a last one that is not full


@functools.lru_cache(maxsize=None)
def case(rows, cols, key="utt-a", seed=0):
    """(x, the fp64 restatement's posterior) - computed once, shared, and never written to"""
    rng = np.random.default_rng(1000 * seed + 7 * rows + cols)
    x = VALUES[rng.integers(0, len(VALUES), size=(rows, cols))]
    x.setflags(write=False)
    # the reference may decide in fp64 because nothing here is near a threshold: within 4 fp32 ulps of min_post or of u * min_post
    assert int(LP.near(x, key, MIN_POST, True).sum()) == 0
    return x, LP.logprob_to_post(x, key, MIN_POST, True, fp64=True)[0]


def ulps(got, want64):
    """|got - the fp64 value rounded to float32| in float32 ulps of that value"""
    w = np.asarray(want64, np.float64).astype(F)
    return np.abs(got.astype(np.float64) - w.astype(np.float64)) / np.spacing(np.abs(w)).astype(np.float64)


def check(post, ref, x, min_post=MIN_POST):
    assert len(post) == len(ref)
    worst = 0.0
    for r, ((gi, gw), (wi, ww)) in enumerate(zip(post, ref)):
        assert gi.dtype == np.int32 and gw.dtype == F
        assert gi.tolist() == wi.tolist(), (r, gi[:8], wi[:8])   # the kept set, entry for entry and in column order
        p64 = np.exp(x[r, wi].astype(np.float64))
        pruned = p64 < float(F(min_post))
        assert np.all(gw[pruned].view(np.uint32) == F(min_post).view(np.uint32))   # min_post's bits
        if (~pruned).any():
            # HIP documents 1 ulp for the device expf; one more for the rounding of the fp64 value to float32 (csrc/post_kernels.h)
            e = ulps(gw[~pruned], p64[~pruned])
            worst = max(worst, float(e.max()))
            assert np.all(e <= 2.0), (r, float(e.max()))
    return worst


@pytest.mark.parametrize("cols", COLS)
@pytest.mark.parametrize("rows", ROWS)
def test_the_kept_set_is_the_restatements(rows, cols):
    x, ref = case(rows, cols)
    post, details = P.logprob_to_post([x], ["utt-a"], MIN_POST, True, return_details=True)
    assert len(post) == 1 and details["num_nan"] == 0
    worst = check(post[0], ref, x)
    kept = sum(len(i) for i, _ in ref)
    print("rows %d cols %d: %d pairs, worst kept value %.2f ulp" % (rows, cols, kept, worst))
    if rows:
        small = sum(int((np.exp(x[r, i].astype(np.float64)) < 0.01).sum()) for r, (i, _) in enumerate(ref))
        assert kept > 0 and (small > 0 or rows * cols < 50)   # the random pruning did keep some of the small ones


def test_random_prune_false_min_post_zero_and_rows_that_come_out_full_or_empty():
    x, _ = case(130, 257)
    ref = LP.logprob_to_post(x, "utt-a", MIN_POST, False, fp64=True)[0]
    check(P.logprob_to_post([x], ["utt-a"], MIN_POST, False)[0], ref, x)
    assert all(np.all(np.exp(x[r, i].astype(np.float64)) > 0.01) for r, (i, _) in enumerate(ref))
    # min_post = 0 keeps every column, -inf as 0; keys are not needed
    y = np.stack([x[0], np.full(257, -np.inf, F), np.full(257, -40.0, F)])
    for mp in (0.0, -1.0):
        post = P.logprob_to_post([y], ["k"], mp, True)[0]
        for r in range(3):
            assert post[r][0].tolist() == list(range(257))
            assert np.all(ulps(post[r][1], np.exp(y[r].astype(np.float64))) <= 2.0)
        assert not post[1][1].any() and np.all(post[0][1][x[0] == -np.inf] == 0)
    # with min_post = 0.01: -inf gives p = 0 and exp(-40) / 0.01 is below every u: both rows come out empty, and are there
    post = P.logprob_to_post([y], ["k"], MIN_POST, True)[0]
    assert len(post) == 3 and len(post[0][0]) > 0 and len(post[1][0]) == 0 and len(post[2][0]) == 0
    # NaN is dropped and counted, whatever min_post is
    z = y.copy()
    z[0, [3, 200]] = np.nan
    z[1, 256] = np.nan
    for mp in (0.0, MIN_POST):
        clean = P.logprob_to_post([y], ["k"], mp, True)[0]
        (post,), details = P.logprob_to_post([z], ["k"], mp, True, return_details=True)
        assert details["num_nan"] == 3
        assert post[0][0].tolist() == [j for j in clean[0][0].tolist() if j not in (3, 200)]
        assert post[1][0].tolist() == [j for j in clean[1][0].tolist() if j != 256]
        assert post[2][0].tolist() == clean[2][0].tolist()


def same(a, b):
    return len(a) == len(b) and all(np.array_equal(i, j) and np.array_equal(v.view(np.uint32), w.view(np.uint32)) for (i, v), (j, w) in zip(a, b))


def test_an_utterance_has_the_same_bits_alone_in_a_batch_and_under_any_frame_budget():
    cols = 257
    utts = [(("spk%d-utt" % i), case(n, cols, "spk%d-utt" % i, seed=i + 1)[0]) for i, n in enumerate((130, 1, 0, 63, 130))]
    keys, mats = [k for k, _ in utts], [m for _, m in utts]
    alone = [P.logprob_to_post([m], [k], MIN_POST, True)[0] for k, m in utts]
    for k, m, a in zip(keys, mats, alone):
        check(a, case(len(m), cols, k, seed=keys.index(k) + 1)[1], m)
    batch = P.logprob_to_post(mats, keys, MIN_POST, True)
    assert len(batch) == 5 and all(same(a, b) for a, b in zip(alone, batch))
    # 324 rows cut into launches of 7 and of 100 rows: utterances straddle launches
    for budget in (7, 100):
        assert all(same(a, b) for a, b in zip(alone, P.logprob_to_post(mats, keys, MIN_POST, True, frame_budget=budget)))
    # in another order, too
    back = P.logprob_to_post(mats[::-1], keys[::-1], MIN_POST, True)
    assert all(same(a, b) for a, b in zip(alone[::-1], back))


def test_the_key_changes_the_randomly_pruned_set_only():
    x, ref = case(130, 65)
    a = P.logprob_to_post([x], ["utt-a"], MIN_POST, True)[0]
    x2, ref2 = case(130, 65, "utt-b", seed=0)
    assert np.array_equal(x.view(np.uint32), x2.view(np.uint32))   # the same matrix
    b = P.logprob_to_post([x], ["utt-b"], MIN_POST, True)[0]
    check(b, ref2, x)
    big = np.exp(x.astype(np.float64)) >= 0.01
    differ = 0
    for r in range(130):
        (ia, wa), (ib, wb) = a[r], b[r]
        ka, kb = big[r, ia], big[r, ib]
        assert np.array_equal(ia[ka], ib[kb]) and np.array_equal(wa[ka].view(np.uint32), wb[kb].view(np.uint32))
        differ += ia[~ka].tolist() != ib[~kb].tolist()
    assert differ > 100


def _sh(line, cwd=None):
    env = dict(os.environ, PATH=BIN + os.pathsep + os.environ.get("PATH", ""))
    return subprocess.run(["/bin/sh", "-c", line], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, cwd=cwd, timeout=300)


def test_the_tool_writes_the_bindings_posteriors_byte_for_byte(tmp_path):
    utts = [("spk1-a", case(130, 257, "spk1-a", seed=11)[0]), ("spk1-b", np.zeros((0, 257), F)), ("spk2-a", case(63, 257, "spk2-a", seed=12)[0]),
            ("spk3-a", case(1, 65, "spk3-a", seed=13)[0])]   # another width: a batch of its own
    kio.write_ark_matrices(str(tmp_path / "logprob.ark"), utts)
    for min_post, prune in ((MIN_POST, True), (0.025, True), (MIN_POST, False)):
        want = [(k, [list(zip(i.tolist(), w.tolist())) for i, w in (P.logprob_to_post([m], [k], min_post, prune)[0] if len(m) else [])]) for k, m in utts]
        opts = "--min-post=%s --random-prune=%s" % (min_post, str(prune).lower())
        for spec, binary in (("ark", True), ("ark,t", False)):
            r = _sh("logprob-to-post %s ark:logprob.ark %s:post.out" % (opts, spec), cwd=str(tmp_path))
            assert r.returncode == 0, r.stderr
            assert (tmp_path / "post.out").read_bytes() == R.post_table_bytes(want, binary), (min_post, prune, spec)
            pairs = sum(len(f) for _, post in want for f in post)
            log = r.stderr.decode()
            assert "Done 4 utterances; 0 with errors." in log
            assert "194 frames in, %d pairs out, %s pairs per frame." % (pairs, ("%g" % (pairs / 194.0))) in log, log
    # defaults are --min-post=0.01 --random-prune=true; pipes in and out
    r = _sh("cat logprob.ark | logprob-to-post ark:- ark:- | cat > piped.out", cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr
    want = [(k, [list(zip(i.tolist(), w.tolist())) for i, w in (P.logprob_to_post([m], [k])[0] if len(m) else [])]) for k, m in utts]
    assert (tmp_path / "piped.out").read_bytes() == R.post_table_bytes(want, True)
    # NaN input: dropped, with a warning that counts
    bad = utts[0][1].copy()
    bad[5, 7] = bad[100, 256] = np.nan
    kio.write_ark_matrices(str(tmp_path / "nan.ark"), [("spk1-a", bad)])
    r = _sh("logprob-to-post ark:nan.ark ark:/dev/null", cwd=str(tmp_path))
    assert r.returncode == 0 and b"WARNING (logprob-to-post" in r.stderr and b"2 log-probabilities were NaN and were dropped" in r.stderr
    r = _sh("logprob-to-post ark:/dev/null ark:/dev/null", cwd=str(tmp_path))
    assert r.returncode == 1 and b"Done 0 utterances" in r.stderr
