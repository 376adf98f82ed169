"""The sliding-CMN front-end (cmn_prefix_kernel, cmn_select_kernel) over its option space, EXACTLY, on every way in: the
library call (P.cmvn_sliding -> FrontEndRun), Context.frontend, the apply-cmvn-sliding tool and the engine's in-flight
FrontEndJob behind nnet3-xvector-compute's recognised pipeline.

The reference is tests/cmn_sliding_ref.py: the window as a closed form and the window sum as an exact integer, pinned against
oracle/frontend.py and hand-computed windows by tests/test_cmn_sliding_ref.py.

WHY EQUALITY.  The features lie on the grid 2^-6 (x = k 2^-6, |k| <= 2^13 with the per-column offset) and a column's |k| add up
to less than 2^53 (below 2^29 at the longest utterance here; asserted, R.assert_exactness_precondition).  Every prefix value the
device forms is then an exact double in whatever order its segments are summed and combined, and so is the difference of two.
What remains is one fp64 division, one fp64 subtraction and one cast to fp32, each correctly rounded (the library is built without
fast-math) and each done the same way by numpy: bit equality is derived, not measured.  Only test_general_inputs, whose inputs
are off any grid, has a bound, and it is derived there.
"""
import functools
import os
import subprocess

import numpy as np
import pytest

import helpers as H
import cmn_sliding_ref as R
from oracle import frontend as fe
from oracle import kaldi_io as kio

pytestmark = pytest.mark.gpu
BIN = os.path.join(H.ROOT, H.PKG_NAME, "bin")

WINDOWS = (1, 2, 3, 7, 8, 299, 300, 301, 600, 10000)
MIN_WINDOWS = (0, 1, 50, 100, 101, 700)


def segments(cols):
    """cmn_prefix_kernel cuts the time axis into 1024 / dp segments, dp = 32 up to 32 columns and 64 beyond."""
    return 32 if cols <= 32 else 16


def sweep_lengths(cols):
    S = segments(cols)
    return [1, 2, S - 1, S, S + 1, 2 * S + 1, 99, 100, 101, 299, 300, 301, 650]


def same(got, ref, what):
    """Bit equality; the message names the first element that differs."""
    got = np.asarray(got)
    assert got.dtype == np.float32 and ref.dtype == np.float32 and got.shape == ref.shape, (what, got.shape, ref.shape)
    if got.tobytes() == ref.tobytes():
        return
    bad = np.argwhere(np.ascontiguousarray(got).view(np.uint32) != np.ascontiguousarray(ref).view(np.uint32))
    t, d = bad[0]
    pytest.fail("%s: %d of %d values differ, first at frame %d column %d: got %r, want %r"
                % (what, len(bad), got.size, t, d, float(got[t, d]), float(ref[t, d])))


@pytest.fixture(scope="module")
def ctxs():
    """Context.frontend needs a model whose input has the features' width: a tiny one per width."""
    P = H.pkg()
    out = {}
    for D in (23, 60):
        net = H.nm.synthesize(H.tiny_config(feat_dim=D), seed=5)
        out[D] = P.Context(P.Model(raw=net.to_bytes(True), nnet_config="output-node name=output input=tdnn6.affine"))
    return out


# ---------------------------------------------------------------------------------------------------------------- a. option sweep
@pytest.mark.parametrize("center", [True, False])
@pytest.mark.parametrize("cols", [1, 23, 32, 33, 60, 64])
def test_option_sweep(cols, center):
    """Both prefix layouts at their limits (32 segments up to 32 columns, 16 beyond), one ragged batch per option point whose
    lengths straddle the segment count, the minimum window and the window; every utterance compared alone."""
    P = H.pkg()
    lens = sweep_lengths(cols)
    utts = [R.dyadic_features(1000 * cols + T, T, cols) for T in lens]
    for x in utts:
        R.assert_exactness_precondition(x)
    for W in WINDOWS:
        for M in (MIN_WINDOWS if not center else (100,)):
            got = P.cmvn_sliding(utts, cmn_window=W, min_cmn_window=M, center=center)
            assert len(got) == len(utts)
            for T, x, g in zip(lens, utts, got):
                same(g, R.sliding_cmn(x, W, center, M), "W=%d M=%d center=%s T=%d cols=%d" % (W, M, center, T, cols))
        if center and W in (7, 300):   # centred: the minimum window is not used
            other = P.cmvn_sliding(utts, cmn_window=W, min_cmn_window=700, center=True)
            assert np.concatenate(other).tobytes() == np.concatenate(got).tobytes(), W


# --------------------------------------------------------------------------------------------------------------- b. long utterances
@pytest.mark.parametrize("cols", [23, 60])
@pytest.mark.parametrize("T", [9001, 40003])
def test_long_utterances(T, cols):
    """A 90-second recording, which the segmented prefix was written for, and one of 400 seconds: segments of 282 to 2501 frames."""
    P = H.pkg()
    x = R.dyadic_features(77 + T + cols, T, cols)
    R.assert_exactness_precondition(x)
    for W, center, M in ((300, True, 100), (600, False, 100)):
        got, = P.cmvn_sliding([x], cmn_window=W, min_cmn_window=M, center=center)
        same(got, R.sliding_cmn(x, W, center, M), "W=%d M=%d center=%s T=%d cols=%d" % (W, M, center, T, cols))


# ------------------------------------------------------------------------------------------------------------------- c. selection
def selection_batch(cols):
    lens = [120, 77, 301, 0, 650, 40, 333, 0]
    utts = [R.dyadic_features(300 + i, T, cols) for i, T in enumerate(lens)]
    vads = [np.ones(120, np.float32), np.zeros(77, np.float32), np.zeros(301, np.float32), np.zeros(0, np.float32),
            np.zeros(650, np.float32), (np.arange(40) % 2).astype(np.float32), fe.synthetic_vad(3, 333), np.zeros(0, np.float32)]
    vads[2][0] = 1.0          # only the first row
    vads[4][-1] = 1.0         # only the last row
    assert 0 < vads[6].sum() < 333
    return utts, vads


@pytest.mark.parametrize("center", [True, False])
@pytest.mark.parametrize("W", [7, 300, 601])
def test_selection_through_the_context(ctxs, W, center):
    """Context.frontend (minimum window 100): all kept, none kept (no rows out, neighbours intact), only the first row, only the
    last, alternating, runs, and utterances without frames in the middle and at the end of the batch."""
    utts, vads = selection_batch(23)
    for x in utts:
        R.assert_exactness_precondition(x)
    raw, offs = H.pack(utts)
    out, out_off = ctxs[23].frontend(raw, offs, np.concatenate(vads), cmn_window=W, center=center)
    kept = [int((v != 0).sum()) for v in vads]
    assert kept == [120, 0, 1, 0, 1, 20, kept[6], 0]
    assert out_off.tolist() == [0] + np.cumsum(kept).tolist()
    assert out.shape == (sum(kept), 23)
    for i, (x, v) in enumerate(zip(utts, vads)):
        same(out[out_off[i]:out_off[i + 1]], R.select(R.sliding_cmn(x, W, center, 100), v),
             "utterance %d W=%d M=100 center=%s T=%d" % (i, W, center, x.shape[0]))
    out2, off2 = ctxs[23].frontend(raw, offs, None, cmn_window=0, center=center)
    assert out2.tobytes() == raw.tobytes() and np.array_equal(off2, offs)


# ------------------------------------------------------------------------------------------------------------ d. batch independence
@pytest.mark.parametrize("cols", [23, 60])
def test_an_utterance_gives_the_same_bytes_in_any_batch(ctxs, cols):
    P = H.pkg()
    S = segments(cols)
    rng = np.random.default_rng(cols)
    target = R.dyadic_features(9000 + cols, 2 * S + 73, cols)
    tvad = fe.synthetic_vad(11, target.shape[0])
    assert 0 < tvad.sum() < target.shape[0]
    lens = rng.integers(0, 3 * S + 1, size=33)
    lens[[3, 20]] = 0
    others = [R.dyadic_features(9100 + i, int(T), cols) for i, T in enumerate(lens)]
    ovads = [fe.synthetic_vad(50 + i, int(T)) for i, T in enumerate(lens)]
    for W, center in ((300, True), (7, False)):
        ref = R.sliding_cmn(target, W, center, 100)
        alone, = P.cmvn_sliding([target], cmn_window=W, min_cmn_window=100, center=center)
        same(alone, ref, "alone W=%d center=%s cols=%d" % (W, center, cols))
        sel_alone, off_alone = ctxs[cols].frontend(target, [0, target.shape[0]], tvad, cmn_window=W, center=center)
        same(sel_alone, R.select(ref, tvad), "alone, selected W=%d center=%s cols=%d" % (W, center, cols))
        for pos in (0, 16, 32):
            batch = list(others)
            batch[pos] = target
            got = P.cmvn_sliding(batch, cmn_window=W, min_cmn_window=100, center=center)
            assert got[pos].tobytes() == alone.tobytes(), (W, center, pos)
            bv = list(ovads)
            bv[pos] = tvad
            raw, offs = H.pack(batch)
            out, out_off = ctxs[cols].frontend(raw, offs, np.concatenate(bv), cmn_window=W, center=center)
            assert out[out_off[pos]:out_off[pos + 1]].tobytes() == sel_alone.tobytes(), (W, center, pos)
            assert out_off.tolist() == [0] + np.cumsum([int((v != 0).sum()) for v in bv]).tolist()


# -------------------------------------------------------------------------------------------------------- e. the entry points agree
@pytest.mark.parametrize("W,center", [(7, False), (601, True)])
def test_the_library_call_and_the_context_agree(ctxs, W, center):
    P = H.pkg()
    utts = [R.dyadic_features(500 + T, T, 23) for T in (299, 700, 1)]
    raw, offs = H.pack(utts)
    want, want_off = ctxs[23].frontend(raw, offs, None, cmn_window=W, center=center)
    got = P.cmvn_sliding(utts, cmn_window=W, min_cmn_window=100, center=center)
    assert np.array_equal(want_off, offs)
    assert np.concatenate(got).tobytes() == want.tobytes()
    assert not np.array_equal(want, raw)


# ------------------------------------------------------------------------------------------------------------- f. general inputs
@pytest.mark.parametrize("offset", [1000.0, 0.0])
@pytest.mark.parametrize("cols", [23, 60])
@pytest.mark.parametrize("T", [301, 2000])
def test_general_inputs(T, cols, offset, capsys):
    """Gaussian features, off any grid, on a constant offset: |got - v| <= 2^-24 |v| + 2^-149 + E against the restatement's
    float64 value v (before its cast), n the window length, with

        E = 2 (T + 2) 2^-53 (sum over the utterance of |x|) / n  +  2^-52 (|x| + |mean|)

    First term: a prefix value is a sum of at most T doubles in SOME order, off by at most T 2^-53 sum|x| to first order; the
    difference of two doubles that, and its own rounding adds 2^-53 sum|x| at most: (2 T + 1) 2^-53 sum|x|, rounded up to
    2 (T + 2) for the higher-order terms, divided by n.  Second term: the division rounds by 2^-53 |mean| and the subtraction by
    2^-53 |x - mean|, on the device and in the restatement alike.  2^-24 |v| + 2^-149 is the cast to fp32.  Nothing is tuned.
    A mean or a subtraction in float is off by about 2^-24 * 1000 = 6e-5 at offset 1000: four orders above E.  (At offset 1000
    every value has the same exponent, so the sums are exact here too; offset 0 is the case whose prefix sums do round.)"""
    P = H.pkg()
    rng = np.random.default_rng(T + cols)
    x = (rng.standard_normal((T, cols)) + offset).astype(np.float32)
    x64 = x.astype(np.float64)
    tot = np.abs(x64).sum(axis=0)[None, :]
    for W, center, M in ((300, True, 100), (600, False, 100), (7, False, 0)):
        got, = P.cmvn_sliding([x], cmn_window=W, min_cmn_window=M, center=center)
        v = R.sliding_cmn(x, W, center, M, rounded=False)
        s, e = R.bounds(T, W, center, M)
        n = (e - s).astype(np.float64)[:, None]
        mean = x64 - v
        E = 2.0 * (T + 2) * 2.0 ** -53 * tot / n + 2.0 ** -52 * (np.abs(x64) + np.abs(mean))
        bound = 2.0 ** -24 * np.abs(v) + 2.0 ** -149 + E
        err = np.abs(got.astype(np.float64) - v)
        worst = np.unravel_index(np.argmax(err / bound), err.shape)
        with capsys.disabled():
            print("\n  general inputs T=%d cols=%d offset=%g W=%d M=%d center=%s: worst error / bound %.3g (error %.3g, E %.3g) at frame %d column %d"
                  % (T, cols, offset, W, M, center, (err / bound)[worst], err[worst], E[worst], worst[0], worst[1]))
        assert (err <= bound).all(), (W, M, center, worst, err[worst], bound[worst])


# ------------------------------------------------------------------------------------------------------------------- g. the tool
def _run(args, **kw):
    return subprocess.run(args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300, **kw)


@pytest.mark.parametrize("argv,W,M,center", [
    ([], 600, 100, False),                                                              # the tool's own defaults
    (["--center=false", "--cmn-window=200", "--min-cmn-window=50"], 200, 50, False),
    (["--cmn_window=7", "--center=true"], 7, 100, True),                                # the underscore spelling
    (["--min-cmn-window=0", "--center=false", "--cmn-window=200"], 200, 0, False),
])
def test_the_tool(tmp_path, argv, W, M, center):
    """apply-cmvn-sliding on a table of 23, then 40, then 23 columns (a batch holds one width: the tool flushes between them and
    keeps the key order) with an empty matrix in it (warned about, counted as an error)."""
    shapes = [("a", 250, 23), ("b", 90, 23), ("empty", 0, 23), ("c", 130, 40), ("d", 1, 40), ("e", 700, 23), ("f", 33, 23)]
    utts = [(k, R.dyadic_features(600 + i, T, D)) for i, (k, T, D) in enumerate(shapes)]
    for _, x in utts:
        R.assert_exactness_precondition(x)
    kio.write_ark_matrices(str(tmp_path / "in.ark"), utts)
    r = _run([os.path.join(BIN, "apply-cmvn-sliding")] + argv + ["ark:%s/in.ark" % tmp_path, "ark:%s/out.ark" % tmp_path])
    err = r.stderr.decode()
    assert r.returncode == 0, err[-1500:]
    assert "Empty feature matrix for utterance empty" in err, err[-1500:]
    assert "normalization to 6 utterances, 1 had errors" in err, err[-1500:]
    got = list(kio.read_ark(str(tmp_path / "out.ark"), "matrix"))
    assert [k for k, _ in got] == ["a", "b", "c", "d", "e", "f"]
    want = dict(utts)
    for k, g in got:
        same(g, R.sliding_cmn(want[k], W, center, M), "key %s W=%d M=%d center=%s T=%d cols=%d" % ((k, W, M, center) + want[k].shape))


# ------------------------------------------------------------------------------------- h. the engine's path, non-default options
ENGINE_BAR = 1e-4           # the suite's parity bar for x-vectors against the oracle
ENGINE_W = 200


@functools.lru_cache(maxsize=None)
def engine_case():
    """The utterances of test_the_engine_path_with_other_options, with the oracle's x-vectors of select(cmn(x)) for the options
    the test runs - (W = 200, not centred, M = 50) and the same with M = 0 - and for the WRONG ones a defect would produce: M = 100
    in place of either, and centred.  PRECONDITION, asserted here with the oracle alone (tests/test_cmn_sliding_ref.py runs it
    without a GPU): every wrong option moves every x-vector at least 10 bars away from the right one, so that passing the bar
    tells them apart.  The first 100 frames carry the difference between the minimum windows: the utterances are short."""
    net, line = H.synth_model("v2_xvector")
    n2 = H.nm.Nnet3.from_bytes(net.to_bytes(True))
    n2.apply_nnet_config(line)
    ev = H.xo.GraphEvaluator(n2, np.float32)
    lens = [150, 230, 310, 400]
    utts = [("utt%d" % i, H.features(900 + i, T) + 1.5) for i, T in enumerate(lens)]
    vads = [("utt%d" % i, fe.synthetic_vad(30 + i, T)) for i, T in enumerate(lens)]

    def xvectors(center, M):
        return {k: H.xo.extract_xvector(ev, R.select(R.sliding_cmn(x, ENGINE_W, center, M), v), 10000, 25, True)
                for (k, x), (_, v) in zip(utts, vads)}
    right = {50: xvectors(False, 50), 0: xvectors(False, 0)}
    wrong = {"M=100": xvectors(False, 100), "centred": xvectors(True, 100)}
    for M, ref in right.items():
        for name, w in list(wrong.items()) + [("the other M", right[50 - M])]:
            for k in ref:
                d = H.rel_err(w[k][None], ref[k][None])
                assert d >= 10 * ENGINE_BAR, (M, name, k, d)
    return utts, vads, right


@pytest.mark.parametrize("M", [50, 0])
def test_the_engine_path_with_other_options(tmp_path, M):
    """nnet3-xvector-compute handed the recipes' pipeline string with other options than the recipes': recognised, run on the
    device by the engine's in-flight front-end (FrontEndJob), with THESE options - the minimum window as typed, 0 included (the
    tool the string names takes it so).  Not byte identity with the tools' output: the extractor calibrates on the job's chunks."""
    utts, vads, right = engine_case()
    net, _ = H.synth_model("v2_xvector")
    (tmp_path / "final.raw").write_bytes(net.to_bytes(True))
    kio.write_ark_matrices(str(tmp_path / "feats.ark"), utts, scp_path=str(tmp_path / "feats.scp"))
    kio.write_ark_vectors(str(tmp_path / "vad.ark"), vads, scp_path=str(tmp_path / "vad.scp"))
    pipe = ("ark:apply-cmvn-sliding --norm-vars=false --center=false --cmn-window=%d --min-cmn-window=%d scp:%s/feats.scp ark:- | "
            "select-voiced-frames ark:- scp,s,cs:%s/vad.scp ark:- |" % (ENGINE_W, M, tmp_path, tmp_path))
    r = _run([os.path.join(BIN, "nnet3-xvector-compute"), "--use-gpu=yes", "--min-chunk-size=25", "--chunk-size=10000",
              "--output-node=tdnn6.affine", str(tmp_path / "final.raw"), pipe, "ark,scp:%s/x.ark,%s/x.scp" % (tmp_path, tmp_path)])
    err = r.stderr.decode()
    assert r.returncode == 0, err[-1500:]
    assert ("feature pipeline recognised (apply-cmvn-sliding --norm-vars=false --center=false --cmn-window=%d --min-cmn-window=%d "
            "| select-voiced-frames scp,s,cs:%s/vad.scp): it runs on the device" % (ENGINE_W, M, tmp_path)) in err, err[-1500:]
    assert "Done 4 utterances, failed for 0" in err, err[-1500:]
    got = dict(kio.read_scp(str(tmp_path / "x.scp"), "vector"))
    assert sorted(got) == sorted(right[M])
    for k, ref in right[M].items():
        d = H.rel_err(got[k][None], ref[None])
        assert d < ENGINE_BAR, (M, k, d)
