"""GPU tests of the edge cases of the path: maximum chunk size, multi-chunk utterances, many tiny utterances per tile,
non-finite features (must not leak into neighbours), determinism, compressed feature archives through the CLI."""
import os
import subprocess

import numpy as np
import pytest

import helpers as H
from oracle import kaldi_io as kio

pytestmark = pytest.mark.gpu
BIN = os.path.join(H.ROOT, H.PKG_NAME, "bin")
TOL = 1e-4


@pytest.fixture(scope="module")
def v2():
    P = H.pkg()
    net, line = H.synth_model("v2_xvector")
    model = P.Model(raw=net.to_bytes(True), nnet_config=line)
    n2 = H.nm.Nnet3.from_bytes(net.to_bytes(True))
    n2.apply_nnet_config(line)
    return P, net, line, model, P.Context(model), H.xo.GraphEvaluator(n2, np.float32)


def test_maximum_chunk_size_and_long_utterance(v2):
    # max_chunk_size=10000 (run_xvector_new.sh:83): a 10000-frame chunk is one pooling window; 25000 frames -> 3 chunks
    P, net, line, model, ctx, ev = v2
    x = H.features(4242, 25000)
    out, ok = ctx.extract_utterances(x, [0, 25000], 10000, 25, True)
    assert ok[0]
    ref = H.xo.extract_xvector(ev, x, 10000, 25, True)
    assert H.rel_err(out, ref[None]) < TOL
    one = ctx.forward_batch(x[:10000], [0, 10000])
    assert H.rel_err(one, ev.compute(x[:10000])) < TOL


def test_many_tiny_utterances_share_tiles(v2):
    # 300 utterances of 15..40 frames: up to 16 utterances per 256-row tile, several per 16-row... no: each starts a
    # new 16-row group; checks the per-group masks and per-utterance reductions
    P, net, line, model, ctx, ev = v2
    rng = np.random.default_rng(8)
    lens = [int(t) for t in rng.integers(15, 41, 300)]
    utts = [H.features(2000 + i, T) for i, T in enumerate(lens)]
    feats, offs = H.pack(utts)
    out = ctx.forward_batch(feats, offs)
    idx = list(range(0, 300, 13))
    ref = np.stack([ev.compute(utts[i])[0] for i in idx])
    assert H.rel_err(out[idx], ref) < TOL
    assert np.all(np.isfinite(out))


def test_non_finite_features_stay_in_their_utterance(v2):
    P, net, line, model, ctx, ev = v2
    utts = [H.features(3000 + i, T) for i, T in enumerate([100, 64, 100, 37])]
    clean, offs = H.pack(utts)
    base = ctx.forward_batch(clean, offs)
    bad = [u.copy() for u in utts]
    bad[1][0, 3] = np.nan           # first frame of utterance 1 (adjacent to the last frames of utterance 0)
    bad[1][-1, 0] = np.inf          # and its last frame (adjacent to utterance 2)
    f2, _ = H.pack(bad)
    out = ctx.forward_batch(f2, offs)
    assert not np.all(np.isfinite(out[1]))
    for i in (0, 2, 3):
        assert np.array_equal(out[i], base[i]), i      # neighbours are bit-identical: no cross-utterance arithmetic


def test_contexts_give_their_device_memory_back(v2):
    # the 4-bit residual planes of the default arithmetic were allocated per lane and never freed.  Ten contexts
    # created, run (activation buffers of both lanes, tables, pinned slots) and destroyed must not keep device memory.
    import torch
    P, net, line, model, ctx, ev = v2
    feats, offs = H.pack([H.features(600 + i, 400) for i in range(8)])

    def cycle():
        c = P.Context(model)
        c.forward_batch(feats, offs)
        c.close()

    cycle()                                 # one-time allocations of the runtime (code objects, streams)
    # A leak costs every cycle; the runtime's own pools (and torch's, in a process that ran two hundred tests before this one)
    # grow once in a while: three rounds of ten contexts, and the round that lost least must have lost (almost) nothing.
    # Round 6: the test used to run early in the session; behind the kernel tests ONE round of ten was seen to lose 46 MB that
    # the next rounds did not lose again.
    lost = []
    for _ in range(3):
        torch.cuda.synchronize()
        free0, _ = torch.cuda.mem_get_info()
        for _ in range(10):
            cycle()
        torch.cuda.synchronize()
        free1, _ = torch.cuda.mem_get_info()
        lost.append(free0 - free1)
    assert min(lost) < (8 << 20), lost      # one context of this size holds ~60 MB


def test_repeatability_and_single_utterance_batch(v2):
    P, net, line, model, ctx, ev = v2
    x = H.features(77, 400)
    a = ctx.forward_batch(x, [0, 400])
    b = ctx.forward_batch(x, [0, 400])
    assert np.array_equal(a, b)
    with pytest.raises(P.XvError):
        ctx.forward_batch(x[:0], [0])               # empty batch is an argument error, not a crash


@pytest.mark.parametrize("topology,mode", [("v5_cvector", "fp16mx2"), ("v2_xvector", "auto"), ("v5_cvector", "auto")])
def test_results_do_not_depend_on_what_else_the_gpu_is_doing(topology, mode):
    """The same batch again and again while another stream keeps the CUs and the memory system busy and a second context
    runs the same job from another thread: every result bit-identical to the first.  (Round 4 found a latent race of the
    1.5-pass kernels this way - a wave of the late wave group read the weight scales of a K step three ahead out of a
    three-slot ring when it was held up for a microsecond; alone on the chip the timing never allowed it.  The batch is the
    shape that hit it: 100 chunks, small enough for the per-tile kernel on the c-vector network's layers.  The 1.25-pass
    arithmetic - the 256 x 256 kernel with few tiles per workgroup - runs the same gauntlet.)"""
    import threading
    torch = pytest.importorskip("torch")
    P = H.pkg()
    net, line = H.synth_model(topology, 123)
    model = P.Model(raw=net.to_bytes(True), nnet_config=line)
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(40000)
    feats = torch.randn(100 * 400, 23, generator=g, device=dev) * (8.0 * 0.9 ** torch.arange(23, device=dev))
    offs = np.arange(101, dtype=np.int32) * 400
    stop = []

    def noise():
        st = torch.cuda.Stream()
        a = torch.randn(4096, 4096, device=dev, dtype=torch.float16)
        b = torch.randn(1 << 25, device=dev)
        with torch.cuda.stream(st):
            while not stop:
                for _ in range(4):
                    (a @ a)
                    b.add_(1.0)
                st.synchronize()
    bad = []

    def worker(tag):
        ctx = P.Context(model, device=0, precision=P.PRECISIONS[mode])
        outs = [torch.empty(100, 512, device=dev) for _ in range(3)]
        ref = None
        for it in range(240):
            o = outs[it % 3]
            ctx.forward_batch_device(feats.data_ptr(), offs, o.data_ptr(), 512, None)
            if it % 3 == 0:
                ctx.synchronize()
                r = o.cpu().numpy().copy()
                if ref is None:
                    ref = r
                elif not np.array_equal(ref, r):
                    bad.append((tag, it, float(np.abs(ref - r).max())))
        ctx.synchronize()
    tn = threading.Thread(target=noise)
    tn.start()
    try:
        ts = [threading.Thread(target=worker, args=("t%d" % i,)) for i in range(2)]
        for t in ts:
            t.start()
        for t in ts:
            t.join()
    finally:
        stop.append(1)
        tn.join()
    assert not bad, bad[:5]


def test_batch_that_starts_at_a_large_row_offset(v2):
    """xv_forward_batch with row_offsets[0] > 0 (a window of a larger feature buffer).  The engine stages only the rows of
    the batch and hands the kernels a base shifted DOWN by row_offsets[0] rows, so element 0 of that base lies far below the
    staging buffer: the first-layer kernel's unconditional loads for slots without a source frame must not go there
    (a fault is fatal with XNACK off).  Same bits as the batch at offset 0, in every arithmetic."""
    P, net, line, model, ctx, ev = v2
    utts = [H.features(500 + i, T) for i, T in enumerate((400, 57, 333, 15))]
    feats, offs = H.pack(utts)
    shift = 3_000_000                                   # 276 MB of rows in front: far outside anything mapped nearby
    for c in (ctx, P.Context(model, precision=P.PREC_FP16X3)):
        want = c.forward_batch(feats, offs)
        # rows below row_offsets[0] are never read: pass a base the batch's own rows start 3M rows above
        base = feats.ctypes.data - shift * feats.shape[1] * 4
        out = np.empty_like(want)
        o2 = (np.asarray(offs) + shift).astype(np.int32)
        P._check(P.lib().xv_forward_batch(c._h, base, o2.ctypes.data, len(o2) - 1, out.ctypes.data))
        assert np.array_equal(out, want)


def test_compressed_feature_archive_through_the_cli(tmp_path, v2):
    # steps/make_mfcc.sh writes compress=true archives (make_mfcc.sh:12); the extractor must read CM/CM2 directly
    P, net, line, model, ctx, ev = v2
    (tmp_path / "final.raw").write_bytes(net.to_bytes(True))
    utts = [("c%d" % i, H.features(5000 + i, T)) for i, T in enumerate([300, 45])]
    expect = {}
    with open(tmp_path / "feats.ark", "wb") as f:
        for (k, m), method in zip(utts, ("CM", "CM2")):
            f.write(k.encode() + b" \x00B")
            expect[k] = kio.write_compressed_matrix(f, m, method)      # what a conforming reader reconstructs
    r = subprocess.run([os.path.join(BIN, "nnet3-xvector-compute"), "--min-chunk-size=25", "--chunk-size=10000",
                        "--output-node=tdnn6.affine", str(tmp_path / "final.raw"), "ark:%s/feats.ark" % tmp_path,
                        "ark:%s/x.ark" % tmp_path], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0, r.stderr.decode()
    got = dict(kio.read_ark(str(tmp_path / "x.ark"), "vector"))
    for k, m in expect.items():
        ref = H.xo.extract_xvector(ev, m, 10000, 25, True)
        assert H.rel_err(got[k][None], ref[None]) < TOL, k


@pytest.mark.parametrize("feat_dim,offsets,w1", [
    (5, (-2, -1, 0, 1, 2), 8),        # the tiny net: dp = 8, K = 40 of 128
    (24, (-2, -1, 0, 1, 2), 600),     # dp = 24, K = 120; 600 -> 640 columns: two column groups of the first-layer kernel
    (30, (-2, 0), 72),                # dp = 32, non-unit spacing: the splice address is per K chunk, not a contiguous window
    (30, (-3, 0, 3), 72),             # (64 + 6) x 32 staged floats > 4 per thread: prep_input + the generic GEMM
    (16, (-7, -1, 0, 2, 4, 5, 6, 8), 40),   # eight irregular offsets, K = 128 exactly, span 15
    (40, (-1, 0, 1), 64),             # dp = 40 > 32: not for the first-layer kernel - prep_input + the generic GEMM
    (23, (-15, 0, 15), 64),           # the widest span a model may have (+-15 frames): (64 + 30) x 24 staged floats: generic path
    (16, (-15, 0, 15), 64),           # the same span with 16-float rows fits
])
def test_first_layer_shapes(feat_dim, offsets, w1):
    """The layers that read the network input run tdnn_first_kernel where its layout allows (feature rows of <= 24 floats,
    noff x roundup(dim, 8) <= 128 compact K columns, at most four staged floats per thread and unit) and prep_input + the generic kernel elsewhere:
    every shape against the oracle in the three-pass arithmetic and in the default (fp16mx2 planes + 4-bit residual, or the
    hi-only planes of fp16mx), with chunks in both row regions, and the profile report says which kernel ran."""
    P = H.pkg()
    app = "Append(%s)" % ", ".join("input" if o == 0 else "Offset(input, %d)" % o for o in offsets)
    # wider layers behind the first one so that the 4-bit modes apply to them (multiples of 128 columns of K per source)
    cfg = H.tiny_config(feat_dim=feat_dim, w1=w1, w2=128, pool=128, emb=16)
    old = "Append(Offset(input, -2), Offset(input, -1), input, Offset(input, 1), Offset(input, 2))"
    assert old in cfg
    cfg = cfg.replace(old, app).replace("input-dim=%d output-dim=%d" % (5 * feat_dim, w1), "input-dim=%d output-dim=%d" % (len(offsets) * feat_dim, w1))
    net = H.nm.synthesize(cfg, seed=21)
    line = "output-node name=output input=tdnn6.affine"
    model = P.Model(raw=net.to_bytes(True), nnet_config=line)
    n2 = H.nm.Nnet3.from_bytes(net.to_bytes(True))
    n2.apply_nnet_config(line)
    ev = H.xo.GraphEvaluator(n2, np.float64)
    rng = np.random.default_rng(4)
    lens = [400, 61, 333, 80, 200]
    utts = [(rng.standard_normal((T, feat_dim)) * 3).astype(np.float32) for T in lens]
    feats, offs = H.pack(utts)
    ref = np.stack([ev.compute(u)[0] for u in utts])
    dp = (feat_dim + 7) // 8 * 8
    span = max(offsets) - min(offsets)
    fits = dp <= 24 and len(offsets) * dp <= 128 and span <= 30 and (64 + span) * dp <= 4 * 512   # kernels.h FirstLayerApplicable
    for prec, tol in (("fp16x3", 2e-5), ("default", 1e-4)):
        ctx = P.Context(model, precision=P.PRECISIONS[prec])
        out = ctx.forward_batch(feats, offs)
        errs = [H.rel_err(out[i:i + 1], ref[i:i + 1]) for i in range(len(utts))]
        assert max(errs) < tol, (prec, errs)
        ctx.set_profiling(True)
        ctx.forward_batch(feats, offs)
        labels = " | ".join(l for (l, _, _) in ctx.profile_report())
        assert ("tdnn_first_kernel" in labels) == fits, labels
        assert ("prep_input" in labels) == (not fits), labels
