"""GPU tests of the feature compressor (csrc/compress_kernels.hip) against the fp32 restatement tests/compress_ref.py - for
equality: every operation of the format is one IEEE single-precision rounding on both sides - of the model-free sliding CMN
against the extractor's front-end, and of stage 3 / a compressed stage 1 with the recipes' own command lines."""
import functools
import os
import struct
import subprocess

import numpy as np
import pytest

import compress_ref as C
import helpers as H
from oracle import kaldi_io as kio

pytestmark = pytest.mark.gpu
BIN = os.path.join(H.ROOT, H.PKG_NAME, "bin")

# each row count is the smallest at which its branch can go wrong: 1 / 3 / 4 the short-column header, 5 the first with
# quartiles, 8 | 9 the automatic method's flip, 10 where 3 q != (3 rows) / 4, 64 | 65 and 257 around the 44-row step of the
# selection and the 128-row block of the encode pass, 1000 several blocks, 4099 a prime with more than one 16384-element chunk
ROWS = [1, 3, 4, 5, 8, 9, 10, 64, 65, 257, 1000, 4099]
CASES = ["gaussian", "constant_column", "constant_0", "constant_-3.5", "ties", "signed_zeros", "wide_span", "denormals"]


def case_matrix(case, rows, cols, seed):
    rng = np.random.default_rng(seed)
    m = (rng.standard_normal((rows, cols)) * np.linspace(0.5, 20.0, cols)).astype(np.float32)
    c = min(3, cols - 1)
    if case == "constant_column":
        m[:, c] = 2.5
    elif case == "constant_0":
        m[:] = 0.0
    elif case == "constant_-3.5":
        m[:] = -3.5
    elif case == "ties":             # one value repeated across s[q] and another across s[3 q], in shuffled order
        q = rows // 4
        s = np.sort(m[:, c])
        s[max(0, q - 2):q + 3] = s[q] if rows else 0
        s[max(0, 3 * q - 2):3 * q + 3] = s[min(3 * q, rows - 1)]
        m[:, c] = rng.permutation(s)
    elif case == "signed_zeros":
        m[:, c] = np.where(rng.random(rows) < 0.5, np.float32(0.0), np.float32(-0.0))
        m[m[:, 0] < 0, 0] = -0.0
    elif case == "wide_span":
        m[:, c] = (10.0 ** rng.uniform(-30, 30, rows)).astype(np.float32)
        m[0, c], m[-1, c] = 1e-30, 1e30
    elif case == "denormals":
        m[:] = (rng.integers(-2000, 2000, size=(rows, cols)) * np.float64(2.0 ** -149)).astype(np.float32)
    return m


@functools.lru_cache(maxsize=None)
def batch(cols):
    rows = ROWS if cols == 23 else [257]
    return tuple((case, r, case_matrix(case, r, cols, 1000 * i + r)) for i, case in enumerate(CASES) for r in rows)


@functools.lru_cache(maxsize=None)
def reference(cols, method):
    return tuple(C.compress(m, method) for _, _, m in batch(cols))


@pytest.mark.parametrize("cols", [23, 1, 24, 130])
@pytest.mark.parametrize("method", [1, 2, 3, 5])
def test_bytes_equal_the_fp32_restatement(method, cols):
    """One ragged launch per method and column count; every object byte for byte."""
    P = H.pkg()
    mats = [m for _, _, m in batch(cols)]
    got, flags = P.compress(mats, method=method, return_flags=True)
    assert not any(flags)
    wrong = []
    for (case, rows, m), (fmt, want), obj in zip(batch(cols), reference(cols, method), got):
        assert P.compressed_size(rows, cols, method) == (len(want), fmt)
        if obj != want:
            first = next(i for i, (a, b) in enumerate(zip(obj, want)) if a != b)
            wrong.append((case, rows, fmt, first, len(want)))
    assert not wrong, wrong
    if method == 1:
        fmts = {rows: fmt for (_, rows, _), (fmt, _) in zip(batch(cols), reference(cols, method))}
        if cols == 23:
            assert fmts[8] == "CM2" and fmts[9] == "CM"
            assert P.compressed_size(8, cols, 1)[1] == "CM2" and P.compressed_size(9, cols, 1)[1] == "CM"


def test_a_matrix_compresses_the_same_alone_and_in_a_batch():
    P = H.pkg()
    rng = np.random.default_rng(7)
    mats = [rng.standard_normal((r, 23)).astype(np.float32) * (1 + i) for i, r in enumerate([300, 0, 77, 9, 1000, 0, 513])]
    for method in (1, 2, 3, 5):
        together = P.compress(mats, method=method)
        for i in (0, 2, 4, 6):           # first, middle (between empty neighbours), last
            assert P.compress([mats[i]], method=method)[0] == together[i], (method, i)
        assert together[1] == together[5] == b"\0" * 16


def test_nonfinite_and_empty():
    P = H.pkg()
    rng = np.random.default_rng(8)
    clean = [rng.standard_normal((r, 23)).astype(np.float32) for r in (40, 9, 130, 700, 12)]
    mats = [m.copy() for m in clean]
    mats[1][8, 22] = np.nan
    mats[2][129, 0] = np.inf
    mats[3][350, 7] = -np.inf
    mats.insert(2, np.zeros((0, 23), np.float32))
    clean.insert(2, np.zeros((0, 23), np.float32))
    for method in (1, 3):
        objs, flags = P.compress(mats, method=method, return_flags=True)
        assert flags == [False, True, False, True, True, False]
        want = P.compress(clean, method=method)
        for i in (0, 2, 5):
            assert objs[i] == want[i] == C.compress(clean[i], method)[1]
        assert objs[2] == struct.pack("<ffii", 0.0, 0.0, 0, 0)
    assert P.compress([np.zeros((5, 0), np.float32), np.zeros((0, 0), np.float32)]) == [b"\0" * 16] * 2
    for bad in (0, 4, 6, 7):
        with pytest.raises(P.XvError):
            P.compress(clean, method=bad)


@pytest.mark.parametrize("center", [True, False])
def test_cmvn_sliding_equals_the_front_end(center):
    P = H.pkg()
    net, line = H.synth_model("v2_xvector")
    ctx = P.Context(P.Model(raw=net.to_bytes(True), nnet_config=line))
    utts = [H.features(90 + i, T) + 3.0 for i, T in enumerate([299, 700, 1])]      # shorter than the window, longer, one row
    raw, offs = H.pack(utts)
    want, want_off = ctx.frontend(raw, offs, None, cmn_window=300, center=center)
    got = P.cmvn_sliding(utts, cmn_window=300, min_cmn_window=100, center=center)
    assert np.array_equal(want_off, offs)
    assert np.concatenate(got).tobytes() == want.tobytes()
    assert not np.array_equal(np.concatenate(got), raw)


def _run(args, **kw):
    return subprocess.run(args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300, **kw)


def read_compressed_scp(path):
    """{key: (token, object bytes)} of a script file whose entries point at compressed objects; resolves "file:offset"."""
    out = {}
    for line in open(path).read().splitlines():
        key, rx = line.split(None, 1)
        ark, off = rx.rsplit(":", 1)
        data = open(ark, "rb").read()
        off = int(off)
        assert data[off:off + 2] == b"\0B" and data[off - len(key) - 1:off] == key.encode() + b" ", line
        token = data[off + 2:data.index(b" ", off + 2)].decode()
        start = off + 2 + len(token) + 1
        _, _, rows, cols = struct.unpack("<ffii", data[start:start + 16])
        size = {"CM": 16 + cols * 8 + rows * cols, "CM2": 16 + 2 * rows * cols, "CM3": 16 + rows * cols}[token]
        out[key] = (token, data[start:start + size])
    return out


def test_stage3_runs_with_the_recipes_argv(tmp_path):
    """local/nnet3/xvector/prepare_feats_for_egs.sh:66-71 with its own argv - three processes, two of them with the device - and
    then the pipeline without selection of sid/nnet3_cvector/cvector/prepare_feats.sh:88-92."""
    from oracle import frontend as fe
    P = H.pkg()
    d = tmp_path
    lens = [500, 120, 333, 64, 401]
    utts = [("utt%d" % i, H.features(700 + i, T) + 1.5) for i, T in enumerate(lens)]
    vads = [("utt%d" % i, fe.synthetic_vad(40 + i, T)) for i, T in enumerate(lens)]
    del vads[3]                                                        # utt3 has no VAD decision
    kio.write_ark_matrices(str(d / "feats.ark"), utts, scp_path=str(d / "feats.scp"))
    kio.write_ark_vectors(str(d / "vad.ark"), vads, scp_path=str(d / "vad.scp"))
    env = dict(os.environ, PATH=BIN + os.pathsep + os.environ.get("PATH", ""), XVEC_COMPRESS="1")
    cmd = ("apply-cmvn-sliding --norm-vars=false --center=true --cmn-window=300 scp:%s/feats.scp ark:- | "
           "select-voiced-frames ark:- scp,s,cs:%s/vad.scp ark:- | "
           "copy-feats --compress=true --write-num-frames=ark,t:%s/utt2num_frames.1 ark:- ark,scp:%s/xvector_feats.1.ark,%s/xvector_feats.1.scp"
           % ((d,) * 5))
    r = _run(["bash", "-c", "set -o pipefail; " + cmd], env=env)
    err = r.stderr.decode()
    assert r.returncode == 0, err
    assert "No VAD input found for utterance utt3" in err and "processed 4 utterances, 1 had errors" in err, err
    assert "--compress=true honoured" in err and "compressed 4 matrices" in err and "Copied 4 feature matrices" in err, err
    cmn = dict(zip([k for k, _ in utts], P.cmvn_sliding([m for _, m in utts], cmn_window=300, center=True)))
    voiced = {k: cmn[k][v != 0] for k, v in vads}
    got = read_compressed_scp(str(d / "xvector_feats.1.scp"))
    assert list(got) == ["utt0", "utt1", "utt2", "utt4"]
    n2f = dict(l.split() for l in open(d / "utt2num_frames.1").read().splitlines())
    assert n2f == {k: str(m.shape[0]) for k, m in voiced.items()}
    for k, (token, obj) in got.items():
        assert (token, obj) == C.compress(voiced[k], 1), k
        assert token == "CM"
    back = dict(kio.read_scp(str(d / "xvector_feats.1.scp"), "matrix"))      # and an independent reader takes them
    assert all(back[k].shape == voiced[k].shape for k in voiced)
    # v3-v5 without selection
    cmd = ("apply-cmvn-sliding --norm-vars=false --center=true --cmn-window=300 scp:%s/feats.scp ark:- | "
           "copy-feats --compress=true --write-num-frames=ark,t:%s/utt2num_frames.2 ark:- ark,scp:%s/xvector_feats.2.ark,%s/xvector_feats.2.scp"
           % ((d,) * 4))
    r = _run(["bash", "-c", "set -o pipefail; " + cmd], env=env)
    assert r.returncode == 0, r.stderr.decode()
    got = read_compressed_scp(str(d / "xvector_feats.2.scp"))
    assert list(got) == [k for k, _ in utts]
    for k, (token, obj) in got.items():
        assert (token, obj) == C.compress(cmn[k], 1), k


def test_stage1_compressed_feeds_the_device_expansion(tmp_path):
    """steps/make_mfcc.sh:125-129 under XVEC_COMPRESS=1 writes CM objects; extract_xvectors_new.sh:79's pipeline string on them
    takes the extractor's compressed path (the bytes go up as they are and are expanded on the device) and gives the vectors of
    the same job on the floats those objects decode to."""
    from test_gpu_mfcc import speechlike, write_wav
    d = tmp_path
    (d / "mfcc.conf").write_text("--sample-frequency=8000\n--frame-length=25\n--low-freq=20\n--high-freq=3700\n--num-ceps=23\n--snip-edges=false\n")
    lens = {"spk1-a": 40000, "spk1-b": 24000, "spk2-a": 56000}
    for i, (k, n) in enumerate(lens.items()):
        write_wav(str(d / (k + ".wav")), speechlike(800 + i, n))
    (d / "wav.scp").write_text("".join("%s %s/%s.wav\n" % (k, d, k) for k in lens))
    env = dict(os.environ, PATH=BIN + os.pathsep + os.environ.get("PATH", ""))
    cmd = ("compute-mfcc-feats --verbose=2 --config=%s/mfcc.conf scp,p:%s/wav.scp ark:- | "
           "copy-feats --write-num-frames=ark,t:%s/utt2num_frames.1 --compress=true ark:- ark,scp:%s/raw_mfcc.1.ark,%s/feats.scp" % ((d,) * 5))
    r = _run(["bash", "-c", "set -o pipefail; " + cmd], env=dict(env, XVEC_COMPRESS="1"))
    assert r.returncode == 0 and b"compressed 3 matrices" in r.stderr, r.stderr.decode()
    stored = read_compressed_scp(str(d / "feats.scp"))
    assert [t for t, _ in stored.values()] == ["CM"] * 3
    # the floats the objects decode to, as an uncompressed archive (the tool's reader, no switch, no device)
    r = _run([os.path.join(BIN, "copy-feats"), "scp:%s/feats.scp" % d, "ark,scp:%s/decoded.ark,%s/decoded.scp" % (d, d)], env=env)
    assert r.returncode == 0, r.stderr.decode()
    r = _run([os.path.join(BIN, "compute-vad"), "--vad-energy-threshold=5.5", "--vad-energy-mean-scale=0.5", "scp:%s/decoded.scp" % d,
              "ark,scp:%s/vad.ark,%s/vad.scp" % (d, d)], env=env)
    assert r.returncode == 0, r.stderr.decode()
    net, line = H.synth_model("v2_xvector")
    (d / "final.raw").write_bytes(net.to_bytes(True))
    (d / "extract.config").write_text(line + "\n")
    outs = {}
    for tag in ("feats", "decoded"):
        feat = ("ark:apply-cmvn-sliding --norm-vars=false --center=true --cmn-window=300 scp:%s/%s.scp ark:- | "
                "select-voiced-frames ark:- scp,s,cs:%s/vad.scp ark:- |" % (d, tag, d))
        r = _run([os.path.join(BIN, "nnet3-xvector-compute"), "--use-gpu=no", "--min-chunk-size=25", "--chunk-size=10000",
                  "%s/nnet3-copy --nnet-config=%s/extract.config %s/final.raw - |" % (BIN, d, d), feat,
                  "ark,scp:%s/x_%s.ark,%s/x_%s.scp" % (d, tag, d, tag)], env=dict(env, XVEC_TIMING="1"))        # the timing lines name the path taken
        assert r.returncode == 0, r.stderr.decode()
        outs[tag] = (dict(kio.read_scp("%s/x_%s.scp" % (d, tag), "vector")), r.stderr.decode())
    assert "utterances went to the device compressed" in outs["feats"][1], outs["feats"][1][-1500:]
    assert "went to the device compressed" not in outs["decoded"][1]
    assert list(outs["feats"][0]) == list(lens)
    for k in lens:
        assert outs["feats"][0][k].tobytes() == outs["decoded"][0][k].tobytes(), k
