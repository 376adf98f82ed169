"""Host side of per-speaker CMVN: xv_cmvn_norm against the numpy restatement, nnet3-am-copy, the refusals.  No GPU."""
import os
import subprocess

import numpy as np
import pytest

import cmvn_ref as R
import helpers as H

P = H.pkg()
BIN = os.path.join(H.ROOT, H.PKG_NAME, "bin")


def _run(tool, *args, **kw):
    return subprocess.run([os.path.join(BIN, tool)] + list(args), stdout=subprocess.PIPE, stderr=subprocess.PIPE, **kw)


def _stats_cases():
    rng = np.random.default_rng(5)
    out = []
    for rows, cols, loc, sd in ((1, 1, 0.5, 1.0), (3, 5, 50.0, 1.0), (1000, 23, -7.0, 3.0), (77, 40, 1e3, 1e-2), (9, 65, 0.0, 100.0)):
        x = rng.normal(loc, sd, size=(rows, cols)).astype(np.float32)
        out.append(R.stats(x))
    # two utterances of one speaker added; a constant column (variance floored); a count that is not an integer
    out.append(out[1] + R.stats(rng.normal(49, 2, size=(11, 5)).astype(np.float32)))
    st = R.stats(np.full((6, 3), 1.25, np.float32))
    out.append(st)
    st = out[2].copy()
    st[0, -1] = 999.5
    out.append(st)
    return out


@pytest.mark.parametrize("norm_means,norm_vars,reverse", [(True, False, False), (True, True, False), (True, False, True), (True, True, True),
                                                          (False, False, False)])
def test_norm_equals_the_restatement_bit_for_bit(norm_means, norm_vars, reverse):
    for st in _stats_cases():
        cols = st.shape[1] - 1
        for skip in ((), (0,), tuple(range(0, cols, 2))):
            got, gf = P.cmvn_norm(st, norm_means, norm_vars, reverse, skip, return_floored=True)
            want, wf = R.cmvn_norm(st, norm_means, norm_vars, reverse, skip, return_floored=True)
            assert got.dtype == np.float32 and got.shape == (2, cols)
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (st.shape, skip)
            assert gf == wf


def test_norm_refusals():
    st = _stats_cases()[1]
    with pytest.raises(P.XvError) as e:
        P.cmvn_norm(st, norm_means=False, norm_vars=True)
    assert e.value.status == P.XV_ERR_ARG and "cannot normalize the variance but not the mean" in str(e.value)
    empty = st.copy()
    empty[0, -1] = 0.0
    with pytest.raises(P.XvError) as e:
        P.cmvn_norm(empty)
    assert "Insufficient stats for cepstral mean and variance normalization: count = 0" in str(e.value)
    with pytest.raises(P.XvError):
        P.cmvn_norm(st, skip_dims=(5,))
    with pytest.raises(P.XvError):
        P.cmvn_norm(np.zeros((3, 4)))


# ---- the scripts' feature strings still run as commands -------------------------------------------------------------------------
S = "/data/split4/2"
SCRIPT_FORMS = [
    # extract_bn.sh:59 / make_bottleneck_features_new.sh:91
    "ark,s,cs:apply-cmvn  --utt2spk=ark:%s/utt2spk scp:%s/cmvn.scp scp:%s/feats.scp ark:- |" % (S, S, S),
    # extract_am_embedding.sh:67
    "ark:apply-cmvn --norm-vars=false --utt2spk=ark:%s/utt2spk scp:%s/cmvn.scp scp:%s/feats.scp ark:- |" % (S, S, S),
    # extract_cvectors_with_am.sh:94 / extract_output_with_am.sh:89: quoted, with the selection stage; and the same bare
    "ark:apply-cmvn --norm-means=true --utt2spk='ark:%s/utt2spk' scp:%s/cmvn.scp scp:%s/feats.scp ark:- | "
    "select-voiced-frames ark:- scp,s,cs:%s/vad.scp ark:- |" % (S, S, S, S),
    "ark:apply-cmvn --utt2spk=ark:%s/utt2spk scp:%s/cmvn.scp scp:%s/feats.scp ark:- | select-voiced-frames ark:- scp,s,cs:%s/vad.scp ark:- |"
    % (S, S, S, S),
]


def test_the_sliding_recogniser_does_not_take_the_per_speaker_pipeline():
    """A guard, not a test of the new tools (it holds on the code before them too): the extractor's fused front-end is sliding CMN,
    so a per-speaker apply-cmvn pipeline must not be taken for it; it is run as written (tests/test_gpu_cmvn_pipeline.py)."""
    for text in SCRIPT_FORMS:
        assert P.recognize_feature_pipeline(text) is None, text
    sliding = "ark:apply-cmvn-sliding --norm-vars=false --center=true --cmn-window=300 scp:f.scp ark:- | select-voiced-frames ark:- scp,s,cs:v.scp ark:- |"
    assert P.recognize_feature_pipeline(sliding) is not None


# ---- nnet3-am-copy ----------------------------------------------------------------------------------------------------------------
def _mdl(raw, binary):
    if binary:
        assert raw[:2] == b"\x00B"
        junk = bytes(range(256)) * 3 + b"<Triples> \x04\x07\x00\x00\x00 </Triples> <LogProbs> FV \x04\x02\x00\x00\x00" + b"\x00" * 8
        return (b"\x00B<TransitionModel> " + junk + b"</TransitionModel> " + raw[2:] +
                b"<LeftContext> \x04\x0d\x00\x00\x00<RightContext> \x04\x07\x00\x00\x00<Priors> FV \x04\x00\x00\x00\x00")
    junk = b"<Topology>\n<TopologyEntry>\n<ForPhones>\n1 2 3\n</ForPhones>\n</TopologyEntry>\n</Topology>\n<Triples> 2\n1 0 0\n</Triples>\n"
    return b"<TransitionModel> \n" + junk + b"</TransitionModel> \n" + raw + b"<LeftContext> 13 <RightContext> 7 <Priors>  [ ]\n"


@pytest.mark.parametrize("binary", [True, False])
def test_am_copy_writes_what_nnet3_copy_writes_from_the_bare_network(tmp_path, binary):
    net = H.nm.synthesize([H.config_text("am")], seed=3)
    raw = net.to_bytes(binary)
    (tmp_path / "final.raw").write_bytes(raw)
    (tmp_path / "final.mdl").write_bytes(_mdl(raw, binary))
    r = _run("nnet3-copy", str(tmp_path / "final.raw"), str(tmp_path / "want.raw"))
    assert r.returncode == 0, r.stderr
    r = _run("nnet3-am-copy", "--raw=true", str(tmp_path / "final.mdl"), str(tmp_path / "got.raw"))
    assert r.returncode == 0, r.stderr
    assert b"LOG (nnet3-am-copy" in r.stderr
    assert (tmp_path / "got.raw").read_bytes() == (tmp_path / "want.raw").read_bytes()
    # the scripts' own pipe (extract_bn.sh:57), as a model rxfilename
    (tmp_path / "extract.config").write_text("output-node name=output input=tdnn5.batchnorm\n")
    rx = "%s/nnet3-am-copy --raw=true %s/final.mdl - | %s/nnet3-copy --nnet-config=%s/extract.config - - |" % (BIN, tmp_path, BIN, tmp_path)
    want = P.Model(raw=raw, nnet_config="output-node name=output input=tdnn5.batchnorm").pack()
    assert P.Model(rxfilename=rx).pack() == want


def test_am_copy_refuses_everything_but_raw_true(tmp_path):
    net = H.nm.synthesize([H.config_text("am")], seed=3)
    raw = net.to_bytes(True)
    (tmp_path / "final.mdl").write_bytes(_mdl(raw, True))
    (tmp_path / "final.raw").write_bytes(raw)
    mdl, out = str(tmp_path / "final.mdl"), str(tmp_path / "o.raw")
    for args in (["--raw=false"], [], ["--raw=true", "--edits=x"], ["--raw=true", "--learning-rate=0.1"], ["--raw=true", "--set-raw-nnet=a.raw"],
                 ["--raw=true", "--nnet-config=x"], ["--raw="]):
        r = _run("nnet3-am-copy", *args, mdl, out)
        assert r.returncode != 0, args
        assert not os.path.exists(out), args
    # a bare network is not an acoustic model
    r = _run("nnet3-am-copy", "--raw=true", str(tmp_path / "final.raw"), out)
    assert r.returncode != 0 and b"<TransitionModel>" in r.stderr
    # a bare --raw is "true", as Kaldi reads a boolean option without a value
    r = _run("nnet3-am-copy", "--raw", mdl, out)
    assert r.returncode == 0, r.stderr
    os.remove(out)
    # the name is matched whole: a copy under another name that merely contains "am-copy" is nnet3-copy
    other = str(tmp_path / "my-am-copy")
    os.symlink(os.path.join(BIN, "nnet3-am-copy"), other)
    r = subprocess.run([other, "--raw=true", mdl, out], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 1 and b"nnet3-copy" in r.stderr and b"not supported" in r.stderr
    # ... and nnet3-copy has not learnt --raw
    r = _run("nnet3-copy", "--raw=true", str(tmp_path / "final.raw"), out)
    assert r.returncode == 1 and b"not supported" in r.stderr


def test_the_tools_refuse_what_is_not_built(tmp_path):
    r = _run("compute-cmvn-stats", "--weights=ark:w.ark", "scp:f.scp", "ark:o.ark")
    assert r.returncode == 255 and b"ERROR (compute-cmvn-stats" in r.stderr and b"--weights" in r.stderr
    r = _run("apply-cmvn", "--norm-means=false", "--norm-vars=true", "s", "scp:f.scp", "ark:o.ark")
    assert r.returncode == 255 and b"You cannot normalize the variance but not the mean." in r.stderr
    r = _run("apply-cmvn", "--skip-dims=1:x", "s", "scp:f.scp", "ark:o.ark")
    assert r.returncode == 255 and b"skip-dims" in r.stderr
    for tool, rest in (("compute-cmvn-stats", ["scp:f.scp", "ark:o.ark"]), ("apply-cmvn", ["s", "scp:f.scp", "ark:o.ark"])):
        r = _run(tool, "--device=gpu0", *rest)   # not a number: refused, not read as device 0
        assert r.returncode == 255 and b"device" in r.stderr, r.stderr
    for tool, n in (("compute-cmvn-stats", 1), ("apply-cmvn", 2)):
        r = _run(tool, *["a"] * n)
        assert r.returncode == 1 and b"Usage: " + tool.encode() in r.stderr
        r = _run(tool, "--help")
        assert r.returncode == 0 and b"Usage: " + tool.encode() in r.stderr
