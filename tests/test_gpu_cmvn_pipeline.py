"""The bottleneck path of the recipes, end to end with the scripts' own strings: steps/compute_cmvn_stats.sh:104, then the
`nnet3-compute --use-gpu=no "$raw_nnet" "$feats" ark:- | copy-feats --compress=true ...` of sid/nnet3_cvector/am/extract_bn.sh:57-69,
where $raw_nnet is the nnet3-am-copy | nnet3-copy model pipe and $feats the per-speaker apply-cmvn rspecifier."""
import os
import subprocess

import numpy as np
import pytest

import cmvn_ref as R
import helpers as H
from oracle import kaldi_io as kio

pytestmark = pytest.mark.gpu
BIN = os.path.join(H.ROOT, H.PKG_NAME, "bin")
TOL = 1e-4   # nnet3-compute against the fp32 oracle: the tolerance tests/test_gpu_cli.py holds the same tool and network to


def _sh(line, env_extra=None):
    # the scripts name the tools bare: they are found on PATH, as under run.pl; XVEC_COMPRESS=1 is path.sh's switch that lets
    # copy-feats honour --compress=true
    env = dict(os.environ, PATH=BIN + os.pathsep + os.environ.get("PATH", ""), XVEC_COMPRESS="1")
    env.update(env_extra or {})
    return subprocess.run(["/bin/sh", "-c", line], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env, timeout=300)


def test_extract_bn_runs_with_the_recipes_argv(tmp_path):
    """The per-speaker pipeline is run as the commands it names (no fused form of it is built), so the check is: the scripts' one
    line gives, byte for byte, what the same tools give one at a time through files; and the uncompressed network output agrees with the fp32 oracle fed the restatement's normalised
    features (computed from the statistics the tool itself wrote)."""
    d = tmp_path
    srcdir, sdata, dir_ = d / "am", d / "split1" / "1", d / "bnf"
    for p in (srcdir, sdata, dir_):
        p.mkdir(parents=True)
    net = H.nm.synthesize([H.config_text("am")], seed=21, head_stddev=1.0)
    raw = net.to_bytes(True)
    (srcdir / "final.mdl").write_bytes(b"\x00B<TransitionModel> " + bytes(range(256)) + b"</TransitionModel> " + raw[2:] +
                                       b"<LeftContext> \x04\x0d\x00\x00\x00<RightContext> \x04\x07\x00\x00\x00<Priors> FV \x04\x00\x00\x00\x00")
    spk2utt = {"spkA": ["spkA-u1", "spkA-u2"], "spkB": ["spkB-u1"], "spkC": ["spkC-u1", "spkC-u2"]}
    lens = {"spkA-u1": 120, "spkA-u2": 7, "spkB-u1": 333, "spkC-u1": 61, "spkC-u2": 258}
    utts = [(k, H.features(900 + i, lens[k]) + np.float32(3.0 * (i % 3))) for i, k in enumerate(sorted(lens))]
    kio.write_ark_matrices(str(sdata / "raw_mfcc.ark"), utts, scp_path=str(sdata / "feats.scp"), compressed="CM")
    (sdata / "spk2utt").write_text("".join("%s %s\n" % (s, " ".join(us)) for s, us in spk2utt.items()))
    (sdata / "utt2spk").write_text("".join("%s %s\n" % (u, s) for s, us in sorted(spk2utt.items()) for u in us))
    (dir_ / "extract.config").write_text("output-node name=output input=tdnn5.batchnorm\n")

    # steps/compute_cmvn_stats.sh:104
    r = _sh("compute-cmvn-stats --spk2utt=ark:%s/spk2utt scp:%s/feats.scp ark,scp:%s/cmvn_1.ark,%s/cmvn.scp" % (sdata, sdata, sdata, sdata))
    assert r.returncode == 0, r.stderr
    assert "Done accumulating CMVN stats for 5 utterances; 0 had errors." in r.stderr

    # extract_bn.sh:57-69
    raw_nnet = "nnet3-am-copy --raw=true %s/final.mdl - | nnet3-copy --nnet-config=%s/extract.config - - |" % (srcdir, dir_)
    feats = "ark,s,cs:apply-cmvn  --utt2spk=ark:%s/utt2spk scp:%s/cmvn.scp scp:%s/feats.scp ark:- |" % (sdata, sdata, sdata)
    line = 'nnet3-compute --use-gpu=no "%s" "%s" ark:- | copy-feats --compress=true ark:- ark,scp:%s/raw_bnfeat_%%s.1.ark,%s/raw_bnfeat_%%s.1.scp' \
        % (raw_nnet, feats, dir_, dir_)
    r = _sh(line % ("a", "a"))
    assert r.returncode == 0, r.stderr
    assert "Applied cepstral mean normalization to 5 utterances, errors on 0" in r.stderr
    assert "Done 5 utterances, failed for 0" in r.stderr
    assert "--compress=true honoured" in r.stderr and "compressed 5 matrices" in r.stderr and "Copied 5 feature matrices" in r.stderr
    outs = {"a": (dir_ / "raw_bnfeat_a.1.ark").read_bytes()}
    assert [l.split()[0] for l in open(dir_ / "raw_bnfeat_a.1.scp")] == sorted(lens)

    # the same tools one at a time, through files
    for step in ("nnet3-am-copy --raw=true %s/final.mdl %s/am.raw" % (srcdir, d),
                 "nnet3-copy --nnet-config=%s/extract.config %s/am.raw %s/bn.raw" % (dir_, d, d),
                 "apply-cmvn --utt2spk=ark:%s/utt2spk scp:%s/cmvn.scp scp:%s/feats.scp ark:%s/normed.ark" % (sdata, sdata, sdata, d),
                 "nnet3-compute --use-gpu=no %s/bn.raw ark:%s/normed.ark ark:%s/bn_float.ark" % (d, d, d),
                 "copy-feats --compress=true ark:%s/bn_float.ark ark:%s/bn_cm.ark" % (d, d)):
        r = _sh(step)
        assert r.returncode == 0, (step, r.stderr)
    assert outs["a"] == (d / "bn_cm.ark").read_bytes()

    # the numbers: the oracle on the restatement's features
    r = _sh("copy-feats scp:%s/feats.scp ark:%s/expanded.ark" % (sdata, d))
    assert r.returncode == 0, r.stderr
    stored = dict(kio.read_ark(str(d / "expanded.ark")))
    stats = R.read_double_matrices(str(sdata / "cmvn_1.ark"))
    utt2spk = {u: s for s, us in spk2utt.items() for u in us}
    n2 = H.nm.Nnet3.from_bytes(raw)
    n2.apply_nnet_config("output-node name=output input=tdnn5.batchnorm")
    ev = H.xo.GraphEvaluator(n2, np.float32)
    got = dict(kio.read_ark(str(d / "bn_float.ark")))
    assert sorted(got) == sorted(lens)
    for k in sorted(lens):
        x = R.apply(stored[k], R.cmvn_norm(stats[utt2spk[k]]))
        ref = H.xo.compute_all_frames(ev, x)
        assert got[k].shape == ref.shape == (lens[k], 128)
        err = H.rel_err(got[k], ref)
        print("%s: rel err %.3g" % (k, err))
        assert err < TOL, k


def test_the_select_voiced_frames_form_runs_through_nnet3_xvector_compute(tmp_path):
    """sid/nnet3_cvector/cvector/extract_cvectors_with_am.sh:94 / extract_output_with_am.sh:89: the per-speaker pipeline with the
    selection stage, as the feature rspecifier of nnet3-xvector-compute, with the quoted --utt2spk the scripts write and bare.
    It is run as the commands it names, so both give, byte for byte, the vectors of the same tools run one at a time through
    files, with the same utterances left out; and the frames that reach the extractor are the restatement's, bit for bit."""
    from oracle import frontend as fe
    d = tmp_path
    spk2utt = {"spkA": ["spkA-u1", "spkA-u2"], "spkB": ["spkB-u1"], "spkC": ["spkC-u1"]}
    lens = {"spkA-u1": 310, "spkA-u2": 127, "spkB-u1": 256, "spkC-u1": 90}
    utts = [(k, H.features(950 + i, lens[k]) + np.float32(2.0 * i)) for i, k in enumerate(sorted(lens))]
    vads = [(k, fe.synthetic_vad(60 + i, lens[k])) for i, k in enumerate(sorted(lens))]
    del vads[3]                                                        # spkC-u1 has no VAD decision
    kio.write_ark_matrices(str(d / "raw_mfcc.ark"), utts, scp_path=str(d / "feats.scp"), compressed="CM")
    kio.write_ark_vectors(str(d / "vad.ark"), vads, scp_path=str(d / "vad.scp"))
    (d / "spk2utt").write_text("".join("%s %s\n" % (s, " ".join(us)) for s, us in spk2utt.items()))
    (d / "utt2spk").write_text("".join("%s %s\n" % (u, s) for s, us in sorted(spk2utt.items()) for u in us))
    net, line = H.synth_model("v2_xvector")
    (d / "final.raw").write_bytes(net.to_bytes(True))
    (d / "extract.config").write_text(line + "\n")
    r = _sh("compute-cmvn-stats --spk2utt=ark:%s/spk2utt scp:%s/feats.scp ark,scp:%s/cmvn_1.ark,%s/cmvn.scp" % (d, d, d, d))
    assert r.returncode == 0, r.stderr

    nnet = "nnet3-copy --nnet-config=%s/extract.config %s/final.raw - |" % (d, d)
    compute = 'nnet3-xvector-compute --use-gpu=no --min-chunk-size=25 --chunk-size=10000 "%s" "%s" ark,scp:%s/x_%s.ark,%s/x_%s.scp'
    kept = [k for k, _ in vads]
    outs = {}
    for tag, utt2spk_opt in (("quoted", "--utt2spk='ark:%s/utt2spk'" % d), ("bare", "--utt2spk=ark:%s/utt2spk" % d)):
        feat_am = ("ark:apply-cmvn --norm-vars=false %s scp:%s/cmvn.scp scp:%s/feats.scp ark:- | "
                   "select-voiced-frames ark:- scp,s,cs:%s/vad.scp ark:- |" % (utt2spk_opt, d, d, d))
        r = _sh(compute % (nnet, feat_am, d, tag, d, tag))
        assert r.returncode == 0, r.stderr
        assert "Applied cepstral mean normalization to 4 utterances, errors on 0" in r.stderr
        assert "No VAD input found for utterance spkC-u1" in r.stderr and "processed 3 utterances, 1 had errors" in r.stderr
        assert [l.split()[0] for l in open(d / ("x_%s.scp" % tag))] == kept
        outs[tag] = (d / ("x_%s.ark" % tag)).read_bytes()

    # the same tools one at a time, through files
    for step in ("apply-cmvn --norm-vars=false --utt2spk=ark:%s/utt2spk scp:%s/cmvn.scp scp:%s/feats.scp ark:%s/normed.ark" % (d, d, d, d),
                 "select-voiced-frames ark:%s/normed.ark scp,s,cs:%s/vad.scp ark:%s/voiced.ark" % (d, d, d),
                 "nnet3-copy --nnet-config=%s/extract.config %s/final.raw %s/x.raw" % (d, d, d),
                 "nnet3-xvector-compute --use-gpu=no --min-chunk-size=25 --chunk-size=10000 %s/x.raw ark:%s/voiced.ark ark:%s/x_single.ark" % (d, d, d),
                 "copy-feats scp:%s/feats.scp ark:%s/expanded.ark" % (d, d)):
        r = _sh(step)
        assert r.returncode == 0, (step, r.stderr)
    single = (d / "x_single.ark").read_bytes()
    assert len(single) > 0 and outs["quoted"] == single and outs["bare"] == single

    # what reached the extractor: the restatement's normalised frames, the voiced ones
    stored = dict(kio.read_ark(str(d / "expanded.ark")))
    stats = R.read_double_matrices(str(d / "cmvn_1.ark"))
    utt2spk = {u: s for s, us in spk2utt.items() for u in us}
    voiced = dict(kio.read_ark(str(d / "voiced.ark")))
    assert list(voiced) == kept
    for k, v in vads:
        want = R.apply(stored[k], R.cmvn_norm(stats[utt2spk[k]]))[v != 0]
        assert voiced[k].shape == want.shape and np.array_equal(voiced[k].view(np.uint32), want.view(np.uint32)), k
