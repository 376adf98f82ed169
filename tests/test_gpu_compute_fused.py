"""nnet3-compute with the recipes' feature pipelines run on the device (csrc/fuse_pipe.h, table_compute.cc RunTableCompute): every
case is the tool's command line run twice - as it is, where the pipeline is recognised and fused, and under XVEC_DEBUG=fuse_pipe=0,
where the commands it names are run - and the two must write the same bytes, skip the same utterances with the same words and end
with the same status.  The network is the "am" one of tests/helpers.py; --batch-frames=256 makes every job several batches."""
import functools
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import helpers as H
from oracle import frontend as fe
from oracle import kaldi_io as kio

pytestmark = pytest.mark.gpu
BIN = os.path.join(H.ROOT, H.PKG_NAME, "bin")
SPK2UTT = {"spkA": ["spkA-u1", "spkA-u2", "spkA-u3"], "spkB": ["spkB-u1"], "spkC": ["spkC-u1", "spkC-u2", "spkC-u3"]}
LENS = {"spkA-u1": 120, "spkA-u2": 7, "spkA-u3": 200, "spkB-u1": 333, "spkC-u1": 61, "spkC-u2": 258, "spkC-u3": 90}
BOTTLENECK = ["--output-node=tdnn5.batchnorm"]


def _sh(argv, env_extra=None):
    env = dict(os.environ, PATH=BIN + os.pathsep + os.environ.get("PATH", ""))
    env.pop("XVEC_DEBUG", None)
    env.update(env_extra or {})
    return subprocess.run(argv, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env, timeout=300)


@functools.lru_cache(maxsize=None)
def _model(d, dim=23):
    text = H.config_text("am")
    if dim != 23:
        text = text.replace("input-node name=input dim=23", "input-node name=input dim=%d" % dim).replace("input-dim=115", "input-dim=%d" % (5 * dim))
    path = os.path.join(d, "am%d.raw" % dim)
    open(path, "wb").write(H.nm.synthesize([text], seed=21, head_stddev=1.0).to_bytes(True))
    return path


def _data(d, lens, spk2utt, dim=23, compressed="CM", seed=900):
    """The split data directory of the scripts: feats.scp over a raw archive, spk2utt / utt2spk, cmvn.scp from the project's
    compute-cmvn-stats, and a vad.scp."""
    os.makedirs(d)
    utts = [(k, H.features(seed + i, lens[k], dim) + np.float32(3.0 * (i % 3))) for i, k in enumerate(sorted(lens))]
    kio.write_ark_matrices(os.path.join(d, "raw.ark"), utts, scp_path=os.path.join(d, "feats.scp"), compressed=compressed)
    open(os.path.join(d, "spk2utt"), "w").write("".join("%s %s\n" % (s, " ".join(us)) for s, us in spk2utt.items()))
    open(os.path.join(d, "utt2spk"), "w").write("".join("%s %s\n" % (u, s) for s, us in sorted(spk2utt.items()) for u in us))
    vads = [(k, fe.synthetic_vad(60 + i, lens[k])) for i, k in enumerate(sorted(lens))]
    kio.write_ark_vectors(os.path.join(d, "vad.ark"), vads, scp_path=os.path.join(d, "vad.scp"))
    r = _sh([os.path.join(BIN, "compute-cmvn-stats"), "--spk2utt=ark:%s/spk2utt" % d, "scp:%s/feats.scp" % d,
             "ark,scp:%s/cmvn.ark,%s/cmvn.scp" % (d, d)])
    assert r.returncode == 0, r.stderr
    return d


@pytest.fixture(scope="module")
def base(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("fused"))
    return root, _data(os.path.join(root, "cm"), LENS, SPK2UTT)


def _message(log, pattern):
    """The messages of the log lines that match, without the 'LEVEL (program:...)' prefix, which names the program that spoke."""
    return re.findall(r"^(?:LOG|WARNING) \(\S+\) (%s.*)$" % pattern, log, flags=re.M)


def _both(root, tag, model, feats, options=BOTTLENECK):
    """The command line fused and as commands: (fused run, run as commands, {tag: archive bytes}, {tag: keys})."""
    runs, arks, keys = {}, {}, {}
    for how, env in (("fused", {}), ("commands", {"XVEC_DEBUG": "fuse_pipe=0"})):
        out = os.path.join(root, "%s_%s" % (tag, how))
        r = _sh([os.path.join(BIN, "nnet3-compute"), "--use-gpu=no", "--batch-frames=256"] + list(options) +
                [model, feats, "ark,scp:%s.ark,%s.scp" % (out, out)], env)
        runs[how] = r
        arks[how] = open(out + ".ark", "rb").read() if os.path.exists(out + ".ark") else None
        keys[how] = [l.split()[0] for l in open(out + ".scp")] if os.path.exists(out + ".scp") else None
    assert "feature pipeline recognised" in runs["fused"].stderr, runs["fused"].stderr
    assert "feature pipeline recognised" not in runs["commands"].stderr, runs["commands"].stderr
    return runs["fused"], runs["commands"], arks, keys


def _same_output(fused, commands, arks, keys, want_keys):
    assert fused.returncode == 0, fused.stderr
    assert commands.returncode == 0, commands.stderr
    assert keys["fused"] == keys["commands"] == want_keys
    assert len(arks["fused"]) > 0 and arks["fused"] == arks["commands"]
    # what the tools in front report, and nnet3-compute's own last line
    for pattern in ("Applied ", "Done selecting voiced frames", r"Done \d+ utterances"):
        assert _message(fused.stderr, pattern) == _message(commands.stderr, pattern), pattern
    assert len(_message(fused.stderr, r"Done \d+ utterances")) == 1


def _forms(d):
    bn = "ark,s,cs:apply-cmvn %%s --utt2spk=ark:%s/utt2spk scp:%s/cmvn.scp scp:%s/feats.scp ark:- |" % (d, d, d)
    sliding = "ark:apply-cmvn-sliding --norm-vars=false --center=true --cmn-window=300 scp:%s/feats.scp ark:- |" % d
    select = " select-voiced-frames ark:- scp,s,cs:%s/vad.scp ark:- |" % d
    return {
        "extract_bn": (bn % "", "Applied cepstral mean normalization to 7 utterances, errors on 0"),
        "extract_bn_norm_vars": (bn % "--norm-vars=true", "Applied cepstral mean and variance normalization to 7 utterances, errors on 0"),
        "extract_bn_select": (bn % "" + select, "Applied cepstral mean normalization to 7 utterances, errors on 0"),
        "extract_log_post_plain": (sliding, "Applied sliding-window cepstral mean normalization to 7 utterances, 0 had errors."),
        "extract_log_post_select": (sliding + select, "Applied sliding-window cepstral mean normalization to 7 utterances, 0 had errors."),
    }


@pytest.mark.parametrize("form", ["extract_bn", "extract_bn_norm_vars", "extract_bn_select", "extract_log_post_plain", "extract_log_post_select"])
def test_the_scripts_strings_give_the_same_bytes_fused_and_as_commands(base, form):
    root, d = base
    feats, applied = _forms(d)[form]
    fused, commands, arks, keys = _both(root, form, _model(root), feats)
    _same_output(fused, commands, arks, keys, sorted(LENS))
    assert _message(fused.stderr, "Applied ") == [applied]
    assert ("Done selecting voiced frames; processed 7 utterances, 0 had errors." in fused.stderr) == form.endswith("select")
    assert "Done 7 utterances, failed for 0" in fused.stderr
    rows = {k: m.shape for k, m in kio.read_ark(os.path.join(root, form + "_fused.ark"))}
    voiced = {k: int(np.count_nonzero(fe.synthetic_vad(60 + i, LENS[k]))) for i, k in enumerate(sorted(LENS))}
    assert rows == {k: (voiced[k] if form.endswith("select") else LENS[k], 128) for k in LENS}


@pytest.mark.parametrize("dim,compressed", [(23, None), (65, "CM")])
def test_float_and_wide_features_take_the_float_upload(base, dim, compressed):
    """An archive of float matrices ("FM") read as "ark:", and stored features of 65 columns, which the device expansion does not
    take: both go up as float rows."""
    root, _ = base
    d = _data(os.path.join(root, "f%d" % dim), LENS, SPK2UTT, dim=dim, compressed=compressed, seed=300 + dim)
    feats = "ark,s,cs:apply-cmvn --norm-vars=true --utt2spk=ark:%s/utt2spk scp:%s/cmvn.scp ark:%s/raw.ark ark:- |" % (d, d, d)
    fused, commands, arks, keys = _both(root, "float%d" % dim, _model(root, dim), feats)
    _same_output(fused, commands, arks, keys, sorted(LENS))


def test_apply_exp_on_the_log_softmax_head(base):
    root, d = base
    feats = _forms(d)["extract_bn_select"][0]
    fused, commands, arks, keys = _both(root, "exp", _model(root), feats, options=["--apply-exp=true"])
    _same_output(fused, commands, arks, keys, sorted(LENS))
    post = dict(kio.read_ark(os.path.join(root, "exp_fused.ark")))
    assert post["spkB-u1"].shape[1] == 5139 and abs(float(post["spkB-u1"][0].sum()) - 1.0) < 1e-3


def test_both_runs_skip_the_same_utterances_with_the_tools_words(base):
    """spkB has no statistics; of the others one utterance has no VAD entry, one a VAD of another length, one no voiced frame."""
    root, d = base
    e = os.path.join(root, "errors")
    os.makedirs(e)
    open(os.path.join(e, "cmvn.scp"), "w").write("".join(l for l in open(os.path.join(d, "cmvn.scp")) if not l.startswith("spkB ")))
    vads = []
    for i, k in enumerate(sorted(LENS)):
        v = fe.synthetic_vad(60 + i, LENS[k])
        if k == "spkA-u3":
            continue                      # no entry
        if k == "spkC-u1":
            v = v[:-3]                    # another length
        if k == "spkC-u3":
            v = np.zeros_like(v)          # nothing voiced
        vads.append((k, v))
    kio.write_ark_vectors(os.path.join(e, "vad.ark"), vads, scp_path=os.path.join(e, "vad.scp"))
    feats = ("ark,s,cs:apply-cmvn  --utt2spk=ark:%s/utt2spk scp:%s/cmvn.scp scp:%s/feats.scp ark:- | select-voiced-frames ark:- scp,s,cs:%s/vad.scp ark:- |"
             % (d, e, d, e))
    fused, commands, arks, keys = _both(root, "errors", _model(root), feats)
    _same_output(fused, commands, arks, keys, ["spkA-u1", "spkA-u2", "spkC-u2"])
    warnings = ["No normalization statistics available for key spkB-u1, producing no output for this utterance",
                "No VAD input found for utterance spkA-u3",
                "Mismatch in number of frames 61 for features and VAD 58, for utterance spkC-u1",
                "No features were judged as voiced for utterance spkC-u3"]
    for w in warnings:
        assert fused.stderr.count(w) == 1 and commands.stderr.count(w) == 1, w
    assert "Applied cepstral mean normalization to 6 utterances, errors on 1" in fused.stderr
    assert "Done selecting voiced frames; processed 3 utterances, 3 had errors." in fused.stderr
    assert "Done 3 utterances, failed for 0" in fused.stderr


def test_statistics_of_another_width_end_both_runs_with_255(base):
    root, d = base
    e = os.path.join(root, "width")
    os.makedirs(e)
    with open(os.path.join(e, "cmvn.ark"), "wb") as f:
        for s in sorted(SPK2UTT):
            st = np.zeros((2, 25), dtype="<f8")       # the statistics of 24 columns; the features have 23
            st[0, :] = 100.0
            st[1, :24] = 200.0
            f.write(s.encode() + b" \x00BDM \x04" + struct.pack("<i", 2) + b"\x04" + struct.pack("<i", 25) + st.tobytes())
    feats = "ark,s,cs:apply-cmvn --utt2spk=ark:%s/utt2spk ark:%s/cmvn.ark scp:%s/feats.scp ark:- |" % (d, e, d)
    fused, commands, arks, keys = _both(root, "width", _model(root), feats)
    assert fused.returncode == 255 and commands.returncode == 255, (fused.returncode, commands.returncode)
    message = "Dimension mismatch: cmvn stats have dimension 2x25, feats have dimension 23 (utterance spkA-u1)"
    assert message in fused.stderr and message in commands.stderr
    assert not keys["fused"] and not keys["commands"]


def test_forty_utterances_come_out_in_table_order(base):
    root, _ = base
    rng = np.random.default_rng(40)
    lengths = [1, 300] + [int(x) for x in rng.integers(1, 301, size=38)]
    rng.shuffle(lengths)
    lens = {"s%d-utt%02d" % (i % 5, i): n for i, n in enumerate(lengths)}
    spk2utt = {"s%d" % s: [k for k in lens if k.startswith("s%d-" % s)] for s in range(5)}
    d = _data(os.path.join(root, "forty"), lens, spk2utt, seed=5000)
    table = [l.split()[0] for l in open(os.path.join(d, "feats.scp"))]
    assert table == sorted(lens) and len(table) == 40
    feats = "ark,s,cs:apply-cmvn  --utt2spk=ark:%s/utt2spk scp:%s/cmvn.scp scp:%s/feats.scp ark:- |" % (d, d, d)
    fused, commands, arks, keys = _both(root, "forty", _model(root), feats)
    _same_output(fused, commands, arks, keys, table)
    assert [(k, m.shape[0]) for k, m in kio.read_ark(os.path.join(root, "forty_fused.ark"))] == [(k, lens[k]) for k in table]
