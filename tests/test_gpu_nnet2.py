"""GPU tests of nnet-am-compute through the C ABI (xv_nnet2_compute) and the command line: a miniature of the recipe's network (dim 8,
the recipe's splices, LDA 40 -> 24, p-norm 60 -> 6, final 6 -> 37, sum-group -> 17) against float64 under the rule of
nnet2_ref.tolerance; a frame's row byte for byte alone, in a batch, across row blocks and for every --chunk-size; the options; the
recipe's dimensions; and the shell pipeline of sid/extract_ivectors_dnn.sh:92-95.  Every command runs under its own timeout."""
import os
import subprocess

import numpy as np
import pytest

import helpers as H
import nnet2_ref as R
from oracle import kaldi_io as kio

pytestmark = pytest.mark.gpu

BIN = os.path.join(H.ROOT, H.PKG_NAME, "bin")
LENGTHS = (1, 2, 12, 13, 22, 23, 50, 300)   # around the left (13), the right (9) and the whole (22) context


def _sh(line, cwd, limit=120):
    env = dict(os.environ, PATH=BIN + os.pathsep + os.environ.get("PATH", ""))
    return subprocess.run(["/bin/sh", "-c", "timeout -k 10 %d %s" % (limit, line) if "|" not in line else line], stdout=subprocess.PIPE,
                          stderr=subprocess.PIPE, env=env, cwd=cwd, timeout=limit + 60)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def mini(tmp_path_factory):
    d = tmp_path_factory.mktemp("nnet2")
    comps, priors = R.miniature()
    rng = np.random.default_rng(9)
    utts = [("utt%03d" % t, rng.normal(size=(t, 8)).astype(np.float32)) for t in LENGTHS]
    R.write_model(str(d / "final.mdl"), comps, priors, True)
    R.write_model(str(d / "final.txt.mdl"), comps, priors, False)
    kio.write_ark_matrices(str(d / "feats.ark"), utts)
    net = H.pkg().nnet2.Nnet2(str(d / "final.mdl"))
    # the references, once
    ref64 = [R.forward(comps, priors, x, apply_log=True) for _, x in utts]
    ref32 = [R.forward(comps, priors, x, np.float32, apply_log=True) for _, x in utts]
    alone = [net.compute([x], apply_log=True)[0] for _, x in utts]
    return dict(dir=d, comps=comps, priors=priors, utts=utts, net=net, ref64=ref64, ref32=ref32, alone=alone)


def test_log_posteriors_against_float64(mini):
    worst = 0.0
    for (key, x), got, r64, r32 in zip(mini["utts"], mini["alone"], mini["ref64"], mini["ref32"]):
        tol = R.tolerance(r64, r32)
        err = np.abs(got - r64)
        worst = max(worst, float((err / tol).max()))
        assert got.shape == r64.shape == (len(x), 17) and np.all(err <= tol), key
    print("miniature network: largest error / bound %.3g" % worst)
    top = np.exp(np.concatenate(mini["ref64"])).max(axis=1)
    assert top.min() > 0.2 and np.ptp(top) > 1e-3   # not flat over the 17 senones, and a function of the frame far above the bound


def test_a_row_is_the_same_bytes_alone_in_a_batch_and_across_blocks(mini):
    net, xs = mini["net"], [x for _, x in mini["utts"]]
    order = [6, 0, 7, 3, 1, 5, 2, 4]
    for block in (16, 48, 0):
        got = net.compute([xs[i] for i in order], apply_log=True, block_rows=block)
        for i, g in zip(order, got):
            assert np.array_equal(_bits(g), _bits(mini["alone"][i])), (block, i)
    for block in (16, 48):
        assert np.array_equal(_bits(net.compute([xs[7]], apply_log=True, block_rows=block)[0]), _bits(mini["alone"][7]))
    # nothing of the head's options reaches the layers: without the logarithm the same rows, exponentiated
    post = net.compute([xs[7]])[0]
    assert np.allclose(np.log(post), mini["alone"][7], atol=1e-5) and np.allclose(post.sum(axis=1), 1.0, atol=1e-5)


def test_chunk_size_changes_no_byte_and_text_and_binary_models_agree(mini):
    d = str(mini["dir"])
    want = None
    for i, (model, chunk) in enumerate((("final.mdl", 0), ("final.mdl", 1), ("final.mdl", 7), ("final.mdl", 256), ("final.txt.mdl", 256))):
        r = _sh("nnet-am-compute --use-gpu=yes --apply-log=true --chunk-size=%d %s ark:feats.ark ark:out%d.ark" % (chunk, model, i), d)
        assert r.returncode == 0 and b"Done 8 utterances, 423 frames; 0 with errors." in r.stderr, r.stderr
        got = open(os.path.join(d, "out%d.ark" % i), "rb").read()
        want = want or got
        assert got == want, (model, chunk)
    table = dict(kio.read_ark(os.path.join(d, "out0.ark")))
    for (key, _), a in zip(mini["utts"], mini["alone"]):
        assert np.array_equal(_bits(table[key]), _bits(a)), key


def test_without_padding_the_rows_whose_context_is_there(mini):
    net, xs = mini["net"], [x for _, x in mini["utts"]]
    got = net.compute(xs, apply_log=True, pad_input=False)
    assert [len(g) for g in got] == [0, 0, 0, 0, 0, 1, 28, 278]
    for g, a in zip(got[5:], mini["alone"][5:]):
        assert np.array_equal(_bits(g), _bits(a[13:len(a) - 9]))
    d = str(mini["dir"])
    r = _sh("nnet-am-compute --pad-input=false --apply-log=true final.mdl ark:feats.ark ark:nopad.ark", d)
    assert r.returncode == 0 and b"Done 3 utterances, 307 frames; 5 with errors." in r.stderr and r.stderr.count(b"WARNING (nnet-am-compute") == 5, r.stderr
    table = dict(kio.read_ark(os.path.join(d, "nopad.ark")))
    assert sorted(table) == ["utt023", "utt050", "utt300"] and np.array_equal(_bits(table["utt050"]), _bits(got[6]))
    # an empty utterance is skipped with a warning, and a table of nothing else is exit status 1
    kio.write_ark_matrices(os.path.join(d, "empty.ark"), [("none", np.zeros((0, 8), np.float32))])
    r = _sh("nnet-am-compute final.mdl ark:empty.ark ark:/dev/null", d)
    assert r.returncode == 1 and b"Zero-length utterance: none" in r.stderr and b"Done 0 utterances" in r.stderr


def test_divide_by_priors(mini):
    P = H.pkg()
    net, (key, x) = mini["net"], mini["utts"][6]
    for log in (False, True):
        got = net.compute([x], apply_log=log, divide_by_priors=True)[0]
        r64 = R.forward(mini["comps"], mini["priors"], x, apply_log=log, divide_by_priors=True)
        r32 = R.forward(mini["comps"], mini["priors"], x, np.float32, apply_log=log, divide_by_priors=True)
        assert np.all(np.abs(got - r64) <= R.tolerance(r64, r32)), log
    d = mini["dir"]
    bare = P.nnet2.Nnet2(R.write_model(str(d / "nopriors.mdl"), mini["comps"], ()))
    with pytest.raises(P.XvError) as e:
        bare.compute([x], divide_by_priors=True)
    assert e.value.status == P.XV_ERR_ARG and "the model has no priors" in str(e.value)
    assert np.array_equal(_bits(bare.compute([x], apply_log=True)[0]), _bits(mini["alone"][6]))
    r = _sh("nnet-am-compute --divide-by-priors=true nopriors.mdl ark:feats.ark ark:/dev/null", str(d))
    assert r.returncode == 255 and b"ERROR (nnet-am-compute) --divide-by-priors=true, but the model has no priors" in r.stderr


def test_the_recipe_s_dimensions(tmp_path):
    """40-dim input, the four splices, 3500 -> 350, 10500 -> 5000 outputs, six hidden layers: 20 frames"""
    P = H.pkg()
    rng = np.random.default_rng(12)
    comps = R.multisplice(rng, 40, 200, 3500, 350, 10500, R.random_sizes(rng, 10500, 5000), extra_hidden=1, final_std=0.3)
    net = P.nnet2.Nnet2(R.write_model(str(tmp_path / "final.mdl"), comps, ()))
    i = net.info
    assert (i["left_context"], i["right_context"], i["input_dim"], i["output_dim"], i["max_plane_cols"], i["max_pre_cols"]) == (13, 9, 40, 5000, 352, 10500)
    x = rng.normal(size=(20, 40)).astype(np.float32)
    got = net.compute([x], apply_log=True)[0]
    r64, r32 = R.forward(comps, (), x, apply_log=True), R.forward(comps, (), x, np.float32, apply_log=True)
    tol = R.tolerance(r64, r32)
    err = np.abs(got - r64)
    print("recipe dimensions: largest error / bound %.3g, fp32 restatement %.3g" % ((err / tol).max(), np.abs(r32 - r64).max()))
    assert got.shape == (20, 5000) and np.all(err <= tol)
    assert np.array_equal(_bits(net.compute([x, x[:7]], apply_log=True, block_rows=8)[0]), _bits(got))


def test_a_relu_network_against_float64(tmp_path):
    """splice, affine, ReLU, normalize; affine, ReLU; affine, softmax: the stage's other nonlinearity, with and without normalize"""
    P = H.pkg()
    comps, priors = R.relu_model()
    net = P.nnet2.Nnet2(R.write_model(str(tmp_path / "relu.mdl"), comps, priors))
    rng = np.random.default_rng(5)
    xs = [rng.normal(size=(t, 5)).astype(np.float32) for t in (1, 3, 4, 70)]
    got = net.compute(xs, apply_log=True, block_rows=16)
    for x, g in zip(xs, got):
        r64, r32 = R.forward(comps, priors, x, apply_log=True), R.forward(comps, priors, x, np.float32, apply_log=True)
        assert g.shape == r64.shape and np.all(np.abs(g - r64) <= R.tolerance(r64, r32)), len(x)
        assert np.array_equal(_bits(g), _bits(net.compute([x], apply_log=True)[0]))
    assert [len(g) for g in net.compute(xs, pad_input=False)] == [0, 0, 1, 67]


def _read_text_post(path):
    out = {}
    for line in open(path):
        key, rest = line.split(None, 1)
        frames = [f.split() for f in rest.replace("]", "").split("[")[1:]]
        out[key] = [frozenset(int(t) for t in f[0::2]) for f in frames]
    return out


def test_the_pipeline_of_extract_ivectors_dnn(tmp_path):
    """nnet-am-compute | select-voiced-frames | logprob-to-post --min-post=0.025 as sid/extract_ivectors_dnn.sh:92-95 writes it, with
    --random-prune=false (the draws of the random pruning have their own tests: tests/test_gpu_logprob_post.py): the (frame, senone)
    sets of the float64 reference, frames with a reference posterior within the tolerance of the threshold left out - at most 2 %
    (tests/test_nnet2_ref.py holds the fp32 restatement to the same).  Then the line exactly as written, with the default random pruning:
    every reference pair at or above the threshold is there."""
    comps, priors, utts, vads = R.pipeline_case()
    d = str(tmp_path)
    R.write_model(os.path.join(d, "final.mdl"), comps, priors)
    kio.write_ark_matrices(os.path.join(d, "feats.ark"), utts, scp_path=os.path.join(d, "feats.scp"))
    kio.write_ark_vectors(os.path.join(d, "vad.ark"), vads, scp_path=os.path.join(d, "vad.scp"))
    r = _sh("timeout -k 10 120 nnet-am-compute --use-gpu=yes --apply-log=true --chunk-size=256 final.mdl scp:feats.scp ark:- "
            "| timeout -k 10 120 select-voiced-frames ark:- scp,s,cs:vad.scp ark:- "
            "| timeout -k 10 120 logprob-to-post --min-post=0.025 --random-prune=false ark:- ark,t:post.txt", d, limit=300)
    assert r.returncode == 0 and b"Done 3 utterances, 237 frames; 0 with errors." in r.stderr, r.stderr
    got = _read_text_post(os.path.join(d, "post.txt"))
    left_out = total = 0
    wants, nears = {}, {}
    for (key, x), (_, v) in zip(utts, vads):
        l64, l32 = R.forward(comps, priors, x, apply_log=True), R.forward(comps, priors, x, np.float32, apply_log=True)
        p64 = np.exp(l64)
        near = R.near_threshold(p64, R.tolerance(l64, l32) * p64, v)
        want = R.kept_sets(p64, v)
        wants[key], nears[key] = want, near
        assert len(got[key]) == len(want) == int(v.sum())
        assert all(g == w for g, w, n in zip(got[key], want, near) if not n), key
        left_out += int(near.sum())
        total += len(near)
    print("pipeline: %d of %d voiced frames left out" % (left_out, total))
    assert left_out <= 0.02 * total
    # exactly as the script writes it, with the default --random-prune=true: what reaches the threshold is kept whatever is drawn,
    # and what is drawn is only added to it
    r = _sh("timeout -k 10 120 nnet-am-compute --use-gpu=yes --apply-log=true --chunk-size=256 final.mdl scp:feats.scp ark:- "
            "| timeout -k 10 120 select-voiced-frames ark:- scp,s,cs:vad.scp ark:- "
            "| timeout -k 10 120 logprob-to-post --min-post=0.025 ark:- ark,t:post_default.txt", d, limit=300)
    assert r.returncode == 0 and b"Done 3 utterances, 237 frames; 0 with errors." in r.stderr, r.stderr
    drawn = _read_text_post(os.path.join(d, "post_default.txt"))
    for key, _ in utts:
        assert len(drawn[key]) == len(got[key])
        assert all(w <= g or n for g, w, n in zip(drawn[key], wants[key], nears[key])), key
