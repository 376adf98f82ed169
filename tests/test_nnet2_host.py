"""CPU tests of the host half of nnet-am-compute: the model reader and its lowering through bin/nnet-am-info (which opens no
device), every refusal by its message, truncated files, and the plan that cuts the packed sequence into row blocks of a bounded
device workspace (xv_nnet2_plan: pure, through the library without a device).  No GPU is needed or looked for."""
import os
import subprocess

import numpy as np
import pytest

import helpers as H
import nnet2_ref as R

BIN = os.path.join(H.ROOT, H.PKG_NAME, "bin")
INFO = os.path.join(BIN, "nnet-am-info")
# what DimsOf gives for the recipe's network (40-dim input, 3500 -> 350 p-norm, 10500 -> 5000 outputs): planes of 352 halves (350
# rounded up to the K tile), pre-activations of 10500 floats, the largest splice offset 7
RECIPE = dict(num_components=0, num_updatable_components=0, left_context=13, right_context=9, input_dim=40, output_dim=5000, softmax_dim=10500,
              prior_dim=5000, num_layers=8, max_plane_cols=352, max_pre_cols=10500, halo=7, parameter_dim=0)


def _info(path):
    return subprocess.run([INFO, path], stdin=subprocess.DEVNULL, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)


def _refused(tmp_path, comps, priors=(), binary=True):
    r = _info(R.write_model(str(tmp_path / "bad.mdl"), comps, priors, binary))
    assert r.returncode == 255 and r.stdout == b"", (r.returncode, r.stderr)
    lines = r.stderr.decode().splitlines()
    assert lines[-1].startswith("ERROR (nnet-am-info) "), lines
    return lines[-1]


@pytest.mark.parametrize("binary", [True, False])
def test_info_lines_of_a_written_model(tmp_path, binary):
    comps, priors = R.miniature()
    r = _info(R.write_model(str(tmp_path / "final.mdl"), comps, priors, binary))
    assert r.returncode == 0, r.stderr.decode()
    out = r.stdout.decode()
    lines = out.splitlines()
    n_params = sum(np.asarray(c[1]).size + np.asarray(c[2]).size for c in comps if c[0] in R.AFFINE and c[0] != "FixedAffine")
    assert lines[:7] == ["num-components %d" % len(comps), "num-updatable-components 6", "left-context 13", "right-context 9", "input-dim 8",
                         "output-dim 17", "parameter-dim %d" % n_params]
    assert lines[7] == "component 0 : SpliceComponent, input-dim=8, output-dim=40, context=-2:-1:0:1:2"
    assert lines[8] == "component 1 : FixedAffineComponent, input-dim=40, output-dim=24"
    assert lines[10] == "component 3 : PnormComponent, input-dim=60, output-dim=6"
    assert lines[-2] == "component %d : SumGroupComponent, input-dim=37, output-dim=17" % (len(comps) - 1)
    assert lines[-1] == "prior dimension: 17" and len(lines) == 7 + len(comps) + 1
    # sid/init_full_ubm_from_dnn.sh:94 takes the senone count with grep -oP 'output-dim\ \K[0-9]+'
    assert out.count("output-dim ") == 1 and out.count("output-dim=") == len(comps)


def test_binary_and_text_give_the_same_lines_and_the_old_splice_spelling_the_same_contexts(tmp_path):
    rng = np.random.default_rng(3)
    comps = R.multisplice(rng, 8, 24, 60, 6, 37, legacy_first=True)
    outs = [_info(R.write_model(str(tmp_path / ("m%d.mdl" % b)), comps, (), bool(b))).stdout for b in (0, 1)]
    assert outs[0] == outs[1] and b"left-context 13\nright-context 9\n" in outs[0] and outs[0].endswith(b"prior dimension: 0\n")
    assert b"context=-2:-1:0:1:2" in outs[0]


def test_a_relu_network_is_read_and_lowered(tmp_path):
    P = H.pkg()
    comps, priors = R.relu_model()
    for binary in (True, False):
        path = R.write_model(str(tmp_path / ("relu%d.mdl" % binary)), comps, priors, binary)
        lines = _info(path).stdout.decode().splitlines()
        assert lines[:7] == ["num-components 8", "num-updatable-components 3", "left-context 2", "right-context 1", "input-dim 5", "output-dim 12",
                             "parameter-dim %d" % (20 * 15 + 20 + 9 * 20 + 9 + 12 * 9 + 12)]
        assert lines[9] == "component 2 : RectifiedLinearComponent, input-dim=20, output-dim=20" and lines[-1] == "prior dimension: 0"
        i = P.nnet2.Nnet2(path).info
        assert (i["num_layers"], i["max_plane_cols"], i["max_pre_cols"], i["halo"]) == (3, 32, 20, 2)


def test_a_splice_wider_than_the_kernel_takes_is_refused_by_the_reader(tmp_path):
    rng = np.random.default_rng(8)
    ctx = list(range(-16, 17))   # 33 offsets
    comps = [("Splice", 2, ctx), ("Affine", rng.normal(size=(3, 66)), np.zeros(3)), ("Softmax", 3)]
    assert "component 0 (SpliceComponent): 33 offsets are more than the 32 the affine kernel takes" in _refused(tmp_path, comps)
    assert _info(R.write_model(str(tmp_path / "ok.mdl"), [("Splice", 2, ctx[1:]), ("Affine", rng.normal(size=(3, 64)), np.zeros(3)), ("Softmax", 3)])).returncode == 0


def test_usage_and_missing_file():
    r = subprocess.run([INFO], stdin=subprocess.DEVNULL, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert r.returncode == 1 and b"Usage: nnet-am-info <nnet-in>" in r.stderr
    r = _info("/nonexistent/final.mdl")
    assert r.returncode == 255 and r.stderr.decode().splitlines()[-1].startswith("ERROR (nnet-am-info) ")
    r = subprocess.run([os.path.join(BIN, "nnet-am-compute"), "--chunk-size=4", "--pad-input=false", "a", "ark:b", "ark:c"], stdin=subprocess.DEVNULL,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert r.returncode == 255 and "ERROR (nnet-am-compute) --chunk-size > 0 requires --pad-input=true" in r.stderr.decode().splitlines()


# ------------------------------------------------------------------------------------------------------------------- the refusals
def _tiny(rng, **kw):
    return R.multisplice(rng, 4, 6, 8, 4, 5, splices=([-1, 0, 1], [-1, 1]), **kw)


def test_every_refusal_names_its_component(tmp_path):
    rng = np.random.default_rng(5)
    good = _tiny(rng)
    assert _info(R.write_model(str(tmp_path / "good.mdl"), good)).returncode == 0
    # another component type
    bad = list(good)
    bad[4] = ("Sigmoid", 4)
    assert "component 4 is a SigmoidComponent, which nnet-am-compute does not evaluate" in _refused(tmp_path, bad)
    # const-component-dim
    bad = list(good)
    bad[0] = ("Splice", 4, [-1, 0, 1], False, 2)
    assert "component 0 (SpliceComponent): const-component-dim=2 is not built" in _refused(tmp_path, bad)
    # P
    bad = list(good)
    bad[3] = ("Pnorm", 8, 4, 1.0)
    assert "component 3 (PnormComponent): P=1.000000 is not built (only the 2-norm)" in _refused(tmp_path, bad)
    # p-norm dimensions
    bad = list(good)
    bad[3] = ("Pnorm", 8, 3)
    assert "component 3 (PnormComponent): input-dim=8 is not a multiple of output-dim=3" in _refused(tmp_path, bad)
    # the end of the network
    assert "does not end in SoftmaxComponent [SumGroupComponent] (its last component is AffineComponentPreconditionedOnline)" in _refused(tmp_path, good[:-1])
    assert "does not end in an affine component, SoftmaxComponent [SumGroupComponent]" in _refused(tmp_path, good[:-2] + [("Softmax", 4)])
    # dimensions that do not chain
    bad = list(good)
    bad[4] = ("Normalize", 5)
    assert "the dimensions do not chain: component 3 (PnormComponent) gives 4, component 4 (NormalizeComponent) takes 5" in _refused(tmp_path, bad)
    bad = good + [("SumGroup", [2, 2])]
    assert "the dimensions do not chain: component %d (SoftmaxComponent) gives 5, component %d (SumGroupComponent) takes 4" % (len(good) - 1, len(good)) in \
        _refused(tmp_path, bad, binary=False)


def test_a_truncated_model_is_an_input_error_never_a_signal(tmp_path):
    comps, priors = R.miniature()
    blob = R.model_bytes(comps, priors, True)
    path = str(tmp_path / "cut.mdl")
    cuts = list(range(0, len(blob), 97))
    assert len(cuts) > 50
    for n in cuts:
        with open(path, "wb") as f:
            f.write(blob[:n])
        r = _info(path)
        assert r.returncode == 255 and r.stdout == b"" and r.stderr.decode().splitlines()[-1].startswith("ERROR (nnet-am-info) "), (n, r.returncode, r.stderr)


# ------------------------------------------------------------------------------------------------------------------------ the plan
def _blocks(rows, rpb, n):
    return [(b * rpb, min(rows, (b + 1) * rpb)) for b in range(n)]


def test_the_plan_is_pure_and_its_blocks_cover_every_row_once():
    P = H.pkg()
    rng = np.random.default_rng(7)
    for _ in range(200):
        rows = int(rng.integers(0, 300000))
        block = int(rng.integers(0, 2)) * int(rng.integers(1, 800))
        cap = int(rng.integers(64, 1024)) << 20
        a = P.nnet2.plan(RECIPE, rows, block, cap)
        assert a == P.nnet2.plan(dict(RECIPE), rows, block, cap)
        rpb, n, nbytes = a
        assert rpb >= 1 and nbytes <= cap and (block == 0 or rpb == block)
        blocks = _blocks(rows, rpb, n)
        assert n == -(-rows // rpb) and all(b > a_ for a_, b in blocks)
        assert [a_ for a_, _ in blocks] == [b for _, b in [(0, 0)] + blocks[:-1]] and (not blocks or blocks[-1][1] == rows)
    assert P.nnet2.plan(RECIPE, 0)[1:] == (0, 0)


def test_a_thirty_minute_recording_stays_under_the_cap():
    P = H.pkg()
    rows = 200000 + 13 + 9
    rpb, n, nbytes = P.nnet2.plan(RECIPE, rows)
    assert nbytes <= 256 << 20 and n > 1 and rpb * n >= rows
    assert P.nnet2.plan(RECIPE, rows, 0, 64 << 20)[2] <= 64 << 20
    # the most that fit: one more row per block would not
    per_row = P.nnet2.plan(RECIPE, rows, 2)[2] - P.nnet2.plan(RECIPE, rows, 1)[2]
    assert nbytes + per_row > 256 << 20 and per_row == 2 * 352 * 2 + 10500 * 4 + 40 * 4 + 5000 * 4 + 4
    # a short sequence takes what it needs
    assert P.nnet2.plan(RECIPE, 100) == (100, 1, P.nnet2.plan(RECIPE, 100, 100)[2])


def test_a_workspace_that_cannot_hold_one_block_is_an_argument_error():
    P = H.pkg()
    one = P.nnet2.plan(RECIPE, 10, 1)[2]
    assert P.nnet2.plan(RECIPE, 10, 1, one) == (1, 10, one)
    for args in ((10, 1, one - 1), (10, 0, one - 1), (10, 5000, 64 << 20), (-1, 0, 0), (10, (1 << 20) + 1, 0)):
        with pytest.raises(P.XvError) as e:
            P.nnet2.plan(RECIPE, *args)
        assert e.value.status == P.XV_ERR_ARG, args
    with pytest.raises(P.XvError) as e:
        P.nnet2.plan(dict(RECIPE, max_pre_cols=0), 10)
    assert e.value.status == P.XV_ERR_ARG


def test_opening_a_model_needs_no_device_and_gives_its_dimensions(tmp_path):
    P = H.pkg()
    comps, priors = R.miniature()
    m = P.nnet2.Nnet2(R.write_model(str(tmp_path / "final.mdl"), comps, priors))
    i = m.info
    assert (i["left_context"], i["right_context"], i["input_dim"], i["output_dim"], i["softmax_dim"], i["prior_dim"]) == (13, 9, 8, 17, 37, 17)
    assert (i["num_layers"], i["max_plane_cols"], i["max_pre_cols"], i["halo"]) == (7, 32, 60, 7)
    assert m.out_rows(30) == 30 and m.out_rows(30, False) == 8 and m.out_rows(22, False) == 0 and m.out_rows(0) == 0
    m.close()
    with pytest.raises(P.XvError) as e:
        P.nnet2.Nnet2(R.write_model(str(tmp_path / "bad.mdl"), comps[:-2], priors))
    assert e.value.status == P.XV_ERR_IO and "does not end in SoftmaxComponent" in str(e.value)
