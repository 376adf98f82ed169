"""The host side of the phonetic i-vector path (csrc/post.h): fgmm-global-init-from-accs against numpy in fp64, nnet3-info through the
grep pipeline of sid/init_full_ubm_from_nnet3.sh:91, and the usage and refusal messages of the four tools.  No device is opened."""
import os
import subprocess

import numpy as np
import pytest

import helpers as H
import ubm_ref as R
import ubm_train_ref as T

BIN = os.path.join(H.ROOT, H.PKG_NAME, "bin")
U = 2.0 ** -24
F = np.float32
GREP = "| grep 'output-node' | grep -oP 'dim=\\K[0-9]+'"   # init_full_ubm_from_nnet3.sh:91


def run(args, stdin=None, shell=False):
    env = dict(os.environ, PATH=BIN + os.pathsep + os.environ.get("PATH", ""), HIP_VISIBLE_DEVICES="")
    if not shell:
        args = [os.path.join(BIN, args[0])] + list(args[1:])
    return subprocess.run(args, input=stdin, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, shell=shell, timeout=120)


# ------------------------------------------------------------------------------------------------- fgmm-global-init-from-accs
def known_case(D, G, seed):
    """known means and covariances, and the statistics a Gaussian with exactly those moments leaves: occ, occ mu, occ (C + mu mu').
    C = A A' / D + I has eigenvalues in [1, about 5]: well conditioned."""
    rng = np.random.default_rng(seed)
    occ = rng.uniform(50.0, 500.0, G)
    mu = rng.normal(0.0, 1.0, size=(G, D))
    cs = []
    for _ in range(G):
        a = rng.normal(size=(D, D))
        cs.append(a @ a.T / D + np.eye(D))
    il = np.tril_indices(D)
    mean = occ[:, None] * mu
    cov = np.stack([occ[g] * (cs[g] + np.outer(mu[g], mu[g]))[il] for g in range(G)])
    return occ, mean, cov, mu, cs


def numpy_init(occ, mean, cov, D):
    """the issue's formulas in float64: (weights, inverse covariances [G, D, D], Sigma^-1 mu [G, D])"""
    w = occ / occ.sum()
    inv, lin = [], []
    for g in range(len(occ)):
        mu = mean[g] / occ[g]
        c = R.unpack(cov[g], D) / occ[g] - np.outer(mu, mu)
        inv.append(np.linalg.inv(c))
        lin.append(inv[-1] @ mu)
    return w, np.stack(inv), np.stack(lin)


@pytest.mark.parametrize("D,G,seed", [(5, 3, 1), (17, 4, 2)])
def test_init_from_accs_equals_numpy_in_fp64(tmp_path, D, G, seed):
    occ, mean, cov, mu, cs = known_case(D, G, seed)
    w, inv, lin = numpy_init(occ, mean, cov, D)
    for g in range(G):   # the case is what it says: the covariance comes back, and it is well conditioned
        np.testing.assert_allclose(np.linalg.inv(inv[g]), cs[g], rtol=1e-9, atol=1e-12)
        assert np.linalg.cond(cs[g]) < 20
    il = np.tril_indices(D)
    P = H.pkg()
    got = P.fgmm_init_from_accs(occ, mean, cov)
    assert got["removed"] == [] and got["bad_gconsts"] == 0
    for g in range(G):
        np.testing.assert_allclose(got["inv_covars_f64"][g], inv[g][il], rtol=1e-12, atol=0)
    # the model is the same numbers rounded to float once
    assert np.array_equal(got["inv_covars"], got["inv_covars_f64"].astype(F))
    assert np.all(np.abs(got["weights"] - w) <= U * w)
    assert np.all(np.abs(got["means_invcovars"] - lin) <= U * np.abs(lin).max())
    np.testing.assert_allclose(got["gconsts"], R.full_gconsts(got["weights"], got["means_invcovars"], got["inv_covars"]), rtol=1e-6)
    # the tool reads float32 accumulators: the binding on the same rounded values gives the model's bytes
    for binary in (True, False):
        acc = T.read_accs(T.accs_bytes(occ, mean, cov, 7, binary))
        (tmp_path / "stats.acc").write_bytes(T.accs_bytes(occ, mean, cov, 7, binary))
        r = run(["fgmm-global-init-from-accs", "--verbose=2", "--binary=%s" % str(binary).lower(), str(tmp_path / "stats.acc"), str(G), str(tmp_path / "final.ubm")])
        assert r.returncode == 0, r.stderr
        assert b"0 bad gconsts" in r.stderr and b"Written model to " + str(tmp_path / "final.ubm").encode() in r.stderr
        data = (tmp_path / "final.ubm").read_bytes()
        assert (data[:2] == b"\0B") == binary
        model = R.read_full_gmm(data)
        py = P.fgmm_init_from_accs(acc["occ"].astype(np.float64), acc["mean"].astype(np.float64), acc["cov"].astype(np.float64))
        for name in ("weights", "means_invcovars", "inv_covars"):
            assert np.array_equal(model[name], py[name]), name
        # and float32 statistics move the result by what their rounding allows: a few ulps times the condition number
        assert np.all(np.abs(model["inv_covars"] - got["inv_covars"]) <= 200 * U * np.abs(got["inv_covars"]).max(axis=1, keepdims=True))


def test_a_gaussian_without_occupancy_is_removed_or_named(tmp_path):
    D, G = 5, 4
    occ, mean, cov, _, _ = known_case(D, G, 3)
    occ[2], mean[2], cov[2] = 0.0, 0.0, 0.0
    (tmp_path / "stats.acc").write_bytes(T.accs_bytes(occ, mean, cov, 7, True))
    acc = T.read_accs((tmp_path / "stats.acc").read_bytes())
    r = run(["fgmm-global-init-from-accs", str(tmp_path / "stats.acc"), str(G), str(tmp_path / "final.ubm")])
    assert r.returncode == 0, r.stderr
    assert b"WARNING (fgmm-global-init-from-accs" in r.stderr and b"Removing Gaussian 2: its occupancy is 0" in r.stderr
    model = R.read_full_gmm((tmp_path / "final.ubm").read_bytes())
    keep = [0, 1, 3]
    o = acc["occ"].astype(np.float64)[keep]
    assert model["weights"].shape == (3,) and np.array_equal(model["weights"], (o / o.sum()).astype(F))
    assert abs(float(model["weights"].astype(np.float64).sum()) - 1.0) < 3 * U
    w, inv, lin = numpy_init(o, acc["mean"].astype(np.float64)[keep], acc["cov"].astype(np.float64)[keep], D)
    il = np.tril_indices(D)
    for g in range(3):
        assert np.all(np.abs(model["inv_covars"][g] - inv[g][il]) <= 2 * U * np.abs(inv[g]).max())
    assert np.all(np.isfinite(model["gconsts"]))
    # without the option the same input is an error that names the Gaussian, and nothing is written
    r = run(["fgmm-global-init-from-accs", "--remove-low-count-gaussians=false", str(tmp_path / "stats.acc"), str(G), str(tmp_path / "none.ubm")])
    assert r.returncode == 255 and b"Gaussian 2 cannot be initialised: its occupancy is 0" in r.stderr
    assert not (tmp_path / "none.ubm").exists()
    # a covariance that cannot be inverted is bad in the same way: all the frames of Gaussian 1 on one point
    occ2, mean2, cov2, mu, _ = known_case(D, G, 3)
    il = np.tril_indices(D)
    mean2[1], cov2[1] = occ2[1] * mu[1], occ2[1] * np.outer(mu[1], mu[1])[il]
    got = H.pkg().fgmm_init_from_accs(occ2, mean2, cov2)
    assert got["removed"] == [1] and len(got["weights"]) == 3
    with pytest.raises(H.pkg().XvError, match="Gaussian 1 cannot be initialised: its covariance is not positive definite"):
        H.pkg().fgmm_init_from_accs(occ2, mean2, cov2, remove_low_count_gaussians=False)


def test_init_from_accs_refuses_what_does_not_agree(tmp_path):
    occ, mean, cov, _, _ = known_case(5, 3, 4)
    (tmp_path / "stats.acc").write_bytes(T.accs_bytes(occ, mean, cov, 7, True))
    r = run(["fgmm-global-init-from-accs", str(tmp_path / "stats.acc"), "4", str(tmp_path / "final.ubm")])
    assert r.returncode == 255 and b"the statistics have 3 Gaussians, <num-components> is 4" in r.stderr
    assert not (tmp_path / "final.ubm").exists()
    (tmp_path / "mw.acc").write_bytes(T.accs_bytes(occ, mean, np.zeros_like(cov), 5, True))
    r = run(["fgmm-global-init-from-accs", str(tmp_path / "mw.acc"), "3", "-"])
    assert r.returncode == 255 and b"must carry the means, the covariances and the weights" in r.stderr and r.stdout == b""
    r = run(["fgmm-global-init-from-accs", str(tmp_path / "stats.acc"), "three", "-"])
    assert r.returncode == 255 and b"<num-components> must be a positive integer" in r.stderr
    r = run(["fgmm-global-init-from-accs", "--mix-up=64", str(tmp_path / "stats.acc"), "3", "-"])
    assert r.returncode == 255 and b"--mix-up is not built" in r.stderr
    r = run(["fgmm-global-init-from-accs", str(tmp_path / "stats.acc"), "3"])
    assert r.returncode == 1 and b"Usage: fgmm-global-init-from-accs" in r.stderr
    # fgmm-global-est's other options are taken and change nothing; the recipe's summing pipe is an input
    a = run(["fgmm-global-init-from-accs", str(tmp_path / "stats.acc"), "3", "-"])
    b = run(["fgmm-global-init-from-accs", "--verbose=2", "--min-gaussian-occupancy=1e9", "--variance-floor=10", "--max-condition=1", "--update-flags=w",
             "fgmm-global-sum-accs - %s |" % (tmp_path / "stats.acc"), "3", "-"])
    assert a.returncode == 0 and b.returncode == 0, (a.stderr, b.stderr)
    assert a.stdout == b.stdout and len(a.stdout) > 100 and b"Summed 1 stats" in b.stderr


# ------------------------------------------------------------------------------------------------------------------ nnet3-info
def am_model_file(raw):
    return (b"\x00B<TransitionModel> " + bytes(range(256)) + b"</TransitionModel> " + raw[2:] +
            b"<LeftContext> \x04\x0d\x00\x00\x00<RightContext> \x04\x07\x00\x00\x00<Priors> FV \x04\x00\x00\x00\x00")


@pytest.mark.parametrize("topology", ["v2_xvector", "v3_multitask", "v5_cvector"])
def test_nnet3_info_gives_the_output_dimension_to_the_scripts_grep(tmp_path, topology):
    net, line = H.synth_model(topology)
    (tmp_path / "final.raw").write_bytes(net.to_bytes(True))
    r = run("nnet3-info %s/final.raw" % tmp_path, shell=True)
    assert r.returncode == 0, r.stderr
    text = r.stdout.decode()
    n2 = H.nm.Nnet3.from_bytes(net.to_bytes(True))
    outputs = [H.nm.parse_config_line(l) for l in n2.config_lines]
    outputs = [p[1] for p in outputs if p and p[0] == "output-node"]
    assert outputs
    r = run("nnet3-info %s/final.raw %s" % (tmp_path, GREP), shell=True)
    assert r.returncode == 0, r.stderr
    dims = [int(v) for v in r.stdout.split()]
    assert len(dims) == len(outputs)
    for o, d in zip(outputs, dims):   # every output here is a node of one component: its dimension is that component's
        comp = [H.nm.parse_config_line(l) for l in n2.config_lines]
        node = [p[1] for p in comp if p and p[0] == "component-node" and p[1]["name"] == o["input"]][0]
        c = n2.components[node["component"]]
        want = c.f["linear"].shape[0] if "linear" in c.f else None
        if want is None:   # element-wise: walk to the affine in front
            src = node
            while "linear" not in n2.components[src["component"]].f:
                src = [p[1] for p in comp if p and p[0] == "component-node" and p[1]["name"] == src["input"]][0]
            want = n2.components[src["component"]].f["linear"].shape[0]
        assert d == want
        assert "output-node name=%s input=%s dim=%d objective=linear\n" % (o["name"], o["input"], d) in text
    assert text.startswith("num-parameters: ") and "input-node name=input dim=23\n" in text
    params = sum(c.f["linear"].size + c.f["bias"].size for c in n2.components.values() if "linear" in c.f)
    assert int(text.split()[1]) == params
    n_nodes = sum(1 for l in n2.config_lines if l.startswith("component-node"))
    assert text.count("\ncomponent-node name=") == n_nodes and text.count("input-dim=") >= n_nodes


def test_nnet3_info_on_the_acoustic_model_and_through_the_am_copy_pipe(tmp_path):
    net = H.nm.synthesize([H.config_text("am")], seed=21, head_stddev=1.0)
    raw = net.to_bytes(True)
    (tmp_path / "final.raw").write_bytes(raw)
    (tmp_path / "final.mdl").write_bytes(am_model_file(raw))
    plain = run("nnet3-info %s/final.raw" % tmp_path, shell=True)
    assert plain.returncode == 0, plain.stderr
    assert b"output-node name=output input=output.log-softmax dim=5139 objective=linear\n" in plain.stdout
    assert b"component-node name=tdnn1.affine component=tdnn1.affine input=Append(Offset(input, -2), Offset(input, -1), input, Offset(input, 1), Offset(input, 2)) input-dim=115 output-dim=650\n" in plain.stdout
    assert b"# output: input dim 23, 6 layers, context 13/7, output 5139 per frame\n" in plain.stdout
    nnet_raw = "nnet3-am-copy --raw=true %s/final.mdl - |" % tmp_path   # init_full_ubm_from_nnet3.sh:54
    # :91 as the issue writes it, and as the script writes it: $nnet_raw unquoted, its words arriving one by one
    for form in ('nnet3-info "%s"' % nnet_raw, "nnet_raw='%s'; nnet3-info $nnet_raw" % nnet_raw):
        r = run("%s %s" % (form, GREP), shell=True)
        assert r.returncode == 0, r.stderr
        assert r.stdout == b"5139\n", (form, r.stdout, r.stderr)
    r = run(["nnet3-info", nnet_raw])
    assert r.returncode == 0 and r.stdout == plain.stdout
    r = run(["nnet3-info", "-"], stdin=raw)
    assert r.returncode == 0 and r.stdout == plain.stdout
    r = run(["nnet3-info", str(tmp_path / "final.mdl")])   # a model with its transition model is not a raw network
    assert r.returncode == 255 and b"ERROR (nnet3-info" in r.stderr and r.stdout == b""


# ------------------------------------------------------------------------------------------------------------------ the messages
def test_usage_and_refusals_of_the_four_tools(tmp_path):
    r = run(["nnet3-info"])
    assert r.returncode == 1 and b"Usage: nnet3-info <raw-nnet-rxfilename>" in r.stderr
    r = run(["nnet3-info", "a.raw", "b.raw"])
    assert r.returncode == 1 and b"Usage: nnet3-info" in r.stderr
    r = run(["nnet3-info", "--frobnicate=1", "a.raw"])
    assert r.returncode == 255 and b"frobnicate" in r.stderr
    r = run(["nnet3-info", str(tmp_path / "missing.raw")])
    assert r.returncode == 255 and b"ERROR (nnet3-info" in r.stderr
    r = run(["logprob-to-post", "ark:in.ark"])
    assert r.returncode == 1 and b"Usage: logprob-to-post [options] <logprob-matrix-rspecifier> <posteriors-wspecifier>" in r.stderr
    assert b"--min-post (0.01)" in r.stderr and b"--random-prune (true)" in r.stderr
    r = run(["logprob-to-post", "--min-post=abc", "ark:in.ark", "ark:out.ark"])
    assert r.returncode == 255 and b"--min-post=abc" in r.stderr
    r = run(["logprob-to-post", "--prune=1", "ark:in.ark", "ark:out.ark"])
    assert r.returncode == 255 and b"prune" in r.stderr
    r = run(["fgmm-global-acc-stats-post", "ark:post.ark", "40", "ark:feats.ark"])
    assert r.returncode == 1 and b"Usage: fgmm-global-acc-stats-post [options] <posterior-rspecifier> <number-of-components> <feature-rspecifier> <stats-out>" in r.stderr
    r = run(["fgmm-global-acc-stats-post", "--weights=ark:w.ark", "ark:post.ark", "40", "ark:feats.ark", "x.acc"])
    assert r.returncode == 255 and b"--weights is not built" in r.stderr
    r = run(["fgmm-global-acc-stats-post", "--update-flags=x", "ark:post.ark", "40", "ark:feats.ark", "x.acc"])
    assert r.returncode == 255 and b"Invalid element 'x'" in r.stderr
    r = run(["fgmm-global-acc-stats-post", "ark:post.ark", "0", "ark:feats.ark", "x.acc"])
    assert r.returncode == 255 and b"<num-components> must be a positive integer" in r.stderr
    # the device tools say what they need where there is no GPU (this test runs with none visible); nothing is written
    from oracle import kaldi_io as kio
    kio.write_ark_matrices(str(tmp_path / "lp.ark"), [("utt", np.log(np.full((3, 4), 0.25, F)))])
    r = run(["logprob-to-post", "ark:%s/lp.ark" % tmp_path, "ark:%s/post.ark" % tmp_path])
    assert r.returncode == 255 and b"no HIP device available: logprob-to-post needs a gfx950 GPU (there is no CPU path)" in r.stderr
    # a copy under another name is none of the four
    other = str(tmp_path / "logprob-to-posterior")
    os.symlink(os.path.join(BIN, "logprob-to-post"), other)
    r = subprocess.run([other], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 255 and b"not one of logprob-to-post, fgmm-global-acc-stats-post, fgmm-global-init-from-accs, nnet3-info" in r.stderr
