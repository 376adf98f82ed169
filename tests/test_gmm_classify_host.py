"""The host-only tools of the GMM classifiers through real command lines on tiny tables: compute-vad-from-frame-likes, merge-vads,
fgmm-global-info, and the scalar-float table (what fgmm-global-get-frame-likes --average=true writes) read back by scale-post.
No GPU: none of these opens a device."""
import os
import subprocess

import numpy as np

import gmm_classify_ref as C
import helpers as H
import ubm_ref as R
from oracle import kaldi_io as kio

BIN = os.path.join(H.ROOT, H.PKG_NAME, "bin")

SPEECH = {"utt1": [-1.0, -5.0, -2.0, -2.0], "utt2": [-1.0, -1.0], "utt3": [0.0], "utt4": [-3.0, -3.0, -3.0]}
NOISE = {"utt1": [-2.0, -1.0, -2.0, -2.5], "utt2": [-4.0, 0.0], "utt4": [-1.0, -1.0]}              # utt3 is missing, utt4 is short
MUSIC = {"utt1": [-3.0, -4.0, -2.0, -2.25], "utt2": [-2.5, -0.5], "utt3": [1.0], "utt4": [0.0, 0.0, 0.0]}


def _sh(line, cwd=None):
    env = dict(os.environ, PATH=BIN + os.pathsep + os.environ.get("PATH", ""))
    return subprocess.run(["/bin/sh", "-c", line], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, cwd=cwd, timeout=120)


def _likes(tmp_path):
    for name, table, binary in (("speech", SPEECH, True), ("noise", NOISE, False), ("music", MUSIC, True)):
        items = [(k, np.array(v, np.float32)) for k, v in sorted(table.items())]
        kio.write_ark_vectors(str(tmp_path / (name + ".ark")), items, binary=binary)
    return "ark:%s/speech.ark ark,t:%s/noise.ark ark:%s/music.ark" % (tmp_path, tmp_path, tmp_path)


def _vectors(data):
    return [(k, v.tolist()) for k, v in C.read_vector_table(data)]


def test_the_built_tools_are_there():
    for name in ("fgmm-gselect", "fgmm-global-get-frame-likes", "compute-vad-from-frame-likes", "merge-vads", "fgmm-global-info"):
        assert os.access(os.path.join(BIN, name), os.X_OK), name


def test_vad_from_frame_likes_command_line(tmp_path):
    tables = _likes(tmp_path)
    both = ("utt1", "utt2")
    # the script's argv with its defaults (compute_vad_decision_gmm.sh:117): an empty --map and an empty --priors
    r = _sh("compute-vad-from-frame-likes --map= --priors= %s ark,scp:%s/vad.ark,%s/vad.scp" % (tables, tmp_path, tmp_path))
    assert r.returncode == 0, r.stderr
    assert b"utt3" in r.stderr and b"utt4" in r.stderr and b"Done 2 files; 2 with errors." in r.stderr
    got = _vectors((tmp_path / "vad.ark").read_bytes())
    want = [(k, C.vad_from_frame_likes([SPEECH[k], NOISE[k], MUSIC[k]]).tolist()) for k in both]
    assert got == want
    assert got[0][1] == [0.0, 1.0, 0.0, 0.0], "the three-way tie of utt1's frame 2 goes to the lowest index"
    assert [l.split()[0] for l in (tmp_path / "vad.scp").read_text().splitlines()] == list(both)
    # priors that flip decisions, and a map that renames the classes
    (tmp_path / "map").write_text("0 1\n1 0\n2 2\n")
    r = _sh("compute-vad-from-frame-likes --map=%s/map --priors=0.1,0.1,0.8 %s ark,t:-" % (tmp_path, tables))
    assert r.returncode == 0, r.stderr
    got = _vectors(r.stdout)
    assert got == [(k, C.vad_from_frame_likes([SPEECH[k], NOISE[k], MUSIC[k]], [0.1, 0.1, 0.8], [1, 0, 2]).tolist()) for k in both]
    assert got[0][1] == [2.0, 0.0, 2.0, 2.0]
    # one table alone: every frame is class 0
    r = _sh("compute-vad-from-frame-likes ark:%s/speech.ark ark,t:-" % tmp_path)
    assert r.returncode == 0 and [v for _, v in _vectors(r.stdout)] == [[0.0] * len(SPEECH[k]) for k in sorted(SPEECH)]
    # what is fatal
    r = _sh("compute-vad-from-frame-likes --priors=0.5,0.5 %s ark:/dev/null" % tables)
    assert r.returncode == 255 and b"--priors has 2 entries for 3 tables" in r.stderr
    r = _sh("compute-vad-from-frame-likes --priors=0.5,0,0.5 %s ark:/dev/null" % tables)
    assert r.returncode == 255 and b"must be positive" in r.stderr
    (tmp_path / "short_map").write_text("0 1\n2 2\n")
    r = _sh("compute-vad-from-frame-likes --map=%s/short_map %s ark:/dev/null" % (tmp_path, tables))
    assert r.returncode == 255 and b"no line for index 1" in r.stderr
    r = _sh("compute-vad-from-frame-likes ark:/dev/null")
    assert r.returncode == 1 and b"Usage: compute-vad-from-frame-likes" in r.stderr


def test_merge_vads_command_line(tmp_path):
    energy = {"utt1": [1, 1, 0, 0, 1], "utt2": [1, 0], "utt3": [1], "utt4": [0, 1]}
    gmm = {"utt1": [1, 0, 1, 2, 2], "utt2": [2, 2], "utt4": [1]}   # utt3 is missing, utt4 is short
    for name, table in (("energy", energy), ("gmm", gmm)):
        kio.write_ark_vectors(str(tmp_path / (name + ".ark")), [(k, np.array(v, np.float32)) for k, v in sorted(table.items())],
                              scp_path=str(tmp_path / (name + ".scp")))
    # without a map: 1 iff both are 1 (class 2 counts as not speech)
    r = _sh("merge-vads scp:%s/energy.scp scp:%s/gmm.scp ark,t:-" % (tmp_path, tmp_path))
    assert r.returncode == 0, r.stderr
    assert _vectors(r.stdout) == [("utt1", [1.0, 0.0, 0.0, 0.0, 0.0]), ("utt2", [0.0, 0.0])]
    assert b"utt3" in r.stderr and b"utt4" in r.stderr and b"Done 2 files; 2 with errors." in r.stderr
    # the script's line (compute_vad_decision_gmm.sh:124-126) with a map that keeps music (2) where the energy VAD says 1
    triples = [(0, 0, 0), (0, 1, 0), (0, 2, 0), (1, 0, 0), (1, 1, 1), (1, 2, 2)]
    (tmp_path / "merge_map").write_text("".join("%d %d %d\n" % t for t in triples))
    r = _sh("merge-vads --map=%s/merge_map scp:%s/energy.scp scp:%s/gmm.scp ark,scp:%s/merged.ark,%s/merged.scp"
            % (tmp_path, tmp_path, tmp_path, tmp_path, tmp_path))
    assert r.returncode == 0, r.stderr
    got = _vectors((tmp_path / "merged.ark").read_bytes())
    assert got == [(k, C.merge_vads(energy[k], gmm[k], triples).tolist()) for k in ("utt1", "utt2")]
    assert got == [("utt1", [1.0, 0.0, 0.0, 0.0, 2.0]), ("utt2", [2.0, 0.0])]
    # a pair without a line is fatal and named
    (tmp_path / "holes").write_text("".join("%d %d %d\n" % t for t in triples[:-1]))
    r = _sh("merge-vads --map=%s/holes scp:%s/energy.scp scp:%s/gmm.scp ark:/dev/null" % (tmp_path, tmp_path, tmp_path))
    assert r.returncode == 255 and b"no entry for the pair (1, 2)" in r.stderr
    (tmp_path / "bad").write_text("0 0\n")
    r = _sh("merge-vads --map=%s/bad scp:%s/energy.scp scp:%s/gmm.scp ark:/dev/null" % (tmp_path, tmp_path, tmp_path))
    assert r.returncode == 255 and b"does not have 3 integers" in r.stderr


def test_fgmm_global_info_prints_what_gender_id_greps(tmp_path):
    w, _, b, ic = R.random_full_model(3, 7, 5)
    for binary in (True, False):
        (tmp_path / "final.ubm").write_bytes(R.full_gmm_bytes(w, b, ic, binary))
        r = _sh("fgmm-global-info --print-args=false %s/final.ubm" % tmp_path)
        assert r.returncode == 0, r.stderr
        assert r.stdout.decode().splitlines() == ["number of gaussians 7", "feature dimension 5"]
        # gender_id.sh:68
        r = _sh("fgmm-global-info --print-args=false %s/final.ubm | grep gaussians | awk '{print $NF}'" % tmp_path)
        assert r.stdout.strip() == b"7"
    r = _sh("fgmm-global-info %s/nothing.ubm" % tmp_path)
    assert r.returncode == 255


def test_a_float_table_is_read_back_by_scale_post(tmp_path):
    """The table's two forms as TableWriter::WriteFloat writes them (the restatement's bytes), through scale-post's per-utterance
    scales: ReadFloatTable reads both."""
    post = [("utt1", [[(3, 0.5), (7, 0.5)], [(1, 1.0)]]), ("utt2", [[(2, 0.25), (4, 0.75)]])]
    scales = [("utt1", np.float32(0.5)), ("utt2", np.float32(-71.25))]
    (tmp_path / "post.ark").write_bytes(R.post_table_bytes(post, True))
    for binary in (True, False):
        (tmp_path / "scales.ark").write_bytes(C.float_table_bytes(scales, binary))
        r = _sh("scale-post ark:%s/post.ark ark:%s/scales.ark ark,t:-" % (tmp_path, tmp_path))
        assert r.returncode == 0, r.stderr
        got = R.read_post_table(r.stdout)
        assert got == [(k, R.scale_post(p, float(s))) for (k, p), (_, s) in zip(post, scales)]
