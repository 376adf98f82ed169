"""ivector-extractor-copy and the final.ie reader and writer behind it, run as binaries on files laid down byte by byte
(tests/ivector_ref.py), the refusals of the two tools, and ivector-extract without a device.  No device is opened."""
import os
import subprocess

import numpy as np
import pytest

import helpers as H
import ivector_ref as R

BIN = os.path.join(H.ROOT, H.PKG_NAME, "bin")
P = H.pkg()


def run(args, stdin=None):
    env = dict(os.environ, PATH=BIN + os.pathsep + os.environ.get("PATH", ""), HIP_VISIBLE_DEVICES="")
    return subprocess.run([os.path.join(BIN, args[0])] + list(args[1:]), input=stdin, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                          env=env, timeout=120)


MODEL = R.random_model(3, 4, 5, 6)


@pytest.mark.parametrize("binary_in", [True, False])
def test_copy_reads_both_flavours_and_writes_the_binary_one_byte_for_byte(tmp_path, binary_in):
    src, dst = tmp_path / "in.ie", tmp_path / "out.ie"
    src.write_bytes(R.ie_bytes(binary=binary_in, **MODEL))
    r = run(["ivector-extractor-copy", str(src), str(dst)])
    assert r.returncode == 0, r.stderr
    assert b"LOG (ivector-extractor-copy" in r.stderr
    assert dst.read_bytes() == R.ie_bytes(binary=True, **MODEL)


def test_binary_to_text_to_binary_gives_identical_bytes(tmp_path):
    data = R.ie_bytes(binary=True, **MODEL)
    r = run(["ivector-extractor-copy", "--binary=false", "-", "-"], stdin=data)
    assert r.returncode == 0, r.stderr
    text = r.stdout
    assert text.startswith(b"<IvectorExtractor> <w>  [ ]\n<w_vec>  [ 0.25 0.25 0.25 0.25 ]\n<M> 4  [\n")
    assert text.rstrip().endswith(b"</IvectorExtractor>")
    # 17 significant digits: every number reads back as the float64 it was
    (tmp_path / "t.ie").write_bytes(text)
    r = run(["ivector-extractor-copy", "cat %s |" % (tmp_path / "t.ie"), "-"])
    assert r.returncode == 0, r.stderr
    assert r.stdout == data
    # and the library reads what the tool wrote
    got = P.ivex_read(str(tmp_path / "t.ie"))
    assert np.array_equal(got["M"], MODEL["M"]) and np.array_equal(got["sigma_inv"], MODEL["sigma_inv"])
    assert np.array_equal(got["w_vec"], MODEL["w_vec"]) and got["prior_offset"] == MODEL["prior_offset"]
    P.ivex_write(str(tmp_path / "w.ie"), binary=True, **MODEL)
    assert (tmp_path / "w.ie").read_bytes() == data


def test_a_model_with_weight_rows_is_refused_by_name(tmp_path):
    for binary in (True, False):
        (tmp_path / "w.ie").write_bytes(R.ie_bytes(binary=binary, w_rows=4, **MODEL))
        for tool, rest in (("ivector-extractor-copy", ["/dev/null"]), ("ivector-extract", ["ark:/dev/null", "ark:/dev/null", "ark:/dev/null"])):
            r = run([tool, str(tmp_path / "w.ie")] + rest)
            assert r.returncode == 255, r.stderr
            assert b"ERROR (" + tool.encode() in r.stderr and b"i-vector-dependent weights" in r.stderr and b"<w>" in r.stderr


def test_spk2utt_is_refused_by_name(tmp_path):
    (tmp_path / "m.ie").write_bytes(R.ie_bytes(**MODEL))
    r = run(["ivector-extract", "--spk2utt=ark:/dev/null", str(tmp_path / "m.ie"), "ark:/dev/null", "ark:/dev/null", "ark:/dev/null"])
    assert r.returncode == 255 and b"--spk2utt is not built" in r.stderr


@pytest.mark.parametrize("binary", [True, False])
def test_truncated_files_and_a_wrong_closing_token_are_errors(tmp_path, binary):
    data = R.ie_bytes(binary=binary, **MODEL)
    for cut in (len(data) // 3, len(data) - 30, len(data) - 3):
        (tmp_path / "cut.ie").write_bytes(data[:cut])
        r = run(["ivector-extractor-copy", str(tmp_path / "cut.ie"), "/dev/null"])
        assert r.returncode == 255 and b"ERROR (ivector-extractor-copy" in r.stderr, (cut, r.stderr)
    (tmp_path / "bad.ie").write_bytes(R.ie_bytes(binary=binary, closing="</IvectorExtractorX>", **MODEL))
    r = run(["ivector-extractor-copy", str(tmp_path / "bad.ie"), "/dev/null"])
    assert r.returncode == 255 and b"expected token </IvectorExtractor>" in r.stderr


def test_ivector_extract_without_a_gpu_is_an_error(tmp_path):
    (tmp_path / "m.ie").write_bytes(R.ie_bytes(**MODEL))
    r = run(["ivector-extract", "--verbose=2", "--num-threads=4", str(tmp_path / "m.ie"), "ark:/dev/null", "ark:/dev/null", "ark:/dev/null"])
    assert r.returncode == 255, r.stderr
    assert b"ERROR (ivector-extract" in r.stderr and b"GPU" in r.stderr


def test_limits_are_errors_that_name_them(tmp_path):
    big = dict(w_vec=np.ones(1), M=np.zeros((1, 1, 1025)), sigma_inv=np.ones((1, 1)), prior_offset=1.0)
    (tmp_path / "big.ie").write_bytes(R.ie_bytes(**big))
    r = run(["ivector-extract", str(tmp_path / "big.ie"), "ark:/dev/null", "ark:/dev/null", "ark:/dev/null"])
    assert r.returncode == 255 and b"limit of 1024" in r.stderr
    wide = dict(w_vec=np.ones(1), M=np.zeros((1, 97, 2)), sigma_inv=np.ones((1, 97 * 98 // 2)), prior_offset=1.0)
    (tmp_path / "wide.ie").write_bytes(R.ie_bytes(**wide))
    r = run(["ivector-extract", str(tmp_path / "wide.ie"), "ark:/dev/null", "ark:/dev/null", "ark:/dev/null"])
    assert r.returncode == 255 and b"limit of 96" in r.stderr
