"""CPU tests of the host half of adaptive score normalisation: the plan that cuts a score matrix into row chunks of a bounded
device workspace (xv_plda_dense_plan: pure, through the library without a device), the argument checks of the device entries
that come before any device call, and the early exits of ivector-plda-scoring-asnorm (usage, options, argument counts) in the
style of tests/test_cli_transcripts.py.  No GPU is needed or looked for."""
import os
import re
import subprocess

import numpy as np
import pytest

import helpers as H

BIN = os.path.join(H.ROOT, H.PKG_NAME, "bin")
TOOL = os.path.join(BIN, "ivector-plda-scoring-asnorm")
_HDR = open(os.path.join(H.ROOT, H.PKG_NAME, "csrc", "plda_dense_kernels.h")).read()
TILE_M = int(re.search(r"\bkDenseTileM = (\d+)\b", _HDR).group(1))
_MAX = re.search(r"\bkTopnMaxCols = (\d+) << (\d+);", _HDR)
MAX_COLS = int(_MAX.group(1)) << int(_MAX.group(2))
GRID_ROWS = 65535 * TILE_M   # what one launch's grid covers


def _chunks(rows, rpc, n):
    return [(c * rpc, min(rows, (c + 1) * rpc)) for c in range(n)]


def test_no_rows_make_no_chunks_and_one_row_makes_one():
    P = H.pkg()
    assert P.asnorm.plda_dense_plan(0, 100, 150, 1 << 20)[1:] == (0, 0)
    rpc, n, nbytes = P.asnorm.plda_dense_plan(1, 100, 150, 1 << 20)
    assert (n, nbytes) == (1, 100 * 8) and rpc == (1 << 20) // 800 // TILE_M * TILE_M
    assert P.asnorm.plda_dense_plan(1, 100, 150, 800) == (1, 1, 800)          # a workspace of exactly one row


@pytest.mark.parametrize("cols,cap", [(100, 1 << 20), (2272, 1 << 24), (10000, 256 << 20), (7, 7 * 8 * 5), (3, 3 * 8 * (TILE_M + 9))])
def test_rows_below_at_and_above_a_chunk(cols, cap):
    P = H.pkg()
    fit = cap // (cols * 8)
    want = fit // TILE_M * TILE_M if fit >= TILE_M else fit            # whole tiles of the scoring kernel where one fits
    for rows, n_want in ((want - 1, 1), (want, 1), (want + 1, 2), (3 * want, 3), (3 * want + 1, 4)):
        if rows < 1:
            continue
        rpc, n, nbytes = P.asnorm.plda_dense_plan(rows, cols, 150, cap)
        assert (rpc, n) == (want, n_want) and nbytes == min(rows, want) * cols * 8 <= cap, (rows, rpc, n, nbytes)


def test_the_chunks_cover_every_row_once_and_in_order():
    P = H.pkg()
    rng = np.random.default_rng(0)
    for _ in range(200):
        rows, cols = int(rng.integers(0, 100000)), int(rng.integers(1, 20000))
        cap = cols * 8 * int(rng.integers(1, 4000)) + int(rng.integers(0, 8))
        rpc, n, nbytes = P.asnorm.plda_dense_plan(rows, cols, int(rng.integers(1, 513)), cap)
        spans = _chunks(rows, rpc, n)
        assert [b for _, b in spans[:-1]] == [a for a, _ in spans[1:]] and all(0 < b - a <= rpc for a, b in spans)
        assert (spans[0][0], spans[-1][1]) == (0, rows) if rows else not spans
        assert rpc * cols * 8 <= cap and nbytes == min(rows, rpc) * cols * 8
        assert rpc % TILE_M == 0 or rpc < TILE_M


def test_a_chunk_is_never_more_than_one_launch_covers_and_the_default_workspace():
    P = H.pkg()
    assert P.asnorm.plda_dense_plan(10 ** 8, 2, 1, 1 << 40)[:2] == (GRID_ROWS, -(-10 ** 8 // GRID_ROWS))
    assert P.asnorm.plda_dense_plan(100000, 10000, 150) == P.asnorm.plda_dense_plan(100000, 10000, 150, 256 << 20)
    assert P.asnorm.plda_dense_plan(100000, 10000, 150)[:2] == (3328, 31)


def test_a_workspace_too_small_for_one_row_and_other_bad_arguments_are_refused():
    P = H.pkg()
    with pytest.raises(P.XvError, match="does not hold one row of 100 scores") as e:
        P.asnorm.plda_dense_plan(5, 100, 150, 799)
    assert e.value.status == P.XV_ERR_ARG
    for args in ((-1, 100, 150, 1 << 20), (5, 0, 150, 1 << 20), (5, 100, 0, 1 << 20), (5, 100, 513, 1 << 20), (1 << 31, 100, 150, 1 << 20)):
        with pytest.raises(P.XvError) as e:
            P.asnorm.plda_dense_plan(*args)
        assert e.value.status == P.XV_ERR_ARG, args


def test_sizes_out_of_range_are_argument_errors_before_any_device_call():
    """XV_ERR_ARG, not XV_ERR_DEVICE: the same with or without a GPU."""
    P = H.pkg()
    x = np.zeros((2, 4))
    u, v, psi = np.zeros((3, 5), np.float32), np.zeros((4, 5), np.float32), np.ones(5)
    calls = [lambda: P.asnorm.topn_stats(x, 1), lambda: P.asnorm.topn_stats(x, 5), lambda: P.asnorm.topn_stats(np.zeros((1, 1)), 2),
             lambda: P.asnorm.plda_cohort_stats(u, np.ones(3), v, psi, 1), lambda: P.asnorm.plda_cohort_stats(u, np.ones(3), v, psi, 5),
             lambda: P.asnorm.plda_cohort_stats(u, np.ones(3), v, psi, 4, by_column=True),
             lambda: P.asnorm.plda_score_dense(u, np.zeros(3), v, psi),
             lambda: P.asnorm.plda_score_dense(np.zeros((1, 513), np.float32), np.ones(1), np.zeros((1, 513), np.float32), np.ones(513))]
    for i, call in enumerate(calls):
        with pytest.raises(P.XvError) as e:
            call()
        assert e.value.status == P.XV_ERR_ARG, i
    # the limit on the columns is refused by its name (no matrix of that width is needed to ask)
    assert P.lib().xv_topn_stats(0, None, 0, MAX_COLS + 1, 2, None, None, None) == P.XV_ERR_ARG
    assert ("more than kTopnMaxCols = %d" % MAX_COLS).encode() in P.lib().xv_last_error()


# ------------------------------------------------------------------------------------------------ the tool's early exits
def _tool(*args, cwd=None):
    env = {k: v for k, v in os.environ.items() if k != "XVEC_DEVICE"}
    env.update(HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="")
    r = subprocess.run([TOOL] + list(args), cwd=cwd, env=env, stdin=subprocess.DEVNULL, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       timeout=120)
    return r.returncode, r.stdout.decode(), r.stderr.decode()


def _usage():
    rc, out, err = _tool("--help")
    assert rc == 0 and out == ""
    return err


def test_the_usage_names_the_six_arguments_and_every_option():
    usage = _usage()
    assert "Usage: ivector-plda-scoring-asnorm [options] <plda> <train-ivector-rspecifier> <test-ivector-rspecifier>\n" in usage
    assert "<cohort-ivector-rspecifier> <trials-rxfilename> <scores-wxfilename>\n" in usage
    for opt in ("--num-utts=<rspecifier>", "--normalize-length=true", "--simple-length-normalization=false", "--top-n=300",
                "--train-stats=<wxfilename>", "--test-stats=<wxfilename>"):
        assert opt in usage, opt


@pytest.mark.parametrize("n_args", [0, 1, 5, 7])
def test_a_wrong_number_of_arguments_prints_the_usage_and_exits_1(n_args, tmp_path):
    args = ["a%d" % i for i in range(n_args)]
    rc, out, err = _tool(*args, cwd=str(tmp_path))
    assert rc == 1 and out == "" and err.endswith(_usage()) and not os.listdir(str(tmp_path))


@pytest.mark.parametrize("option,message", [
    ("--top-n=1", "ERROR (ivector-plda-scoring-asnorm) --top-n=1 is out of range: the statistics need at least two scores\n"),
    ("--top-n=0", "ERROR (ivector-plda-scoring-asnorm) --top-n=0 is out of range: the statistics need at least two scores\n"),
    ("--top-n=-3", "ERROR (ivector-plda-scoring-asnorm) --top-n=-3 is out of range: the statistics need at least two scores\n"),
    ("--top-n=many", "ERROR (ivector-plda-scoring-asnorm) Invalid value for option --top-n=many\n"),
    ("--top-n=2.5", "ERROR (ivector-plda-scoring-asnorm) Invalid value for option --top-n=2.5\n"),
    ("--normalize-length=perhaps", "ERROR (ivector-plda-scoring-asnorm) Invalid value for option --normalize-length=perhaps\n"),
])
def test_a_bad_option_value_exits_255_and_writes_nothing(option, message, tmp_path):
    rc, out, err = _tool(option, "plda", "ark:train", "ark:test", "ark:cohort", "trials", "scores", cwd=str(tmp_path))
    echo = "ivector-plda-scoring-asnorm %s plda ark:train ark:test ark:cohort trials scores \n" % option   # once the options are read
    assert (rc, out) == (255, "") and err in (message, echo + message) and not os.listdir(str(tmp_path))


@pytest.mark.parametrize("option", ["--dim=3", "--smoothing=0.1", "--top_n=3", "--cohort=x"])
def test_an_option_of_a_sibling_is_an_unknown_one(option, tmp_path):
    rc, out, err = _tool(option, "plda", "ark:train", "ark:test", "ark:cohort", "trials", "scores", cwd=str(tmp_path))
    assert rc == 255 and out == "" and err == "ERROR (ivector-plda-scoring-asnorm) Invalid option %s\n\n%s" % (option, _usage())
    assert not os.listdir(str(tmp_path))


def test_the_sibling_does_not_take_the_new_options():
    r = subprocess.run([os.path.join(BIN, "ivector-plda-scoring"), "--top-n=3", "a", "b", "c", "d", "e"], stdin=subprocess.DEVNULL,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert r.returncode == 255 and r.stderr.decode().startswith("ERROR (ivector-plda-scoring) Invalid option --top-n=3\n")


# ------------------------------------------------------------------------------------------------ the companion header
def test_the_table_of_the_companion_header_matches_its_prototypes():
    """include/xvec_hip_asnorm.h against _abi.ASNORM_SIGNATURES, as tests/test_abi_table.py holds the main table to xvec_hip.h."""
    import importlib

    import test_abi_table as T
    P = H.pkg()
    table = importlib.import_module(P.__name__ + "._abi").ASNORM_SIGNATURES
    text = open(os.path.join(H.ROOT, "include", "xvec_hip_asnorm.h")).read()
    text = re.sub(r"//[^\n]*", " ", re.sub(r"/\*.*?\*/", " ", text, flags=re.S))
    protos = re.findall(r"\b((?:const\s+)?\w+\s*\**)\s*\b(xv_\w+)\s*\(([^)]*)\)\s*;", text)
    assert [name for _, name, _ in protos] == list(table) == ["xv_plda_score_dense", "xv_topn_stats", "xv_plda_cohort_stats",
                                                              "xv_plda_dense_plan"]
    assert not set(table) & set(P.ABI_SYMBOLS) and all(hasattr(P.lib(), name) for name in table)
    for ret, name, params in protos:
        restype, argtypes = table[name]
        params = [p.strip() for p in params.split(",")]
        assert restype is T.RETURNS[" ".join(ret.split())] and len(argtypes) == len(params), name
        for decl, py in zip(params, argtypes):
            base, stars = T._declaration(decl)
            assert T._pointer_matches(py, base, stars) if stars else py is T.SCALARS[base], (name, decl, py)
    for name in ("plda_score_dense", "topn_stats", "plda_cohort_stats", "plda_dense_plan"):
        assert callable(getattr(P.asnorm, name)) and not hasattr(P, name)
