#!/usr/bin/env python3
"""Times the PLDA back-end on one device at SRE16 scale (not called by bench.py): the scatter statistics of 100 k x 512
training rows in 10 k speakers, the PLDA transform of 802 enrolment + 9 294 test rows at dim 150, the scoring of 2 M
random trials, and the host cost of the scoring tool (trial parse, device call, score printing) from its own timing line.
Then score normalisation's all-pairs workload (--asnorm-only: nothing else): the top-300 statistics of 9 294 x 2 272 and of
100 000 x 10 000 pairs at dim 150 through xv_plda_cohort_stats, and the same pairs as a trial list through xv_plda_score.
Device times are kernel times between two events (minimum of 3 after one warm-up).  Prints one JSON line."""
import json
import os
import re
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import helpers as H  # noqa: E402
import plda_ref as R  # noqa: E402
from oracle import kaldi_io as kio  # noqa: E402


def best(f, reps=3):
    f()
    ms, wall = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        ms.append(f())
        wall.append(time.perf_counter() - t0)
    return min(ms), min(wall) * 1e3


# v_mfma_f64_16x16x4_f64 on 256 CUs: AMD's published FP64 matrix figure for the MI355X (the microarchitecture guide's MFMA
# table lists no fp64 row of its own)
PEAK_FP64_MATRIX_TFLOPS = 78.6
TRIAL_LIST_MAX = 50 * 1000 * 1000   # a longer list of all pairs (8 bytes of indices and 8 of score each, through host buffers) is not sent


def all_pairs(P, rng, rows, cols, dim=150, top_n=300):
    """device_ms of the top-N statistics of rows x cols pairs on the dense path, and of the same pairs as a trial list"""
    psi = np.sort(rng.uniform(0, 5, dim))[::-1]
    u = rng.standard_normal((rows, dim), dtype=np.float32)
    v = rng.standard_normal((cols, dim), dtype=np.float32)
    num = rng.integers(1, 9, rows).astype(np.float64)
    ms, wall = best(lambda: P.asnorm.plda_cohort_stats(u, num, v, psi, top_n, return_ms=True)[2])
    rpc, n_chunks, _ = P.asnorm.plda_dense_plan(rows, cols, dim)
    flop = 2.0 * rows * cols * 2 * dim
    r = {"rows": rows, "cols": cols, "dim": dim, "top_n": top_n, "chunks": n_chunks, "rows_per_chunk": rpc,
         "cohort_stats_device_ms": ms, "cohort_stats_host_call_ms": wall, "pairs_per_s_dense": rows * cols / ms * 1e3,
         "tflops_fp64": flop / ms / 1e9, "peak_fp64_matrix_tflops": PEAK_FP64_MATRIX_TFLOPS,
         "fraction_of_peak": flop / ms / 1e9 / PEAK_FP64_MATRIX_TFLOPS}
    if rows * cols <= TRIAL_LIST_MAX:
        tr = np.stack(np.meshgrid(np.arange(rows, dtype=np.int32), np.arange(cols, dtype=np.int32), indexing="ij"), -1).reshape(-1, 2)
        ms_t, wall_t = best(lambda: P.plda_score(u, num, v, psi, tr, return_ms=True)[1])
        r.update(trial_list_device_ms=ms_t, trial_list_host_call_ms=wall_t, trials_per_s_list=rows * cols / ms_t * 1e3,
                 trial_list_over_dense=ms_t / ms)
    else:
        r["trial_list"] = "not sent: %d trials are more than TRIAL_LIST_MAX = %d" % (rows * cols, TRIAL_LIST_MAX)
    return r


def main():
    P = H.pkg()
    rng = np.random.default_rng(0)
    out = {}
    if "--asnorm-only" in sys.argv[1:]:
        out["all_pairs"] = [all_pairs(P, rng, 9294, 2272), all_pairs(P, rng, 100000, 10000)]
        print(json.dumps(out))
        return
    # scatter: 100 k x 512, speakers of 10 rows
    n, d = 100000, 512
    x = rng.standard_normal((n, d), dtype=np.float32)
    segs = [list(range(i, min(i + 10, n))) for i in range(0, n, 10)]
    ms, wall = best(lambda: P.scatter_stats(x, segs, return_ms=True)[3])
    out["scatter"] = {"rows": n, "dim": d, "speakers": len(segs), "device_ms": ms, "host_call_ms": wall,
                      "gflops_fp64": 2.0 * n * d * d / 2 / ms / 1e6}
    # transform: 802 + 9294 rows at dim 150
    dim, n_u, n_v = 150, 802, 9294
    mean = rng.standard_normal(dim)
    t = np.linalg.qr(rng.standard_normal((dim, dim)))[0]
    psi = np.sort(rng.uniform(0, 5, dim))[::-1]
    xs = rng.standard_normal((n_u + n_v, dim), dtype=np.float32)
    ms, wall = best(lambda: P.plda_transform(xs, t, -(t @ mean), psi, return_ms=True)[2])
    out["transform"] = {"rows": n_u + n_v, "dim": dim, "device_ms": ms, "host_call_ms": wall}
    # scoring: 2 M random trials
    n_tr = 2000000
    u = rng.standard_normal((n_u, dim), dtype=np.float32)
    v = rng.standard_normal((n_v, dim), dtype=np.float32)
    num = rng.integers(1, 9, n_u).astype(np.float64)
    tr = np.stack([rng.integers(0, n_u, n_tr), rng.integers(0, n_v, n_tr)], 1).astype(np.int32)
    ms, wall = best(lambda: P.plda_score(u, num, v, psi, tr, return_ms=True)[1])
    s = P.plda_score(u, num, v, psi, tr[:1000])
    ref = np.array([R.llr(u[a], num[a], v[b], psi) for a, b in tr[:1000]])
    out["score"] = {"trials": n_tr, "enrolment": n_u, "test": n_v, "dim": dim, "device_ms": ms, "host_call_ms": wall,
                    "trials_per_s_device": n_tr / ms * 1e3, "max_abs_err_vs_oracle_1k": float(np.abs(s - ref).max())}
    # the scoring tool on the same sizes: its own timing line splits parse / device / print
    with tempfile.TemporaryDirectory() as d:
        R.write_plda(os.path.join(d, "plda"), mean, t, psi)
        kio.write_ark_vectors(os.path.join(d, "enr.ark"), [("s%04d" % i, u[i]) for i in range(n_u)])
        kio.write_ark_vectors(os.path.join(d, "test.ark"), [("t%05d" % i, v[i]) for i in range(n_v)])
        with open(os.path.join(d, "trials"), "w") as f:
            f.write("".join("s%04d t%05d\n" % (a, b) for a, b in tr))
        t0 = time.perf_counter()
        r = subprocess.run([os.path.join(P.BIN_DIR, "ivector-plda-scoring"), os.path.join(d, "plda"), "ark:%s/enr.ark" % d,
                            "ark:%s/test.ark" % d, os.path.join(d, "trials"), os.path.join(d, "scores")],
                           stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
        wall = time.perf_counter() - t0
        err = r.stderr.decode()
        m = re.search(r"Timing: trials read in ([0-9.e+-]+) s, scored on the device in ([0-9.e+-]+) s, written in ([0-9.e+-]+) s", err)
        out["scoring_tool"] = {"exit": r.returncode, "trials": n_tr, "wall_s": wall,
                               "parse_s": float(m.group(1)) if m else None, "device_call_s": float(m.group(2)) if m else None,
                               "print_s": float(m.group(3)) if m else None}
    out["all_pairs"] = [all_pairs(P, rng, 9294, 2272), all_pairs(P, rng, 100000, 10000)]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
