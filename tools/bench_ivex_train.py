#!/usr/bin/env python3
"""Kernel times of i-vector extractor training (csrc/ivex_train_kernels.hip) at the i-vector recipe's size: G = 2048 Gaussians,
D = 60, i-vector dimension 400, 64 utterances of about 3000 frames with about five posteriors a frame.  Reports the ms of the
posterior kernel and of the two rank updates of one flush of 64 utterances (xv_ivex_acc_kernel_time: hipEvent times, the best of
--reps runs after one that warms up) beside their floors (R: 2 G P 8 bytes read and written at the device's measured copy rate, and
2 * 64 G P flops at the highest fp64 matrix rate this project has measured), and the time of one launch group of plain extraction
on the same inputs (xv_ivex_kernel_time), and the wall time of accumulate() without and with the second-order statistics.  --est times ivector-extractor-est's M-step alone (host only, no GPU) on synthetic
statistics of the same shape with --est-threads threads.  Prints one JSON line."""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

COPY_RATE = 6.29e12    # bytes/s, the device's measured copy rate
FP64_RATE = 5.21e12    # flop/s, the quadratic GEMM of profiles/ivex_bench.md at B = 16: the best fp64 MFMA rate measured here


def posterior_threads():
    """the workgroup size of the posterior kernel that was built (csrc/ivex_train_kernels.h)"""
    import re
    with open(os.path.join(ROOT, "speaker-embedding-with-phonetic-information_amd", "csrc", "ivex_train_kernels.h")) as f:
        return int(re.search(r"kIvexPosteriorThreads = (\d+);", f.read()).group(1))


def model(rng, G, D, S):
    M = rng.normal(0.0, 0.05, (G, D, S))
    sig = np.zeros((G, D * (D + 1) // 2))
    r, c = np.tril_indices(D)
    for g in range(G):   # diagonal plus low rank: cheap to make at this size, positive definite, dense
        v = rng.normal(size=(D, 4)) * 0.2
        sig[g] = (np.diag(rng.uniform(0.5, 2.0, D)) + v @ v.T)[r, c]
    return np.full(G, 1.0 / G), M, sig


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gauss", type=int, default=2048)
    ap.add_argument("--dim", type=int, default=60)
    ap.add_argument("--ivector-dim", type=int, default=400)
    ap.add_argument("--utts", type=int, default=64)
    ap.add_argument("--frames", type=int, default=3000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--est", action="store_true")
    ap.add_argument("--est-threads", type=int, default=16)
    a = ap.parse_args()
    P = importlib.import_module("speaker-embedding-with-phonetic-information_amd")
    G, D, S = a.gauss, a.dim, a.ivector_dim
    Pt = S * (S + 1) // 2
    rng = np.random.default_rng(0)
    w_vec, M, sig = model(rng, G, D, S)
    out = {"gauss": G, "dim": D, "ivector_dim": S}
    if a.est:
        st = dict(num_ivectors=5000.0, auxf=0.0, frames=0.0, gamma=rng.uniform(3000.0, 9000.0, G), S=np.zeros((G, D * (D + 1) // 2)),
                  ivector_sum=np.zeros(S), ivector_scatter=np.zeros(Pt))
        r, c = np.tril_indices(S)
        R = np.zeros((G, Pt))
        base = rng.normal(size=(S, S))
        base = base @ base.T / S + np.eye(S)
        for g in range(G):
            R[g] = st["gamma"][g] * (base[r, c] + (r == c) * rng.uniform(0.0, 0.5))
        st["R"] = R
        st["Y"] = np.einsum("gds,st->gdt", M, base) * st["gamma"][:, None, None] + rng.normal(0.0, 1.0, (G, D, S))
        rd, cd = np.tril_indices(D)
        for g in range(G):
            v = rng.normal(size=(D, D))
            st["S"][g] = st["gamma"][g] * (v @ v.T / D + 2.0 * np.eye(D))[rd, cd] + (M[g] @ base @ M[g].T * st["gamma"][g])[rd, cd]
        mu = np.zeros(S)
        mu[0] = 100.0
        st["ivector_sum"] = 5000.0 * mu
        st["ivector_scatter"] = (5000.0 * (base / 4 + np.outer(mu, mu)))[r, c]
        st["frames"] = float(st["gamma"].sum())
        t0 = time.perf_counter()
        res = P.ivex_est(st, w_vec, M, sig, 100.0, num_threads=a.est_threads)
        out["est"] = {"threads": a.est_threads, "wall_s": time.perf_counter() - t0, "gauss_updated": res["gauss_updated"],
                      "eig_floored": res["eig_floored"], "var_floored": res["var_floored"]}
        print(json.dumps(out))
        return
    ie = P.IvectorExtractor(w_vec, M, sig, 2.0)
    lens = [int(t) for t in rng.integers(a.frames - 500, a.frames + 501, a.utts)]
    feats = [rng.normal(0.0, 1.0, (t, D)).astype(np.float32) for t in lens]
    posts = []
    for t in lens:
        idx = rng.integers(0, G, (t, 5)).astype(np.int32)
        w = rng.dirichlet(np.ones(5), t).astype(np.float32)
        posts.append([(idx[i], w[i]) for i in range(t)])
    ex = ie.kernel_time(feats, posts, reps=a.reps)
    acc = P.IvexAccumulator(ie, update_variances=False)
    ms = acc.kernel_time(feats, posts, reps=a.reps)
    acc.close()
    # what the second-order statistics add (the recipe's default): wall time of accumulate(), the packing of the Python lists and
    # the uploads included, without and with --update-variances; the best of --reps calls after one that warms up
    wall = {}
    for var in (False, True):
        acc = P.IvexAccumulator(ie, update_variances=var)
        best = None
        for r in range(a.reps + 1):
            t0 = time.perf_counter()
            acc.accumulate(feats, posts)
            dt = (time.perf_counter() - t0) * 1e3
            best = dt if r == 1 or (r > 1 and dt < best) else best
        acc.close()
        wall[str(var).lower()] = best
    B = a.utts
    out.update({
        "utts": B, "frames": sum(lens), "reps": a.reps, "kernel_ms": ms, "posterior_threads": posterior_threads(),
        "accumulate_wall_ms": {"update_variances_false": wall["false"], "update_variances_true": wall["true"]},
        "extract_group_ms": ex["stats"] + ex["quadratic"] + ex["linear"] + ex["solve"], "extract_kernel_ms": {k: ex[k] for k in ("stats", "quadratic", "linear", "solve")},
        "rank_update_R": {"bytes_floor_ms": 2.0 * G * Pt * 8 / COPY_RATE * 1e3, "flops_floor_ms": 2.0 * B * G * Pt / FP64_RATE * 1e3,
                          "tflops": 2.0 * B * G * Pt / (ms["rank_update_R"] * 1e-3) / 1e12,
                          "tbytes_per_s": 2.0 * G * Pt * 8 / (ms["rank_update_R"] * 1e-3) / 1e12},
        "rank_update_Y": {"bytes_floor_ms": 2.0 * G * D * S * 8 / COPY_RATE * 1e3, "flops_floor_ms": 2.0 * B * G * D * S / FP64_RATE * 1e3,
                          "tflops": 2.0 * B * G * D * S / (ms["rank_update_Y"] * 1e-3) / 1e12},
        "posterior": {"flops": B * 2.0 * S ** 3 / 3, "gflops": B * 2.0 * S ** 3 / 3 / (ms["posterior"] * 1e-3) / 1e9}})
    print(json.dumps(out))


if __name__ == "__main__":
    main()
