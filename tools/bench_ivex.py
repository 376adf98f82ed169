#!/usr/bin/env python3
"""Kernel times of i-vector extraction (csrc/ivex_kernels.hip) at the i-vector recipe's size: G = 2048 Gaussians, D = 60, i-vector
dimension 400 or 600, utterances of 500 to 6000 frames with about five posteriors a frame.  Reports, per batch size, the ms of a
launch group and utterances/s (xv_ivex_kernel_time: hipEvent times, the best of --reps runs after one that warms up), how the time
splits between the statistics, the two GEMMs and the solve, the quadratic GEMM's time against the time to read U once at the
measured copy rate of the device (its floor while memory binds it), its fp64 TFLOP/s, and, for context only, the rate of the
float64 numpy restatement on the same machine.  Prints one JSON line."""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ivector_ref as R  # noqa: E402

COPY_RATE = 6.29e12   # bytes/s, the device's measured copy rate


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gauss", type=int, default=2048)
    ap.add_argument("--dim", type=int, default=60)
    ap.add_argument("--ivector-dim", type=int, default=400)
    ap.add_argument("--batches", type=int, nargs="+", default=[16, 64])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--ref-gauss", type=int, default=64)
    a = ap.parse_args()
    P = importlib.import_module("speaker-embedding-with-phonetic-information_amd")
    G, D, S = a.gauss, a.dim, a.ivector_dim
    rng = np.random.default_rng(0)
    M = rng.normal(0.0, 0.05, (G, D, S))
    sig = np.zeros((G, D * (D + 1) // 2))
    r, c = np.tril_indices(D)
    for g in range(G):   # diagonal plus low rank: cheap to make at this size, positive definite, dense
        v = rng.normal(size=(D, 4)) * 0.2
        sig[g] = (np.diag(rng.uniform(0.5, 2.0, D)) + v @ v.T)[r, c]
    t0 = time.perf_counter()
    ie = P.IvectorExtractor(np.full(G, 1.0 / G), M, sig, 2.0)
    create_s = time.perf_counter() - t0
    out = {"gauss": G, "dim": D, "ivector_dim": S, "reps": a.reps, "create_s": create_s, "batches": {}}
    P_tri = S * (S + 1) // 2
    for B in a.batches:
        lens = [int(t) for t in rng.integers(500, 6001, B)]
        feats = [rng.normal(0.0, 1.0, (t, D)).astype(np.float32) for t in lens]
        posts = []
        for t in lens:
            idx = rng.integers(0, G, (t, 5)).astype(np.int32)
            w = rng.dirichlet(np.ones(5), t).astype(np.float32)
            posts.append([(idx[i], w[i]) for i in range(t)])
        ms = ie.kernel_time(feats, posts, reps=a.reps)
        group = ms["stats"] + ms["quadratic"] + ms["linear"] + ms["solve"]
        out["derive_ms"] = ms["derive"]
        out["batches"][str(B)] = {
            "frames": sum(lens), "kernel_ms": {k: ms[k] for k in ("stats", "quadratic", "linear", "solve")}, "group_ms": group,
            "utts_per_s": B / (group * 1e-3),
            "share": {k: ms[k] / group for k in ("stats", "quadratic", "linear", "solve")},
            "quadratic_floor_ms": G * P_tri * 8 / COPY_RATE * 1e3,
            "quadratic_tflops": 2.0 * B * G * P_tri / (ms["quadratic"] * 1e-3) / 1e12,
            "linear_tflops": 2.0 * B * G * D * S / (ms["linear"] * 1e-3) / 1e12}
    # the restatement, for context: terms and solve of one utterance on the first --ref-gauss Gaussians; the terms scale with G
    Gr = min(a.ref_gauss, G)
    sim, U = R.derived(M[:Gr], sig[:Gr])
    gamma, X = rng.uniform(0.0, 3.0, Gr), rng.normal(size=(Gr, D))
    t0 = time.perf_counter()
    l, Q = R.terms(sim, U, gamma, X, 2.0)
    t1 = time.perf_counter()
    np.linalg.solve(Q, l)
    t2 = time.perf_counter()
    out["numpy"] = {"ref_gauss": Gr, "terms_s_scaled_to_G": (t1 - t0) * G / Gr, "solve_s": t2 - t1,
                    "utts_per_s": 1.0 / ((t1 - t0) * G / Gr + (t2 - t1))}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
