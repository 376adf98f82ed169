#!/usr/bin/env python3
"""Kernel rates of the GMM-UBM stage (csrc/ubm_kernels.hip) at the i-vector recipe's size: G = 2048 Gaussians, D = 60, n = 20, on a
batch of about 10^5 frames.  Reports frames/s of every kernel (xv_ubm_kernel_time: hipEvent times, the best of --reps runs
after one that warms up), the share of the fp32 FMA peak the two scoring kernels reach, and, for context only, the rate of the
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
import ubm_ref as R  # noqa: E402

# The MI355X's fp32 vector peak as specified, 157.3 TFLOP/s = 78.6e12 fused multiply-adds per second.  That figure is the rate of
# the packed form (v_pk_fma_f32, two per lane) and of the fp32 matrix instructions; plain v_fma_f32, which is what these
# kernels issue, peaks at half of it.  The shares below are of the specified peak.
PEAK_FMA = 157.3e12 / 2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=100000)
    ap.add_argument("--gauss", type=int, default=2048)
    ap.add_argument("--dim", type=int, default=60)
    ap.add_argument("--n", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--ref-frames", type=int, default=2000)
    a = ap.parse_args()
    P = importlib.import_module("speaker-embedding-with-phonetic-information_amd")
    G, D, n = a.gauss, a.dim, a.n
    rng = np.random.default_rng(0)
    # diagonal-plus-low-rank inverse covariances: cheap to make at this size, positive definite, dense
    w = np.full(G, 1.0 / G, np.float32)
    means = rng.normal(size=(G, D))
    ic = np.zeros((G, D * (D + 1) // 2), np.float32)
    b = np.zeros((G, D), np.float32)
    for g in range(G):
        v = rng.normal(size=(D, 4)) * 0.2
        inv = np.diag(rng.uniform(0.5, 2.0, D)) + v @ v.T
        ic[g] = R.pack(inv)
        b[g] = inv @ means[g]
    gc_d, mi, iv = P.fgmm_to_gmm(w, b, ic)
    diag = P.Ubm.diag(gc_d, mi, iv)
    full = P.Ubm.full(R.full_gconsts(w, b, ic).astype(np.float32), b, ic)
    lens = []
    while sum(lens) < a.frames:
        lens.append(int(rng.integers(500, 6000)))
    feats = [R.frames_around(i, means, t).astype(np.float32) for i, t in enumerate(lens)]
    T = sum(lens)
    ms = P.ubm_kernel_time(diag, full, feats, n=n, min_post=0.025, reps=a.reps)
    out = {"frames": T, "gauss": G, "dim": D, "n": n, "reps": a.reps, "kernel_ms": ms,
           "frames_per_s": {k: (T / (v * 1e-3) if v > 0 else None) for k, v in ms.items()},
           "fma_peak_share": {"gselect": T * G * 2 * D / (ms["gselect"] * 1e-3) / PEAK_FMA,
                              "full": T * n * (D * D + 2 * D) / (ms["full"] * 1e-3) / PEAK_FMA}}
    x = np.concatenate(feats)[:a.ref_frames]
    t0 = time.perf_counter()
    ll = R.diag_loglikes(x, gc_d, mi, iv)
    sel = R.gselect(ll, n)
    t1 = time.perf_counter()
    R.posteriors(R.full_loglikes(x, R.full_gconsts(w, b, ic), b, ic, sel), 0.025)
    t2 = time.perf_counter()
    out["numpy_frames_per_s"] = {"gselect": len(x) / (t1 - t0), "post": len(x) / (t2 - t1)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
