#!/usr/bin/env python3
"""Kernel times of the E-step of full-covariance UBM training (csrc/ubm_train_kernels.hip) at the i-vector recipe's size: G = 2048
Gaussians, D = 60, n = 20, 2^18 frames, which fgmm-global-acc-stats cuts into blocks of kFgmmAccFrameBlock frames.  Every block is
timed through xv_fgmm_acc_kernel_time (hipEvent times, the best of --reps runs after one that warms up) and the blocks are summed.
Next to the times go two computed floors of fgmm_acc: its bytes at the HBM rate and its fp64 MFMA flops at the peak.  Nothing is
compared with an earlier number: there is none.  Prints one JSON line."""
import argparse
import importlib
import json
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ubm_ref as R  # noqa: E402

HBM_SPEC_BYTES_PER_S = 8.0e12        # the MI355X's HBM3E rate as specified
HBM_COPY_BYTES_PER_S = 6.29e12       # what a float4 copy kernel reaches on it (79 % of the specification)
FP64_MFMA_FLOPS = 78.6e12            # the fp64 matrix rate of AMD's MI355X product specification (256 CUs at 2.4 GHz, 128 per CU and clock)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1 << 18)
    ap.add_argument("--gauss", type=int, default=2048)
    ap.add_argument("--dim", type=int, default=60)
    ap.add_argument("--n", type=int, default=20)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    P = importlib.import_module("speaker-embedding-with-phonetic-information_amd")
    hdr = open(os.path.join(ROOT, "speaker-embedding-with-phonetic-information_amd", "csrc", "ubm_train_kernels.h")).read()
    block = int(re.search(r"kFgmmAccFrameBlock = (\d+);", hdr).group(1))
    G, D, n, T = a.gauss, a.dim, a.n, a.frames
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
    full = P.Ubm.full(P.fgmm_gconsts(w, b, ic), b, ic)
    x = R.frames_around(1, means, T)
    sel = diag.gselect([x], n)[0]
    acc = P.FgmmAccumulator(G, D, "mvw")
    ms = {"sort": 0.0, "full": 0.0, "softmax": 0.0, "acc": 0.0}
    touched = 0
    for r0 in range(0, T, block):
        t = acc.kernel_time(full, x[r0:r0 + block], sel[r0:r0 + block], reps=a.reps)
        for k in ms:
            ms[k] += t[k]
        touched += len(np.unique(sel[r0:r0 + block]))
    pairs = T * n
    tri = D * (D + 1) // 2
    tiles = ((D + 15) // 16) * ((D + 15) // 16 + 1) // 2
    # gathered: a frame row, a sorted index and a posterior per pair.  accumulated: per call and Gaussian that was hit, the partial
    # sums written and read once (buckets longer than a chunk: once per chunk, not counted) and the accumulators read and written
    bytes_acc = pairs * (D * 4 + 8) + touched * (1 + D + tri) * 8 * 4
    flops = pairs * tiles * 16 * 16 * 2
    out = {"frames": T, "gauss": G, "dim": D, "n": n, "reps": a.reps, "frame_block": block, "calls": (T + block - 1) // block, "kernel_ms": ms,
           "frames_per_s": {k: T / (v * 1e-3) for k, v in ms.items() if v > 0},
           "acc_floor_ms": {"hbm_spec": bytes_acc / HBM_SPEC_BYTES_PER_S * 1e3, "hbm_copy": bytes_acc / HBM_COPY_BYTES_PER_S * 1e3,
                            "fp64_mfma": flops / FP64_MFMA_FLOPS * 1e3},
           "acc_bytes": bytes_acc, "acc_mfma_flops": flops}
    out["acc_over_floor"] = {k: ms["acc"] / v for k, v in out["acc_floor_ms"].items()}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
