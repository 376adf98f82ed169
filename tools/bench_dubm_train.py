#!/usr/bin/env python3
"""Kernel times of the two E-steps of diagonal UBM training (csrc/dubm_train_kernels.hip) at the i-vector recipe's size: G = 2048
Gaussians, D = 60, 2^18 frames.  The dense E-step of gmm-global-init-from-feats is one call over all the frames; the sparse one of
gmm-global-acc-stats (n = 30) goes through as the tool sends it, in blocks of kDgmmAccFrameBlock frames, and the blocks are summed.
Every launch group is timed through xv_dgmm_acc_kernel_time (hipEvent times, the best of --reps runs after one that warms up).  Next
to the times go computed floors: the fp32 FMA count of the scores, the fp64 MFMA flops of the dense accumulation, the bytes.  For
context, the time of ubm_diag_gselect on the same frames: it computes the same dense scores once, plus a top-n.  Nothing is compared
with an earlier number: there is none.  Prints one JSON line."""
import argparse
import ctypes
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
FP64_MFMA_FLOPS = 78.6e12            # the fp64 matrix rate of AMD's MI355X product specification
FP32_VALU_FLOPS = 157.3e12           # the fp32 vector rate of the same specification (an FMA is 2 flops)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1 << 18)
    ap.add_argument("--gauss", type=int, default=2048)
    ap.add_argument("--dim", type=int, default=60)
    ap.add_argument("--n", type=int, default=30)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    P = importlib.import_module("speaker-embedding-with-phonetic-information_amd")
    hdr = open(os.path.join(ROOT, "speaker-embedding-with-phonetic-information_amd", "csrc", "dubm_train_kernels.h")).read()
    block = int(re.search(r"kDgmmAccFrameBlock = (\d+);", hdr).group(1))
    G, D, n, T = a.gauss, a.dim, a.n, a.frames
    rng = np.random.default_rng(0)
    means = rng.normal(size=(G, D))
    iv = rng.uniform(0.5, 2.0, size=(G, D)).astype(np.float32)
    mi = (means * iv).astype(np.float32)
    gc = R.diag_gconsts(np.full(G, 1.0 / G), mi, iv).astype(np.float32)
    diag = P.Ubm.diag(gc, mi, iv)
    x = R.frames_around(1, means, T)
    # the selection kernel on all frames, n as in the recipe, timed by xv_ubm_gselect's own events
    L = P.lib()
    off = np.array([0, T], np.int32)
    idx = np.zeros((T, n), np.int32)
    best = None
    for r in range(a.reps + 1):
        ms = ctypes.c_float()
        assert L.xv_ubm_gselect(diag._h, x.ctypes.data, off.ctypes.data, 1, n, idx.ctypes.data, None, ctypes.byref(ms)) == 0
        if r >= 1:
            best = ms.value if best is None else min(best, ms.value)
    acc = P.DgmmAccumulator(G, D, "mvw")
    dense = acc.kernel_time(diag, x, None, dense=True, reps=a.reps)
    sparse = {"sort": 0.0, "scores": 0.0, "softmax": 0.0, "acc": 0.0}
    for r0 in range(0, T, block):
        t = acc.kernel_time(diag, x[r0:r0 + block], idx[r0:r0 + block], dense=False, reps=a.reps)
        for k in sparse:
            sparse[k] += t[k]
    cols = 2 * D + 1
    col_tiles = (cols + 15) // 16
    score_fma = T * G * 2 * D                       # one pass over all (frame, Gaussian) scores
    mfma_flops = T * ((G + 15) // 16 * 16) * col_tiles * 16 * 2
    dense_bytes = T * D * 4 * ((G + 63) // 64)      # every Gaussian tile of dgmm_dense_acc reads the frames once (from L2 or HBM)
    out = {"frames": T, "gauss": G, "dim": D, "n": n, "reps": a.reps, "frame_block": block,
           "dense_kernel_ms": {k: dense[k] for k in ("dense_logsum", "dense_acc", "dense_reduce")},
           "sparse_kernel_ms": sparse, "ubm_diag_gselect_ms": best,
           "floors_ms": {"scores_one_pass_fp32_fma": 2 * score_fma / FP32_VALU_FLOPS * 1e3,
                         "dense_acc_fp64_mfma": mfma_flops / FP64_MFMA_FLOPS * 1e3,
                         "dense_acc_frame_bytes_hbm_spec": dense_bytes / HBM_SPEC_BYTES_PER_S * 1e3},
           "counts": {"score_fma_per_pass": score_fma, "dense_acc_mfma_flops": mfma_flops, "dense_acc_frame_bytes": dense_bytes}}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
