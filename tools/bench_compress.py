#!/usr/bin/env python3
"""Times the feature compressor on one device (not called by bench.py): the three kernels of a batch (time between two events,
best of 5 after a warm-up, copies excluded) and the C ABI call including allocation and copies, for 400-frame and 30 000-frame
matrices of 23 columns in batches of 2^18 frames, as copy-feats forms them, methods 1 ("CM" here) and 3 ("CM2").
Bytes = fp32 values read once + object bytes written; the kernels read the values more than once (minimum / maximum, four
selection passes, encode), so the fraction of the HBM peak says how far the whole batch is from one pass over its data.
Writes profiles/compress_bench.json (or the path given) and prints the same JSON line."""
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import helpers as H  # noqa: E402

HBM_PEAK = 8.0e12          # bytes / s, MI355X
BATCH_FRAMES = 1 << 18     # copy-feats' read-ahead bound


def main():
    P = H.pkg()
    L = P.lib()
    commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, text=True).stdout.strip()
    out = {"build": L.xv_version().decode(), "commit": commit or None, "device": None, "hbm_peak_bytes_per_s": HBM_PEAK,
           "what": "gaussian features, 23 columns, batches of 2^18 frames", "cases": {}}
    try:
        import torch
        out["device"] = torch.cuda.get_device_name(0)
    except Exception:
        pass
    rng = np.random.default_rng(0)
    for frames in (400, 30000):
        n = max(1, BATCH_FRAMES // frames)
        base = [(rng.standard_normal((frames, 23)) * np.linspace(1, 20, 23)).astype(np.float32) for _ in range(min(n, 8))]
        mats = [base[i % len(base)] for i in range(n)]
        for method in (1, 3):
            size, fmt = P.compressed_size(frames, 23, method)
            nbytes = n * (frames * 23 * 4 + size)
            ms = P.compress(mats, method=method, kernel_time_reps=5)
            P.compress(mats[:2], method=method)
            t0 = time.perf_counter()
            P.compress(mats, method=method)
            call = time.perf_counter() - t0
            out["cases"]["%d_frames_%s" % (frames, fmt)] = {
                "matrices": n, "frames": n * frames, "bytes": nbytes, "kernel_ms": ms, "kernel_matrices_per_s": n / ms * 1e3,
                "kernel_bytes_per_s": nbytes / ms * 1e3, "fraction_of_hbm_peak": nbytes / ms * 1e3 / HBM_PEAK,
                "abi_call_s": call, "abi_call_matrices_per_s": n / call}
    line = json.dumps(out)
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "compress_bench.json")
    with open(path, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")
    print(line)


if __name__ == "__main__":
    main()
