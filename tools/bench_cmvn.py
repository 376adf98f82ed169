#!/usr/bin/env python3
"""Times the per-speaker CMVN kernels on one device (not called by bench.py): cmvn_stats (block partials + their reduction) and
cmvn_apply, each the time between two events around its launches, best of 5 after a warm-up, copies excluded.  Two shapes: 23 and
40 columns, batches of 2^18 frames in 400-frame matrices, as the tools read them ahead.
Bytes: cmvn_stats reads every fp32 value once (its partial sums are 1/128 of that); cmvn_apply reads and writes every value once.
The fraction is of the HBM rate the microarchitecture notes give for the MI355X (8 TB/s).
Writes profiles/cmvn_bench.json (or the path given) and prints the same JSON line."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import helpers as H  # noqa: E402

HBM_PEAK = 8.0e12          # bytes / s, MI355X
BATCH_FRAMES = 1 << 18
FRAMES = 400


def main():
    P = H.pkg()
    L = P.lib()
    commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, text=True).stdout.strip()
    # the tree the numbers belong to: the commit where there is one, and in any case a digest of the sources that were timed
    digest = hashlib.sha256()
    for name in ("cmvn_kernels.hip", "cmvn_kernels.h", "cmvn.cc"):
        digest.update(open(os.path.join(ROOT, H.PKG_NAME, "csrc", name), "rb").read())
    out = {"build": L.xv_version().decode(), "commit": commit or None, "cmvn_sources_sha256": digest.hexdigest()[:16], "device": None,
           "hbm_peak_bytes_per_s": HBM_PEAK,
           "what": "gaussian features around 50, 400-frame matrices, batches of 2^18 frames", "cases": {}}
    try:
        import torch
        prop = torch.cuda.get_device_properties(0)
        out["device"] = "%s (%s, %d CUs)" % (prop.name, prop.gcnArchName.split(":")[0], prop.multi_processor_count)
    except Exception:
        pass
    rng = np.random.default_rng(0)
    for cols in (23, 40):
        n = BATCH_FRAMES // FRAMES
        base = [rng.normal(50.0, 1.0, size=(FRAMES, cols)).astype(np.float32) for _ in range(8)]
        mats = [base[i % len(base)] for i in range(n)]
        values = n * FRAMES * cols * 4
        stats_ms, apply_ms = P.cmvn_stats(mats, kernel_time_reps=5)
        case = {"matrices": n, "frames": n * FRAMES}
        for name, ms, nbytes in (("cmvn_stats", stats_ms, values), ("cmvn_apply", apply_ms, 2 * values)):
            case[name] = {"bytes": nbytes, "kernel_ms": ms, "kernel_bytes_per_s": nbytes / ms * 1e3,
                          "fraction_of_hbm_peak": nbytes / ms * 1e3 / HBM_PEAK}
        out["cases"]["%d_columns" % cols] = case
    line = json.dumps(out)
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "cmvn_bench.json")
    with open(path, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")
    print(line)


if __name__ == "__main__":
    main()
