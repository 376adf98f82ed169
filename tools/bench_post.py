#!/usr/bin/env python3
"""Times the logprob-to-post kernels on one device (not called by bench.py): the count pass, the scan and the write pass of one
launch, each the time between two events around its launch, best of 5 after a warm-up, copies to and from the host excluded.
The shape is one utterance of 16384 frames by 6000 columns (a senone network's output; 393 MB, far more than the caches hold) whose
rows are log-softmax outputs of gaussian scores with a standard deviation of 4: a few large posteriors and a long tail per frame.
Beside the kernel pair goes its floor: both passes read the input once, and two reads cost what a device-to-device copy of the
input costs (one read, one write) at the copy bandwidth of the same run.  Two smaller launches (8192 and 2048 rows: 197 and 49 MB,
which the memory-side cache holds) show what a smaller grid costs and what the cache gives the second pass.
Writes profiles/logprob_post_bench.json (or the path given) and prints the same JSON line."""
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

COLS = 6000
SHAPES = (16384, 8192, 2048)
MIN_POST = 0.01


def logprobs(rows, cols, seed=0):
    rng = np.random.default_rng(seed)
    base = rng.normal(0.0, 4.0, size=(256, cols))
    base -= np.log(np.exp(base).sum(axis=1, keepdims=True))
    return np.ascontiguousarray(np.tile(base.astype(np.float32), (rows // 256, 1)))


def main():
    P = H.pkg()
    L = P.lib()
    commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, text=True).stdout.strip()
    digest = hashlib.sha256()
    for name in ("post_kernels.hip", "post_kernels.h", "counter_rng.h", "post.cc"):
        digest.update(open(os.path.join(ROOT, H.PKG_NAME, "csrc", name), "rb").read())
    out = {"build": L.xv_version().decode(), "commit": commit or None, "post_sources_sha256": digest.hexdigest()[:16], "device": None,
           "what": "log-softmax of N(0, 4^2) scores, %d columns, min_post %g" % (COLS, MIN_POST), "cases": {}}
    try:
        import torch
        prop = torch.cuda.get_device_properties(0)
        out["device"] = "%s (%s, %d CUs)" % (prop.name, prop.gcnArchName.split(":")[0], prop.multi_processor_count)
    except Exception:
        pass
    for rows in SHAPES:
        x = logprobs(rows, COLS)
        nbytes = x.size * 4
        post, details = P.logprob_to_post([x], ["bench"], MIN_POST, True, frame_budget=rows, return_details=True)
        pairs = sum(len(i) for i, _ in post[0])
        case = {"rows": rows, "cols": COLS, "input_bytes": nbytes, "pairs": pairs, "pairs_per_frame": pairs / rows}
        for prune in (True, False):
            ms = P.logprob_to_post_kernel_time(x, "bench", MIN_POST, prune, reps=5)
            pair_ms = ms["count"] + ms["write"]
            case["random_prune_%s" % str(prune).lower()] = {
                "count_ms": ms["count"], "scan_ms": ms["scan"], "write_ms": ms["write"], "count_plus_write_ms": pair_ms,
                "copy_ms": ms["copy"], "copy_bytes_per_s": 2 * nbytes / ms["copy"] * 1e3,
                "floor_ms_two_reads_at_copy_bandwidth": ms["copy"], "kernel_pair_over_floor": pair_ms / ms["copy"],
                "kernel_pair_read_bytes_per_s": 2 * nbytes / pair_ms * 1e3}
        out["cases"]["%dx%d" % (rows, COLS)] = case
    line = json.dumps(out)
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "logprob_post_bench.json")
    with open(path, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")
    print(line)


if __name__ == "__main__":
    main()
