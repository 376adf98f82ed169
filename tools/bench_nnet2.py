#!/usr/bin/env python3
"""Times nnet-am-compute on one device (not called by bench.py), at the dimensions of local/dnn/run_nnet2_multisplice.sh: 40-dim input,
the four splices, six hidden p-norm layers 3500 -> 350, 10500 outputs mixed down to 5000, random weights.

Device: the time of every layer (the kernel that prepares its input and its affine) and of the head, between events, the smallest
of 3 calls after a warm-up, on one utterance of FRAMES frames.  Beside each time its two floors: the three fp16 MFMA passes of the
layer's product at 2.5 PFLOP/s (the dense fp16 peak), and the bytes the layer moves through HBM - planes in, weights, pre-activations
out and in again, planes out - at 6.3 TB/s (what a copy reaches).
Command line: the wall rate of bin/nnet-am-compute --apply-log=true writing to /dev/null, and the rate of the same bytes through a pipe
(cat of the tool's output into a reader that discards it).
Writes profiles/nnet2_bench.md (or the path given)."""
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import helpers as H  # noqa: E402
import nnet2_ref as R  # noqa: E402
from oracle import kaldi_io as kio  # noqa: E402

FRAMES = 4000
MFMA_PEAK = 2.5e15
HBM_RATE = 6.3e12


def layer_shapes(comps):
    """(context size, K per offset, N, width after the nonlinearity) of every affine"""
    out, n_ctx = [], 1
    for c in comps:
        if c[0] == "Splice":
            n_ctx = len(c[2])
        elif c[0] in R.AFFINE:
            w = np.asarray(c[1])
            out.append([n_ctx, w.shape[1] // n_ctx, w.shape[0], w.shape[0]])
            n_ctx = 1
        elif c[0] == "Pnorm":
            out[-1][3] = c[2]
    return out


def main():
    P = H.pkg()
    rng = np.random.default_rng(0)
    comps = R.multisplice(rng, 40, 200, 3500, 350, 10500, R.random_sizes(rng, 10500, 5000), extra_hidden=1, final_std=0.3)
    d = tempfile.mkdtemp(prefix="nnet2_bench")
    model = R.write_model(os.path.join(d, "final.mdl"), comps, ())
    net = P.nnet2.Nnet2(model)
    x = rng.normal(size=(FRAMES, 40)).astype(np.float32)
    rows = FRAMES + 22
    best = None
    for rep in range(4):
        _, ms = net.compute([x], apply_log=True, layers=True)
        if rep:
            best = ms if best is None else np.minimum(best, ms)
    lines = ["# nnet-am-compute at the recipe's dimensions", "",
             "`python tools/bench_nnet2.py` on one MI355X (%s).  One utterance of %d frames (%d rows with its padding), one block;" % (
                 P.lib().xv_version().decode(), FRAMES, rows),
             "device time between events, the smallest of 3 calls after a warm-up.  MFMA floor: three fp16 passes of the product at",
             "2.5 PFLOP/s.  HBM floor: planes in, weights, pre-activations out and in, planes out, at 6.3 TB/s.", "",
             "| stage | shape (offsets x K -> N) | device ms | MFMA floor ms | HBM floor ms | time / larger floor |", "|---|---|---|---|---|---|"]
    shapes = layer_shapes(comps)
    total_floor = 0.0
    for i, (n_ctx, k, n, width) in enumerate(shapes):
        k_pad, n_pad = -(-k // 32) * 32, -(-n // 128) * 128
        flops = 3 * 2.0 * rows * n_ctx * k_pad * n_pad
        nbytes = rows * k_pad * 4 + n_pad * n_ctx * k_pad * 4 + 2 * rows * n * 4 + (rows * (-(-width // 32) * 32) * 4 if i + 1 < len(shapes) else 0)
        f1, f2 = flops / MFMA_PEAK * 1e3, nbytes / HBM_RATE * 1e3
        total_floor += max(f1, f2)
        lines.append("| layer %d | %d x %d -> %d | %.3f | %.3f | %.3f | %.1f |" % (i, n_ctx, k, n, best[i], f1, f2, best[i] / max(f1, f2)))
    head_bytes = rows * 10500 * 4 + FRAMES * 5000 * 4
    lines.append("| head | 10500 -> 5000 | %.3f | - | %.3f | %.1f |" % (best[-1], head_bytes / HBM_RATE * 1e3, best[-1] / (head_bytes / HBM_RATE * 1e3)))
    lines.append("| all | | %.3f | | %.3f | %.1f |" % (best.sum(), total_floor + head_bytes / HBM_RATE * 1e3, best.sum() / (total_floor + head_bytes / HBM_RATE * 1e3)))
    lines += ["", "%.0f frames per second of device time." % (FRAMES / best.sum() * 1e3), ""]
    # the command line
    utts = [("utt%04d" % i, rng.normal(size=(FRAMES // 4, 40)).astype(np.float32)) for i in range(16)]
    kio.write_ark_matrices(os.path.join(d, "feats.ark"), utts)
    frames = sum(len(u) for _, u in utts)
    tool = os.path.join(P.BIN_DIR, "nnet-am-compute")
    cmd = "timeout -k 10 300 %s --use-gpu=yes --apply-log=true --chunk-size=256 %s ark:%s/feats.ark " % (tool, model, d)
    walls = {}
    for name, sink in (("/dev/null", "ark:/dev/null"), ("a file", "ark:%s/out.ark" % d), ("a pipe", "ark:- | cat > /dev/null")):
        t = []
        for _ in range(3):
            t0 = time.perf_counter()
            r = subprocess.run(["/bin/sh", "-c", cmd + sink], stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, timeout=400)
            t.append(time.perf_counter() - t0)
            assert r.returncode == 0, r.stderr.decode()[-2000:]
        walls[name] = min(t)
    out_bytes = os.path.getsize(os.path.join(d, "out.ark"))
    t = []
    for _ in range(3):
        t0 = time.perf_counter()
        subprocess.run(["/bin/sh", "-c", "cat %s/out.ark | cat > /dev/null" % d], check=True, timeout=400)
        t.append(time.perf_counter() - t0)
    pipe_s = min(t)
    lines += ["## The command line", "",
              "`nnet-am-compute --use-gpu=yes --apply-log=true --chunk-size=256 final.mdl ark:feats.ark <sink>`: 16 utterances of %d frames" % (FRAMES // 4),
              "(%d frames, %.1f MB of log-posteriors, %.1f KB per frame), the smallest wall time of 3 runs, the model's load (%.0f MB) and" % (
                  frames, out_bytes / 1e6, out_bytes / frames / 1e3, os.path.getsize(model) / 1e6),
              "the start of the device included.", "", "| sink | wall s | frames / s |", "|---|---|---|"]
    for name, w in walls.items():
        lines.append("| %s | %.2f | %.0f |" % (name, w, frames / w))
    lines += ["", "The same %.1f MB through `cat out.ark | cat > /dev/null`: %.3f s, %.0f frames / s (%.2f GB/s)." % (out_bytes / 1e6, pipe_s, frames / pipe_s,
                                                                                                                        out_bytes / pipe_s / 1e9), ""]
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "nnet2_bench.md")
    with open(path, "w") as f:
        f.write("\n".join(lines))
    print("\n".join(lines))
    shutil.rmtree(d, ignore_errors=True)


if __name__ == "__main__":
    main()
