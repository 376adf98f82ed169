#!/usr/bin/env python3
"""End-to-end wall time of bin/nnet3-compute on the acoustic-model path (file in, file out; start-up, PCIe and Kaldi I/O included),
in the style of bench_cli.py: a synthetic split data directory - stored "CM" features behind a feats.scp, spk2utt / utt2spk,
per-speaker cmvn.scp - and the feature string of sid/nnet3_cvector/am/extract_bn.sh:59, timed

  fused      as the tool runs it by default: the pipeline is recognised and run on the device (csrc/fuse_pipe.h)
  commands   under XVEC_DEBUG=fuse_pipe=0: apply-cmvn is a child process that writes floats into a pipe
  plain      on an "ark:" file of the same features, already normalised (floats): the table loop alone
  parent     with --parent-bin=<nnet3-compute of another build>: the plain job with that binary, for an A/B of the loop

each --reps times (default 5), the variants alternating inside every repetition.  Prints one JSON line: per variant the wall
times, their median, and the spread (max - min) over the repetitions; and whether fused and commands wrote the same bytes.

  tools/bench_compute_cli.py [utterances=3000] [frames=400] [--reps=5] [--parent-bin=PATH] [--variants=fused,commands,plain,parent]
                             [--keep=DIR] [--batch-frames=N]
"""
import hashlib
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import cmvn_ref as R  # noqa: E402
import helpers as H  # noqa: E402
from oracle import kaldi_io as kio  # noqa: E402

BIN = os.path.join(ROOT, H.PKG_NAME, "bin")
POOL = 64             # distinct utterances; the table repeats them
UTTS_PER_SPEAKER = 8


def opt(name, default):
    return ([a.split("=", 1)[1] for a in sys.argv[1:] if a.startswith("--%s=" % name)] or [default])[0]


def write_data(d, n, frames):
    import io
    import struct
    pool = [H.features(2000 + i, frames) + np.float32(2.0 * (i % 5)) for i in range(POOL)]
    stored, expanded = [], []
    for m in pool:
        b = io.BytesIO()
        kio.write_compressed_matrix(b, m, "CM")
        stored.append(b.getvalue())
        expanded.append(next(iter(kio.read_ark(io.BytesIO(b"k \0B" + b.getvalue()))))[1])
    n_spk = (n + UTTS_PER_SPEAKER - 1) // UTTS_PER_SPEAKER
    spk_of = lambda i: "spk%06d" % (i // UTTS_PER_SPEAKER)
    key_of = lambda i: "%s-utt%07d" % (spk_of(i), i)
    # per-speaker statistics of the stored values, and the features normalised with them (cmvn_ref: what apply-cmvn computes)
    pool_stats = [R.stats(m) for m in expanded]
    norms = []
    with open(os.path.join(d, "cmvn.ark"), "wb") as f, open(os.path.join(d, "cmvn.scp"), "w") as g:
        for s in range(n_spk):
            st = sum(pool_stats[i % POOL] for i in range(s * UTTS_PER_SPEAKER, min(n, (s + 1) * UTTS_PER_SPEAKER)))
            norms.append(R.cmvn_norm(st))
            f.write(("spk%06d " % s).encode())
            g.write("spk%06d %s/cmvn.ark:%d\n" % (s, d, f.tell()))
            f.write(b"\0BDM \x04" + struct.pack("<i", 2) + b"\x04" + struct.pack("<i", st.shape[1]) + st.astype("<f8").tobytes())
    with open(os.path.join(d, "feats.ark"), "wb") as f, open(os.path.join(d, "feats.scp"), "w") as g, \
            open(os.path.join(d, "normed.ark"), "wb") as h, open(os.path.join(d, "utt2spk"), "w") as u:
        for i in range(n):
            k = key_of(i)
            f.write((k + " ").encode())
            g.write("%s %s/feats.ark:%d\n" % (k, d, f.tell()))
            f.write(b"\0B" + stored[i % POOL])
            u.write("%s %s\n" % (k, spk_of(i)))
            h.write((k + " ").encode() + b"\0B")
            kio.write_matrix(h, R.apply(expanded[i % POOL], norms[i // UTTS_PER_SPEAKER]))
    net = H.nm.synthesize([H.config_text("am")], seed=21, head_stddev=1.0)
    open(os.path.join(d, "am.raw"), "wb").write(net.to_bytes(True))


def run(binary, d, feats, env_extra, batch_frames):
    out = os.path.join(d, "out.ark")
    cmd = [binary, "--use-gpu=yes", "--output-node=tdnn5.batchnorm"] + (["--batch-frames=%s" % batch_frames] if batch_frames else []) + [
        os.path.join(d, "am.raw"), feats, "ark:" + out]
    env = dict(os.environ, PATH=BIN + os.pathsep + os.environ.get("PATH", ""))
    env.pop("XVEC_DEBUG", None)
    env.update(env_extra)
    t0 = time.perf_counter()
    r = subprocess.run(cmd, stderr=subprocess.PIPE, stdout=subprocess.PIPE, env=env)
    wall = time.perf_counter() - t0
    err = r.stderr.decode()
    m = re.search(r"Time taken ([0-9.e+-]+)s", err)
    sha = None
    if os.path.exists(out):
        hsh = hashlib.sha1()
        with open(out, "rb") as f:
            for block in iter(lambda: f.read(1 << 24), b""):
                hsh.update(block)
        sha = hsh.hexdigest()
        os.remove(out)
    return {"rc": r.returncode, "wall_s": wall, "loop_s": float(m.group(1)) if m else None, "sha1": sha,
            "recognised": "feature pipeline recognised" in err, "done": (re.findall(r"Done \d+ utterances, failed for \d+", err) or [None])[-1]}


def main():
    pos = [a for a in sys.argv[1:] if not a.startswith("--")]
    n = int(pos[0]) if pos else 3000
    frames = int(pos[1]) if len(pos) > 1 else 400
    reps = int(opt("reps", "5"))
    parent = opt("parent-bin", "")
    variants = opt("variants", "fused,commands,plain" + (",parent" if parent else "")).split(",")
    keep = opt("keep", "")
    batch_frames = opt("batch-frames", "")
    d = keep or tempfile.mkdtemp(prefix="xvcompute", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
    os.makedirs(d, exist_ok=True)
    write_data(d, n, frames)
    bn = "ark,s,cs:apply-cmvn  --utt2spk=ark:%s/utt2spk scp:%s/cmvn.scp scp:%s/feats.scp ark:- |" % (d, d, d)
    plain = "ark:%s/normed.ark" % d
    binary = os.path.join(BIN, "nnet3-compute")
    how = {"fused": (binary, bn, {}), "commands": (binary, bn, {"XVEC_DEBUG": "fuse_pipe=0"}), "plain": (binary, plain, {}),
           "parent": (parent, plain, {})}
    runs = {v: [] for v in variants}
    for _ in range(reps):
        for v in variants:
            b, feats, env = how[v]
            runs[v].append(run(b, d, feats, env, batch_frames))
    res = {"utts": n, "frames": frames, "reps": reps, "feature_MB_stored": n * frames * 23 / 1e6, "variants": {}}
    for v in variants:
        w = sorted(x["wall_s"] for x in runs[v])
        loops = sorted(x["loop_s"] for x in runs[v] if x["loop_s"] is not None)
        res["variants"][v] = {"wall_s": [round(x["wall_s"], 4) for x in runs[v]], "median_wall_s": round(w[len(w) // 2], 4),
                              "spread_wall_s": round(w[-1] - w[0], 4), "median_loop_s": round(loops[len(loops) // 2], 4) if loops else None,
                              "rc": sorted({x["rc"] for x in runs[v]}), "recognised": sorted({x["recognised"] for x in runs[v]}),
                              "done": sorted({str(x["done"]) for x in runs[v]}), "sha1": sorted({str(x["sha1"]) for x in runs[v]})}
    for a, b in (("fused", "commands"), ("plain", "parent")):
        if a in runs and b in runs:
            res["same_bytes_%s_%s" % (a, b)] = res["variants"][a]["sha1"] == res["variants"][b]["sha1"] and len(res["variants"][a]["sha1"]) == 1 and res["variants"][a]["sha1"] != ["None"]
    print(json.dumps(res))
    if not keep:
        shutil.rmtree(d)


if __name__ == "__main__":
    main()
