#!/usr/bin/env python3
"""Times the feature stage on one device (not called by bench.py): the MFCC kernel alone (kernel time between two events,
best of 5 after a warm-up, copies excluded), the C ABI call including allocation and copies, and compute-mfcc-feats end to
end on wave files, for 8 kHz (the recipes' conf/mfcc.conf) and 16 kHz (Kaldi's defaults).  Bytes = 16-bit samples read +
fp32 features written.  Writes profiles/mfcc_bench.json (or the path given) and prints the same JSON line."""
import ctypes
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import helpers as H  # noqa: E402
import mfcc_ref as R  # noqa: E402
import test_gpu_mfcc as T  # noqa: E402


def main():
    P = H.pkg()
    L = P.lib()
    out = {"build": L.xv_version().decode(), "device": None, "what": "int16 speech-like utterances of 120 s, dither 1.0", "cases": {}}
    try:
        import torch
        out["device"] = torch.cuda.get_device_name(0)
    except Exception:
        pass
    for name, conf, rate, n_utts in (("8k_conf_mfcc", R.CONF_MFCC, 8000, 256), ("16k_kaldi_default", {}, 16000, 128)):
        base = [T.speechlike(900 + i, 120 * rate, float(rate)) for i in range(8)]
        waves = [base[i % 8] for i in range(n_utts)]
        o = P.mfcc_options(**conf)
        off = np.zeros(n_utts + 1, np.int64)
        off[1:] = np.cumsum([len(w) for w in waves])
        samples = np.concatenate(waves)
        frames = sum(P.mfcc_num_frames(len(w), options=o) for w in waves)
        nbytes = samples.nbytes + frames * o.num_ceps * 4
        ms = ctypes.c_float(0)
        P._check(L.xv_mfcc_kernel_time(0, ctypes.byref(o), samples.ctypes.data, off.ctypes.data, n_utts, 5, ctypes.byref(ms)))
        P.mfcc(waves[:4], options=o)
        t0 = time.perf_counter()
        P.mfcc(waves, options=o)
        call = time.perf_counter() - t0
        case = {"utterances": n_utts, "audio_s": n_utts * 120, "frames": frames, "bytes": nbytes,
                "kernel_ms": ms.value, "kernel_frames_per_s": frames / ms.value * 1e3, "kernel_bytes_per_s": nbytes / ms.value * 1e3,
                "abi_call_s": call, "abi_call_frames_per_s": frames / call}
        with tempfile.TemporaryDirectory() as d:
            for i in range(8):
                T.write_wav(os.path.join(d, "w%d.wav" % i), base[i], rate=rate)
            with open(os.path.join(d, "wav.scp"), "w") as f:
                f.write("".join("utt%04d %s/w%d.wav\n" % (i, d, i % 8) for i in range(n_utts)))
            args = [os.path.join(P.BIN_DIR, "compute-mfcc-feats")] + \
                   ["--%s=%s" % (k.replace("_", "-"), str(v).lower()) for k, v in conf.items()] + ["scp,p:%s/wav.scp" % d, "ark:%s/out.ark" % d]
            t0 = time.perf_counter()
            r = subprocess.run(args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
            wall = time.perf_counter() - t0
            case["tool"] = {"exit": r.returncode, "wall_s": wall, "frames_per_s": frames / wall, "bytes_per_s": nbytes / wall,
                            "audio_s_per_s": n_utts * 120 / wall}
        out["cases"][name] = case
    line = json.dumps(out)
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "mfcc_bench.json")
    with open(path, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")
    print(line)


if __name__ == "__main__":
    main()
