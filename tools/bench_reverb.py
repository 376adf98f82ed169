#!/usr/bin/env python3
"""Times the augmentation stage on one device (not called by bench.py), per second of audio: the reverberation kernels alone
(sum of the kernels' times between events, best of 3 after a warm-up, copies excluded), the C ABI call including allocation
and copies, and wav-reverberate end to end on wave files (one process per utterance, each under its own timeout, stopping at
the first failure), for (a) reverberation with a 0.5 s RIR and (b) three additive noises; 8 kHz, utterances of 120 s; and stage 2 + MFCC: compute-mfcc-feats on a wav.scp of wav-reverberate
lines, taken over into its batch against the same job with XVEC_DEBUG=fuse_wav=0 (one process per entry).  The ABI call is
timed once after a small warm-up call.  As
context, not as a bar: the time the fp32 restatement of tests/reverb_ref.py (numpy, one thread) takes for one of the same
utterances on the same box.  Writes profiles/reverb_bench.json (or the path given) and prints the same JSON line."""
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
import reverb_ref as R  # noqa: E402

RATE, SECONDS, N_UTTS, N_TOOL = 8000, 120, 32, 4


def main():
    P = H.pkg()
    L = P.lib()
    out = {"build": L.xv_version().decode(), "device": None, "cases": {},
           "what": "int16 speech-like utterances of %d s at %d Hz, %d per call" % (SECONDS, RATE, N_UTTS)}
    try:
        import torch
        out["device"] = torch.cuda.get_device_name(0)
    except Exception:
        pass
    base = [R.speechlike(900 + i, SECONDS * RATE, float(RATE)) for i in range(4)]
    waves = [base[i % 4] for i in range(N_UTTS)]
    rir = R.decaying_rir(910, RATE // 2).astype(np.float32)
    noises = [R.speechlike(920 + i, SECONDS * RATE).astype(np.float32) for i in range(3)]
    add = [(noises[0], 15.0, 0.0), (noises[1], 10.0, 0.0), (noises[2], 5.0, 30.0)]
    audio = N_UTTS * SECONDS
    cases = {"reverb_rir_0.5s": dict(rirs=[0] * N_UTTS, rir_list=[rir]), "three_noises": dict(additive=[add] * N_UTTS)}
    with tempfile.TemporaryDirectory() as d:
        P.write_wave(os.path.join(d, "in.wav"), base[0], RATE)
        P.write_wave(os.path.join(d, "rir.wav"), rir, RATE)
        for i, nz in enumerate(noises):
            P.write_wave(os.path.join(d, "n%d.wav" % i), nz, RATE)
        argv = {"reverb_rir_0.5s": ["--impulse-response=%s/rir.wav" % d],
                "three_noises": ["--additive-signals=%s" % ",".join("%s/n%d.wav" % (d, i) for i in range(3)), "--snrs=15,10,5",
                                 "--start-times=0,0,30"]}
        for name, kw in cases.items():
            ms = P.reverberate(waves, rate=float(RATE), kernel_time_reps=3, **dict(kw))
            P.reverberate(waves[:2], rate=float(RATE), **{k: (v[:2] if k != "rir_list" else v) for k, v in kw.items()})
            t0 = time.perf_counter()
            P.reverberate(waves, rate=float(RATE), **dict(kw))
            call = time.perf_counter() - t0
            ref_kw = dict(rir=rir) if "rirs" in kw else dict(additive=add)
            t0 = time.perf_counter()
            R.reverberate(base[0], float(RATE), dtype=np.float32, **ref_kw)
            ref = time.perf_counter() - t0
            case = {"utterances": N_UTTS, "audio_s": audio, "kernel_ms": ms, "kernel_audio_s_per_s": audio / ms * 1e3,
                    "abi_call_s": call, "abi_call_audio_s_per_s": audio / call,
                    "numpy_ref32_one_utterance_s": ref, "numpy_ref32_audio_s_per_s": SECONDS / ref}
            wall, rc = 0.0, 0
            for i in range(N_TOOL):
                t0 = time.perf_counter()
                r = subprocess.run(["timeout", "-k", "10", "120", os.path.join(P.BIN_DIR, "wav-reverberate")] + argv[name] +
                                   ["%s/in.wav" % d, "%s/out%d.wav" % (d, i)], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
                wall += time.perf_counter() - t0
                rc = r.returncode
                if rc != 0:
                    break
            case["tool"] = {"exit": rc, "processes": N_TOOL, "wall_s": wall, "audio_s_per_s": N_TOOL * SECONDS / wall}
            out["cases"][name] = case
            if rc != 0:
                break
        # stage 2 + MFCC through compute-mfcc-feats, fused and not
        n_lines = 16
        with open(os.path.join(d, "wav.scp"), "w") as f:
            for i in range(n_lines):
                if i % 2 == 0:
                    f.write('utt%03d cat %s/in.wav | wav-reverberate --shift-output=true --impulse-response="cat %s/rir.wav |" - - |\n' % (i, d, d))
                else:
                    f.write("utt%03d wav-reverberate --shift-output=true %s --start-times='0,0,30' --snrs='15,10,5' %s/in.wav - |\n"
                            % (i, "--additive-signals='%s'" % ",".join("%s/n%d.wav" % (d, k) for k in range(3)), d))
        job = {"entries": n_lines, "audio_s": n_lines * SECONDS}
        for name, knob in (("fused", None), ("fuse_wav=0", "fuse_wav=0")):
            env = dict(os.environ, PATH=P.BIN_DIR + os.pathsep + os.environ.get("PATH", ""))
            if knob:
                env["XVEC_DEBUG"] = knob
            t0 = time.perf_counter()
            r = subprocess.run(["timeout", "-k", "10", "300", os.path.join(P.BIN_DIR, "compute-mfcc-feats"), "--sample-frequency=8000",
                                "scp,p:%s/wav.scp" % d, "ark:%s/%s.ark" % (d, name)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env)
            wall = time.perf_counter() - t0
            job[name] = {"exit": r.returncode, "wall_s": wall, "audio_s_per_s": n_lines * SECONDS / wall}
            if r.returncode != 0:
                break
        if "fuse_wav=0" in job and job["fuse_wav=0"]["exit"] == 0:
            job["same_bytes"] = open(os.path.join(d, "fused.ark"), "rb").read() == open(os.path.join(d, "fuse_wav=0.ark"), "rb").read()
        out["stage2_plus_mfcc"] = job
    line = json.dumps(out)
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "reverb_bench.json")
    with open(path, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")
    print(line)


if __name__ == "__main__":
    main()
