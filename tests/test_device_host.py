"""CPU test of the device selection every stage shares (csrc/device.h UseDevice): in one child process that sees no HIP device,
one device entry point per stage is called through the package with a valid tiny input and must fail with XV_ERR_DEVICE and the
stage's own sentence, and once with an invalid argument, which must be reported as such before any device is looked for."""
import json
import os
import subprocess
import sys

import helpers as H

NO_GPU = dict(os.environ, HIP_VISIBLE_DEVICES="")

# the sentences of the eight UseDevice bodies the stages had before they shared one
NEEDS = {
    "backend_apply": "the back-end kernels need",
    "plda_transform": "the PLDA back-end kernels need",
    "mfcc": "the feature kernels need",
    "vad": "the feature kernels need",
    "reverberate": "the reverberation kernels need",
    "compress": "the compression kernels need",
    "cmvn_sliding": "the feature front-end's kernels need",
    "cmvn_stats": "the CMVN kernels need",
    "add_deltas": "the UBM kernels need",
    "ivector_extractor": "i-vector extraction needs",
}

# (status, a part of the message) of the call with an invalid argument
XV_ERR_IO, XV_ERR_DEVICE, XV_ERR_ARG = 1, 3, 4
REFUSED = {
    "backend_apply": (XV_ERR_ARG, "Dimension mismatch: input vector has dimension 4 and transform has 7 columns"),
    "plda_transform": (XV_ERR_DEVICE, "PldaTransform: example counts must be positive"),
    "mfcc": (XV_ERR_ARG, "You may have set --num-mel-bins too large"),
    "vad": (XV_ERR_ARG, "vad_frames_context must be >= 0"),
    "reverberate": (XV_ERR_IO, "wav-reverberate: utterance 0 has no samples"),
    "compress": (XV_ERR_ARG, "compression method 4 (a fixed range) is not built"),
    "cmvn_sliding": (XV_ERR_IO, "cmvn-sliding: more than 64 feature columns"),
    "cmvn_stats": (XV_ERR_ARG, "xv_cmvn_stats: bad argument"),
    "add_deltas": (XV_ERR_IO, "delta-order must be between 0 and 8"),
    "ivector_extractor": (XV_ERR_IO, "the i-vector dimension 1025 is above the device solve's limit of 1024"),
}


def _child():
    import numpy as np
    P = H.pkg()
    x = np.ones((2, 4), np.float32)
    m = np.ones((3, 5), np.float32)
    conf = dict(sample_frequency=8000.0, frame_length=25.0, low_freq=20.0, high_freq=3700.0, dither=0.0)
    eye, zeros, ones = np.eye(4), np.zeros(4), np.ones(4)

    def cmvn_stats_bad():
        L = P.lib()
        off = np.zeros(2, np.int32)
        st = np.zeros((1, 2, 6))
        P._check(L.xv_cmvn_stats(0, m.ctypes.data, off.ctypes.data, -1, 5, st.ctypes.data, None))

    calls = {
        "backend_apply": (lambda: P.backend_apply(x), lambda: P.backend_apply(x, transform=np.ones((3, 7), np.float32))),
        "plda_transform": (lambda: P.plda_transform(x, eye, zeros, ones), lambda: P.plda_transform(x, eye, zeros, ones, num=[1.0, 0.0])),
        "mfcc": (lambda: P.mfcc([np.zeros(400, np.int16)], **conf), lambda: P.mfcc([np.zeros(400, np.int16)], num_mel_bins=200, **conf)),
        "vad": (lambda: P.vad([m]), lambda: P.vad([m], vad_frames_context=-1)),
        "reverberate": (lambda: P.reverberate([np.ones(100, np.float32)]), lambda: P.reverberate([np.zeros(0, np.float32)])),
        "compress": (lambda: P.compress([m]), lambda: P.compress([m], method=4, kernel_time_reps=1)),
        "cmvn_sliding": (lambda: P.cmvn_sliding([m]), lambda: P.cmvn_sliding([np.ones((3, 65), np.float32)])),
        "cmvn_stats": (lambda: P.cmvn_stats([m]), cmvn_stats_bad),
        "add_deltas": (lambda: P.add_deltas([m]), lambda: P.add_deltas([m], order=9)),
        "ivector_extractor": (lambda: P.IvectorExtractor(np.ones(1), np.ones((1, 2, 2)), np.array([[1.0, 0.0, 1.0]])),
                              lambda: P.IvectorExtractor(np.ones(1), np.ones((1, 2, 1025)), np.array([[1.0, 0.0, 1.0]]))),
    }
    got = {}
    for name, pair in calls.items():
        got[name] = []
        for fn in pair:
            try:
                fn()
                got[name].append([0, ""])
            except P.XvError as e:
                got[name].append([e.status, str(e)])
    print(json.dumps(got))


def test_every_stage_names_itself_without_a_device_and_reports_arguments_first():
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], env=NO_GPU, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    got = json.loads(r.stdout.decode().splitlines()[-1])
    assert sorted(got) == sorted(NEEDS) == sorted(REFUSED)
    for name, who_needs in NEEDS.items():
        (status, msg), (bad_status, bad_msg) = got[name]
        assert status == XV_ERR_DEVICE, (name, status, msg)
        assert msg == "xvec_hip status 3: no HIP device available: %s a gfx950 GPU (there is no CPU path)" % who_needs, name
        assert bad_status == REFUSED[name][0] and REFUSED[name][1] in bad_msg and "no HIP device" not in bad_msg, (name, bad_status, bad_msg)


if __name__ == "__main__":
    _child()
