"""hipcc's resource remarks for the GMM-UBM kernels (cross-compiled, no GPU): no scratch, no spills."""
import os
import re
import shutil
import subprocess

import helpers as H

SRC = os.path.join(H.ROOT, H.PKG_NAME, "csrc", "ubm_kernels.hip")


def test_ubm_kernels_use_no_scratch_and_spill_nothing():
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    assert os.path.exists(hipcc), "hipcc is what builds the library; without it nothing here is checked"
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-c", SRC, "-o", os.devnull,
                        "-Rpass-analysis=kernel-resource-usage"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:]
    names = re.findall(r"Function Name: (\S+)", r.stdout)
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stdout)]
    sspill = [int(x) for x in re.findall(r"SGPRs Spill: (\d+)", r.stdout)]
    vspill = [int(x) for x in re.findall(r"VGPRs Spill: (\d+)", r.stdout)]
    # deltas, selection, three widths of the full-covariance kernel, the softmax (the sort: test_bucket_sort_resources.py)
    assert len(names) == 6 and len(scratch) == len(sspill) == len(vspill) == 6, r.stdout[-2000:]
    assert not any(scratch) and not any(sspill) and not any(vspill), list(zip(names, scratch, sspill, vspill))
