"""hipcc's resource remarks for the logprob-to-post kernels (cross-compiled, no GPU): no scratch, no spills, and the LDS that
csrc/post_kernels.h states.  Only the kernels' resource metadata is read, never their instructions."""
import os
import re
import shutil
import subprocess

import helpers as H

CSRC = os.path.join(H.ROOT, H.PKG_NAME, "csrc")
SRC = os.path.join(CSRC, "post_kernels.hip")


def test_post_kernels_use_no_scratch_spill_nothing_and_keep_to_their_lds():
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    assert os.path.exists(hipcc), "hipcc is what builds the library; without it nothing here is checked"
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fhip-fp32-correctly-rounded-divide-sqrt", "-c", SRC, "-o", os.devnull,
                        "-Rpass-analysis=kernel-resource-usage"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:]
    names = re.findall(r"Function Name: (\S+)", r.stdout)
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stdout)]
    sspill = [int(x) for x in re.findall(r"SGPRs Spill: (\d+)", r.stdout)]
    vspill = [int(x) for x in re.findall(r"VGPRs Spill: (\d+)", r.stdout)]
    lds = [int(x) for x in re.findall(r"LDS Size \[bytes/block\]: (\d+)", r.stdout)]
    # the count pass, the write pass, the scan
    assert len(names) == 3 and len(scratch) == len(sspill) == len(vspill) == len(lds) == 3, r.stdout[-2000:]
    assert not any(scratch) and not any(sspill) and not any(vspill), list(zip(names, scratch, sspill, vspill))
    hdr = open(os.path.join(CSRC, "post_kernels.h")).read()
    threads = int(re.search(r"kPostScanThreads = (\d+);", hdr).group(1))
    assert "kPostCountLdsBytes = 0, kPostWriteLdsBytes = 0, kPostScanLdsBytes = kPostScanThreads * 4;" in hdr
    for name, size in zip(names, lds):
        assert size == (threads * 4 if "scan" in name else 0), (name, size)
    assert sum("scan" in n for n in names) == 1
