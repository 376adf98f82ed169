"""hipcc's resource remarks for the kernels of nnet-am-compute (cross-compiled, no GPU): no scratch, no spills, and the LDS that
csrc/nnet2_kernels.h states.  Only the kernels' resource metadata is read, never their instructions."""
import os
import re
import shutil
import subprocess

import helpers as H

CSRC = os.path.join(H.ROOT, H.PKG_NAME, "csrc")
SRC = os.path.join(CSRC, "nnet2_kernels.hip")


def test_nnet2_kernels_use_no_scratch_spill_nothing_and_keep_to_their_lds():
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    assert os.path.exists(hipcc), "hipcc is what builds the library; without it nothing here is checked"
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-c", SRC, "-o", os.devnull,
                        "-Rpass-analysis=kernel-resource-usage"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:]
    names = re.findall(r"Function Name: (\S+)", r.stdout)
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stdout)]
    sspill = [int(x) for x in re.findall(r"SGPRs Spill: (\d+)", r.stdout)]
    vspill = [int(x) for x in re.findall(r"VGPRs Spill: (\d+)", r.stdout)]
    lds = [int(x) for x in re.findall(r"LDS Size \[bytes/block\]: (\d+)", r.stdout)]
    # the input preparation and the row kernel (one template), the affine, the head
    assert len(names) == 4 and len(scratch) == len(sspill) == len(vspill) == len(lds) == 4, r.stdout[-2000:]
    assert not any(scratch) and not any(sspill) and not any(vspill), list(zip(names, scratch, sspill, vspill))
    hdr = open(os.path.join(CSRC, "nnet2_kernels.h")).read()
    cols = int(re.search(r"kNnet2HeadMaxCols = (\d+);", hdr).group(1))
    threads = int(re.search(r"kNnet2HeadThreads = (\d+);", hdr).group(1))
    assert "kNnet2PrepLdsBytes = 0, kNnet2RowLdsBytes = 0, kNnet2AffineLdsBytes = 0;" in hdr
    assert "kNnet2HeadLdsBytes = kNnet2HeadMaxCols * 4 + kNnet2HeadThreads / 64 * 4;" in hdr
    for name, size in zip(names, lds):
        assert size == (cols * 4 + threads // 64 * 4 if "head" in name else 0), (name, size)
    assert sum("head" in n for n in names) == 1 and sum("affine" in n for n in names) == 1 and sum("row" in n for n in names) == 2
