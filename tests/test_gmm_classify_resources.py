"""hipcc's resource remarks for the rerank kernel of the GMM classifiers (cross-compiled, no GPU): no scratch, no spills, no LDS."""
import os
import re
import shutil
import subprocess

import helpers as H

CSRC = os.path.join(H.ROOT, H.PKG_NAME, "csrc")
SRC = os.path.join(CSRC, "gmm_classify_kernels.hip")


def test_rerank_kernel_uses_no_scratch_and_spills_nothing():
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
    assert len(names) == 1 and "ubm_full_rerank" in names[0], r.stdout[-2000:]
    assert scratch == [0] and sspill == [0] and vspill == [0] and lds == [0], (names, scratch, sspill, vspill, lds)


def test_the_new_kernel_stays_out_of_the_counted_file():
    """test_ubm_resources.py counts the kernels of ubm_kernels.hip; the rerank lives in a file of its own, one wave per frame"""
    assert "ubm_full_rerank" not in open(os.path.join(CSRC, "ubm_kernels.hip")).read()
    hdr = open(os.path.join(CSRC, "gmm_classify_kernels.h")).read()
    w = int(re.search(r"kRerankFramesPerBlock = (\d+);", hdr).group(1))
    threads = int(re.search(r"kRerankThreads = (\d+);", hdr).group(1))
    assert threads == 64 * w
