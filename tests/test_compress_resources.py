"""hipcc's resource remarks for the compression kernels (cross-compiled, no GPU): no scratch, no spills."""
import os
import re
import shutil
import subprocess

import helpers as H

SRC = os.path.join(H.ROOT, H.PKG_NAME, "csrc", "compress_kernels.hip")


def test_compress_kernels_use_no_scratch_and_spill_nothing():
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    assert os.path.exists(hipcc), "hipcc is what builds the library; without it nothing here is checked"
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-c", SRC, "-o", os.devnull,
                        "-Rpass-analysis=kernel-resource-usage"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:]
    names = re.findall(r"Function Name: (\S+)", r.stdout)
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stdout)]
    sspill = [int(x) for x in re.findall(r"SGPRs Spill: (\d+)", r.stdout)]
    vspill = [int(x) for x in re.findall(r"VGPRs Spill: (\d+)", r.stdout)]
    vgprs = [int(x) for x in re.findall(r"\bVGPRs: (\d+)", r.stdout)]
    lds = [int(x) for x in re.findall(r"LDS Size \[bytes/block\]: (\d+)", r.stdout)]
    # minimum / maximum, selection, encode
    assert len(names) == 3 and len(scratch) == len(sspill) == len(vspill) == len(vgprs) == len(lds) == 3, r.stdout[-2000:]
    assert not any(scratch) and not any(sspill) and not any(vspill), list(zip(names, scratch, sspill, vspill))
    # at most 64 registers keep eight waves on a SIMD (the selection kernel runs 1024 threads a workgroup); its two histograms
    # are 48 KiB of LDS
    assert max(vgprs) <= 64, list(zip(names, vgprs))
    assert max(lds) <= 64 * 1024, list(zip(names, lds))
