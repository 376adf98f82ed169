"""hipcc's resource remarks for the augmentation kernels (cross-compiled, no GPU): no scratch, no spills."""
import os
import re
import shutil
import subprocess

import helpers as H

SRC = os.path.join(H.ROOT, H.PKG_NAME, "csrc", "reverb_kernels.hip")


def test_reverb_kernels_use_no_scratch_and_spill_nothing():
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
    # power, RIR spectra, signal spectra, convolution, direct convolution, mix, finish
    assert len(names) == 7 and len(scratch) == len(sspill) == len(vspill) == len(lds) == 7, r.stdout[-2000:]
    assert not any(scratch) and not any(sspill) and not any(vspill), list(zip(names, scratch, sspill, vspill))
    # the FFT kernels hold two fp32 planes of 4096 points (32 KiB) and little else: four workgroups fit a CU's 160 KiB
    assert max(lds) <= 40 * 1024, list(zip(names, lds))
