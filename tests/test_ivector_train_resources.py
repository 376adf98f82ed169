"""hipcc's resource remarks for the kernels of i-vector extractor training (cross-compiled, no GPU): no scratch, no spills, and the
rank update on the fp64 matrix cores."""
import os
import re
import shutil
import subprocess

import helpers as H

CSRC = os.path.join(H.ROOT, H.PKG_NAME, "csrc")
SRC = os.path.join(CSRC, "ivex_train_kernels.hip")


def test_ivex_train_kernels_use_no_scratch_and_spill_nothing():
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    assert os.path.exists(hipcc), "hipcc is what builds the library; without it nothing here is checked"
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-c", SRC, "-o", os.devnull,
                        "-Rpass-analysis=kernel-resource-usage"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:]
    names = re.findall(r"Function Name: (\S+)", r.stdout)
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stdout)]
    sspill = [int(x) for x in re.findall(r"SGPRs Spill: (\d+)", r.stdout)]
    vspill = [int(x) for x in re.findall(r"VGPRs Spill: (\d+)", r.stdout)]
    # the posterior kernel, the rank update, the small sums
    assert len(names) == 3 and len(scratch) == len(sspill) == len(vspill) == 3, r.stdout[-2000:]
    assert not any(scratch) and not any(sspill) and not any(vspill), list(zip(names, scratch, sspill, vspill))


def test_the_rank_update_is_on_the_fp64_matrix_cores():
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    asm = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", SRC, "-o", "-"], stdout=subprocess.PIPE,
                         stderr=subprocess.PIPE, text=True, timeout=600)
    assert asm.returncode == 0, asm.stderr[-2000:]
    body = re.search(r"^\S*ivex_rank_update_kernel\S*:[^\n]*\n(.*?)s_endpgm", asm.stdout, re.S | re.M)
    assert body, "the update kernel is not in the assembly"
    # 16 k steps of 4 per column tile
    assert body.group(1).count("v_mfma_f64_16x16x4_f64") >= 16
