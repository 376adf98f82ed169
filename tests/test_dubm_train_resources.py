"""hipcc's resource remarks for the diagonal-UBM-training kernels (cross-compiled, no GPU): no scratch, no spills, the number of
kernels the header documents, and the dense accumulation on the fp64 matrix cores."""
import os
import re
import shutil
import subprocess

import helpers as H

CSRC = os.path.join(H.ROOT, H.PKG_NAME, "csrc")
SRC = os.path.join(CSRC, "dubm_train_kernels.hip")


def test_dubm_train_kernels_use_no_scratch_and_spill_nothing():
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    assert os.path.exists(hipcc), "hipcc is what builds the library; without it nothing here is checked"
    documented = int(re.search(r"kDgmmNumKernels = (\d+);", open(os.path.join(CSRC, "dubm_train_kernels.h")).read()).group(1))
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-c", SRC, "-o", os.devnull,
                        "-Rpass-analysis=kernel-resource-usage"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:]
    names = re.findall(r"Function Name: (\S+)", r.stdout)
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stdout)]
    sspill = [int(x) for x in re.findall(r"SGPRs Spill: (\d+)", r.stdout)]
    vspill = [int(x) for x in re.findall(r"VGPRs Spill: (\d+)", r.stdout)]
    assert len(names) == documented and len(scratch) == len(sspill) == len(vspill) == documented, names
    for kernel in ("dgmm_sel_loglike", "dgmm_acc_partial", "dgmm_acc_reduce", "dgmm_dense_logsum", "dgmm_dense_acc"):
        assert any(kernel in n for n in names), kernel
    assert not any(scratch) and not any(sspill) and not any(vspill), list(zip(names, scratch, sspill, vspill))
    asm = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-S", "--cuda-device-only", SRC, "-o", "-"],
                         stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert asm.returncode == 0, asm.stderr[-2000:]
    assert "v_mfma_f64_16x16x4_f64" in asm.stdout
    # one score form was kept, the fmaf chain on the vector ALU (dubm_train_kernels.h): there is no f32 MFMA to look for
    assert "v_mfma_f32_16x16x4_f32" not in asm.stdout
