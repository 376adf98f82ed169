"""hipcc's resource remarks for the select-and-normalise kernel (cross-compiled, no GPU): one kernel, no scratch, no spills, a
few hundred bytes of LDS."""
import os
import re
import shutil
import subprocess

import helpers as H

SRC = os.path.join(H.ROOT, H.PKG_NAME, "csrc", "cmvn_select_kernel.hip")


def test_cmvn_apply_select_uses_no_scratch_and_spills_nothing():
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    assert os.path.exists(hipcc), "hipcc is what builds the library; without it nothing here is checked"
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-c", SRC, "-o", os.devnull,
                        "-Rpass-analysis=kernel-resource-usage"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:]
    names = re.findall(r"Function Name: (\S+)", r.stdout)
    assert len(names) == 1 and "cmvn_apply_select_kernel" in names[0], names
    for what in (r"ScratchSize \[bytes/lane\]", "SGPRs Spill", "VGPRs Spill"):
        assert [int(x) for x in re.findall(what + r": (\d+)", r.stdout)] == [0], (what, r.stdout[-2000:])
    # two int32 per output row of the workgroup: where the row comes from and which norm it takes
    rows = int(re.search(r"kCmvnSelectRows = (\d+);", open(SRC.replace("cmvn_select_kernel.hip", "cmvn_kernels.h")).read()).group(1))
    assert [int(x) for x in re.findall(r"LDS Size \[bytes/block\]: (\d+)", r.stdout)] == [8 * rows], r.stdout[-2000:]
