"""hipcc's resource remarks for the counting sort's kernels (cross-compiled, no GPU): no scratch, no spills, and the ranking
kernel's LDS is one chunk of keys."""
import os
import re
import shutil
import subprocess

import helpers as H

SRC = os.path.join(H.ROOT, H.PKG_NAME, "csrc", "bucket_sort.hip")


def test_bucket_sort_kernels_use_no_scratch_and_spill_nothing():
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
    # ranks, the scan over the chunks of several segments and of one, the scan over the keys, placement: the segment table
    # travels by value in the argument struct, and indexing it must not cost scratch
    assert len(names) == 5 and len(scratch) == len(sspill) == len(vspill) == len(lds) == 5, r.stdout[-2000:]
    assert not any(scratch) and not any(sspill) and not any(vspill), list(zip(names, scratch, sspill, vspill))
    chunk = int(re.search(r"kBucketSortChunk = (\d+);", open(SRC[:-3] + "h").read()).group(1))
    assert [l for n, l in zip(names, lds) if "rank_kernel" in n] == [4 * chunk], list(zip(names, lds))
    assert "warning" not in r.stdout, r.stdout[-2000:]
