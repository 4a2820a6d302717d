"""K1 slab kernel: what the compiler made of it (no GPU needed).  Eight workgroups of 256 threads per CU need at most
64 VGPRs and 80 SGPRs per wave and no scratch; the tail-byte table is addressed from LDS address 0, which holds only
while the kernel has no static LDS (its dynamic LDS then starts at 0)."""
import os
import re
import subprocess

import pytest

from poly_amd import build

SRC = os.path.join(build.CSRC, "mash_sketch.hip")


@pytest.fixture(scope="module")
def meta(tmp_path_factory):
    asm = str(tmp_path_factory.mktemp("k1") / "mash_sketch.s")
    flags = [f for f in build.CXXFLAGS if f != "-fPIC"]
    res = subprocess.run([build._hipcc()] + flags + ["--cuda-device-only", "-S", SRC, "-o", asm],
                         capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-2000:]
    text = open(asm).read()
    kernels = {}
    for block in re.split(r"\n\s+- \.", text.split("amdhsa.kernels:", 1)[1]):
        name = re.search(r"\.name:\s+(\S+)", block)
        if name and "sketch_slab_kernel" in name.group(1):
            kernels[int(re.search(r"sketch_slab_kernelILi(\d+)E", name.group(1)).group(1))] = {
                key: int(re.search(rf"\.{key}:\s+(\d+)", block).group(1))
                for key in ("vgpr_count", "sgpr_count", "private_segment_fixed_size", "group_segment_fixed_size")}
    return kernels


@pytest.mark.parametrize("k", (17, 21, 31))
def test_slab_kernel_fits_eight_workgroups_per_cu(meta, k):
    m = meta[k]
    assert m["vgpr_count"] <= 64, m
    assert m["sgpr_count"] <= 80, m
    assert m["private_segment_fixed_size"] == 0, m  # no scratch
    assert m["group_segment_fixed_size"] == 0, m  # the lookup table sits at LDS address 0
