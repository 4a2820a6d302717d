"""K2 counter joins: what the compiler made of them (no GPU needed).  rowjoin_dense_kernel and rowjoin_nbr_kernel run
1024-thread workgroups, one per CU: 16 waves on 4 SIMDs = 4 waves per SIMD of 512 VGPRs, so every instantiation must
stay within 128 VGPRs per wave, and without scratch."""
import os
import re
import subprocess

import pytest

from poly_amd import build

SRC = os.path.join(build.CSRC, "mash_distance.hip")
KEYS = ("vgpr_count", "sgpr_count", "private_segment_fixed_size", "group_segment_fixed_size")


@pytest.fixture(scope="module")
def meta(tmp_path_factory):
    asm = str(tmp_path_factory.mktemp("k2") / "mash_distance.s")
    flags = [f for f in build.CXXFLAGS if f != "-fPIC"]
    res = subprocess.run([build._hipcc()] + flags + ["--cuda-device-only", "-S", SRC, "-o", asm],
                         capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-2000:]
    text = open(asm).read()
    kernels = {}
    for block in re.split(r"\n\s+- \.", text.split("amdhsa.kernels:", 1)[1]):
        name = re.search(r"\.name:\s+(\S+)", block)
        m = name and re.search(r"rowjoin_(dense|nbr)_kernelILi(\d+)ELb([01])ELb([01])E", name.group(1))
        if m:
            kernels[(m.group(1), int(m.group(2)), int(m.group(3)), int(m.group(4)))] = {
                key: int(re.search(rf"\.{key}:\s+(\d+)", block).group(1)) for key in KEYS}
    return kernels


@pytest.mark.parametrize("reg", (0, 1))
@pytest.mark.parametrize("compact", (0, 1))
@pytest.mark.parametrize("bits", (10, 16))
@pytest.mark.parametrize("kernel", ("dense", "nbr"))
def test_join_kernel_keeps_four_waves_per_simd(meta, kernel, bits, compact, reg):
    m = meta[(kernel, bits, compact, reg)]
    assert m["vgpr_count"] <= 128, m
    assert m["private_segment_fixed_size"] == 0, m  # no scratch
