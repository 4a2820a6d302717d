"""K1 slab pass: its survivor threshold (poly_amd/csrc/k1_tauq.h, slab_tauq) is the 64-bit formula
((target << 32) // nwin) | 0xFFFF bit for bit, computed with one 32-bit division.  The header is compiled alone into a
small host program and compared with Python's integers for every nwin from s to 2^20, random nwin up to 2^32 and
beyond, and the neighbourhoods of powers of two, at the (k, s) pairs of tests/test_k1_slab_bounds_gpu.py.  No GPU."""
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

from poly_amd import build

KS = ((21, 1000), (17, 200), (31, 2000))

PROG = r"""
#include "k1_tauq.h"
#include <cstdio>
#include <cstdlib>
#include <vector>
int main(int argc, char **argv)
{
    const uint32_t target = (uint32_t)strtoul(argv[1], nullptr, 10);
    FILE *f = fopen(argv[2], "rb");
    std::vector<int64_t> nwin;
    int64_t x;
    while (fread(&x, sizeof x, 1, f) == 1)
        nwin.push_back(x);
    fclose(f);
    std::vector<uint32_t> out(nwin.size());
    for (size_t i = 0; i < nwin.size(); ++i)
        out[i] = polyhip::k1::slab_tauq(target, nwin[i]);
    f = fopen(argv[3], "wb");
    fwrite(out.data(), sizeof(uint32_t), out.size(), f);
    fclose(f);
    return 0;
}
"""


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        cxx = build._hipcc()
    d = tmp_path_factory.mktemp("tauq")
    src, exe = d / "tauq.cpp", d / "tauq"
    src.write_text(PROG)
    res = subprocess.run([cxx, "-O2", "-std=c++17", "-I", build.CSRC, str(src), "-o", str(exe)],
                         capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-2000:]
    return d, exe


def _want(target, nwin):
    q = (np.uint64(target) << np.uint64(32)) // nwin.astype(np.uint64)
    return np.where(nwin > target, (q | np.uint64(0xFFFF)), np.uint64(0xFFFFFFFF)).astype(np.uint64)


@pytest.mark.parametrize("k,s", KS)
def test_slab_tauq_is_the_64_bit_formula(prog, k, s):
    d, exe = prog
    target = s + 6 * int(math.sqrt(s)) + 16
    rng = np.random.default_rng(s)
    near = [(1 << e) + o for e in range(1, 41) for o in range(-3, 4)]
    near += [(target << e) + o for e in range(0, 18) for o in range(-3, 4)]
    nwin = np.concatenate([
        np.arange(s, 1 << 20, dtype=np.int64),
        rng.integers(1, 1 << 32, 200_000, dtype=np.int64),
        rng.integers(1 << 32, 1 << 40, 1000, dtype=np.int64),
        np.array([n for n in near if n >= 1], dtype=np.int64),
        np.array([1, target - 1, target, target + 1, (1 << 32) - 1, 1 << 32, (1 << 32) + 1], dtype=np.int64),
    ])
    nwin.tofile(str(d / "nwin.bin"))
    res = subprocess.run([str(exe), str(target), str(d / "nwin.bin"), str(d / "tauq.bin")], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    got = np.fromfile(str(d / "tauq.bin"), dtype=np.uint32).astype(np.uint64)
    want = _want(target, nwin)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, [(int(nwin[i]), int(got[i]), int(want[i])) for i in bad[:8]]
