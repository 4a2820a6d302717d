"""The search with mismatches as a cgo caller sees it: tests/abi/abi_bwt_mismatch.c, a plain C program linked against
libpolyhip.so only, takes the banana and (ACGT)^3 cases and the capacity rule through the C ABI from two threads on one
handle and compares with a brute-force compare of its own."""
import subprocess

import pytest

pytestmark = pytest.mark.gpu


def test_two_threads_on_one_handle():
    from poly_amd import build
    exe = build.build_abi_bwt_mismatch()
    res = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(res.stdout, res.stderr)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "abi_bwt_mismatch ok: 2 threads" in res.stdout
