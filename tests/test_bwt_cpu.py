"""search/bwt without a GPU: the CPU oracle against the reference's own tables (tests/golden/bwt/), its cyclic
semantics on hand cases, poly_amd.bwt's argument errors before any device call, and the library's new symbols."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import bwt_oracle as bo  # noqa: E402

GOLD = json.load(open(os.path.join(HERE, "golden", "bwt", "reference_tables.json")))
PANGRAM = (GOLD["pangram_base"] * GOLD["pangram_repeat"]).encode()


@pytest.fixture(scope="module")
def pangram():
    return bo.Oracle(PANGRAM, width=16)


def test_oracle_constructions_agree():
    rng = np.random.default_rng(1)
    cases = [b"banana", b"a", b"aaaa", b"ACGTACGTACGT", b"\x00!#\x80\xff\x00!", PANGRAM[:60]]
    cases += [bytes(rng.choice(np.frombuffer(b"\x00!#AB\x80\xff", np.uint8), size=int(rng.integers(1, 40)))) for _ in range(20)]
    for s in cases:
        T = bo.text(s)
        assert (bo.suffix_array(T) == bo.suffix_array_brute(T)).all(), s


def test_reference_count_table(pangram):
    for pat, want in GOLD["count"]:
        assert pangram.count(pat.encode()) == want, pat


def test_reference_locate_table(pangram):
    for pat, want in GOLD["locate_sorted"]:
        assert sorted(pangram.locate(pat.encode())) == want, pat


def test_reference_extract_transform_len(pangram):
    for a, b, want in GOLD["extract"]:
        assert PANGRAM[a:b].decode() == want
    assert pangram.transform().decode() == GOLD["transform"]
    assert bo.Oracle(b"banana").transform() == GOLD["examples"]["transform_banana"].encode()
    assert len(GOLD["len"]["sequence"]) == GOLD["len"]["len"]


def test_reference_examples():
    ex = GOLD["examples"]
    o = bo.Oracle(ex["sequence"].encode())
    assert sorted(o.locate(b"GCC")) == ex["locate_sorted_GCC"]
    assert o.count(b"CG") == ex["count_CG"]
    assert sorted(o.locate(b"CG")) == ex["locate_sorted_CG"]
    assert ex["sequence"][48:54] == ex["extract_48_54"]


def test_cyclic_semantics_by_hand():
    o = bo.Oracle(b"banana", width=20)
    assert list(o.sa) == [6, 5, 3, 1, 0, 4, 2]
    assert o.count(b"a$") == 1 and o.count(b"$b") == 1 and o.locate(b"$b") == [6]
    assert o.count(b"na$ban") == 1 and o.locate(b"na$ban") == [4]
    assert o.count(b"banana$banana") == 1     # longer than T: wraps
    assert o.count(b"anana$banana$b") == 1
    assert o.count(b"x") == 0 and o.interval(b"x") == (0, 0)
    assert o.count(b"$$") == 0
    assert o.locate(b"ana") == [3, 1]         # row order, not sorted
    for p in (b"a$", b"$b", b"na$ban", b"banana$banana", b"ana", b"$", b"n", b"x", b"a$b", b"$$"):
        assert o.interval(p) == bo.interval_brute(b"banana", p), p


def test_sort_order_puts_null_char_first():
    # '!' (0x21) and 0x00 sort AFTER '$': TestBWTReconstruction's extra '!' is there for this
    o = bo.Oracle(b"!\x00a")
    assert o.sa[0] == 3
    assert [o.T[i] for i in o.sa[1:]] == [0x00, 0x21, 0x61]


def test_new_errors_before_any_device_call(monkeypatch):
    from poly_amd import _lib, bwt

    def no_device(*a, **k):
        raise AssertionError("a device call was made")
    monkeypatch.setattr(_lib, "lib", no_device)
    with pytest.raises(ValueError) as ei:
        bwt.New("")
    assert str(ei.value) == GOLD["errors"]["new_empty"][1]
    with pytest.raises(ValueError) as ei:
        bwt.New("ba$")
    assert str(ei.value) == GOLD["errors"]["new_nullchar"][1]
    with pytest.raises(ValueError) as ei:
        bwt.New(GOLD["errors"]["new_nullchar"][0])
    assert str(ei.value) == GOLD["errors"]["new_nullchar"][1]


def test_library_exports_bwt_symbols():
    from poly_amd import _lib, build
    L = C.CDLL(build.build_lib())
    names = [n for n in _lib.SIGNATURES if n.startswith("polyhip_bwt_")]
    for n in ("polyhip_bwt_create", "polyhip_bwt_create_dev", "polyhip_bwt_destroy", "polyhip_bwt_len",
              "polyhip_bwt_transform", "polyhip_bwt_count", "polyhip_bwt_count_dev", "polyhip_bwt_locate",
              "polyhip_bwt_locate_dev", "polyhip_bwt_extract", "polyhip_bwt_extract_dev", "polyhip_bwt_workspace_bytes"):
        assert n in names
    for n in names:
        assert hasattr(L, n), n


# polyhip_bwt_workspace_bytes(n) as the library of commit c417f13 (the last one with two copies of the build's carve order)
# returned it; the function is host arithmetic and the library loads without a device
WORKSPACE_BYTES = {1: 3584, 2: 3584, 447: 21760, 448: 23040, 4095: 182272, 4096: 183552, 4097: 183552, 65537: 2883328,
                   1000003: 43944960, 5000000: 219710976, 2**32 - 2: 188726842880}


@pytest.mark.parametrize("n", sorted(WORKSPACE_BYTES))
def test_build_workspace_bytes_are_unchanged(n):
    from poly_amd import _lib
    assert _lib.lib().polyhip_bwt_workspace_bytes(n) == WORKSPACE_BYTES[n]


def test_create_refuses_without_touching_a_device():
    """Empty text: the reference's error text, from the library itself (no device needed to refuse it)."""
    from poly_amd import _lib
    h = C.c_void_p()
    st = _lib.lib().polyhip_bwt_create(None, 0, C.byref(h))
    assert st == _lib.ERR_INVALID
    assert _lib.lib().polyhip_last_error().decode() == GOLD["errors"]["new_empty"][1]
    assert not h.value
