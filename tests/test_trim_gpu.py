"""polyhip_trim_reads and polyhip_trim_pairs on the GPU against their CPU oracle (tests/trim_oracle.py): the trimmed bytes, the
offsets, the qualities, start / end / flags / err of every entry and all counters are compared exactly.  Inputs:
tests/trim_inputs.py (what they hold is asserted in tests/test_trim_cpu.py)."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import trim_inputs as ti  # noqa: E402
import trim_oracle as to  # noqa: E402
from map_check import FIELDS, nuc4_scoring  # noqa: E402,F401

pytestmark = pytest.mark.gpu


def _same_bytes(name, got, want):
    if want is None:
        assert got is None, name
        return
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, f"{name}: {got.shape} values, want {want.shape}"
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, f"{name}: {bad.size} values differ, first at {bad[0]}: got {got[bad[0]]}, want {want[bad[0]]}"


def _assert_equal(got, want, paired=False):
    from poly_amd import trim
    for f in ("err", "start", "end", "flags"):
        _same_bytes(f, getattr(got, f), getattr(want, f))
    for q in range(2 if paired else 1):
        pick = (lambda x: x[q]) if paired else (lambda x: x)
        _same_bytes(f"offsets[{q}]", pick(got.offsets), pick(want.offsets))
        _same_bytes(f"seqs[{q}]", pick(got.seqs), pick(want.seqs))
        _same_bytes(f"quals[{q}]", pick(got.quals), pick(want.quals))
    assert trim.last_info() == want.info


def _gpu(s, mode):
    from poly_amd import trim
    lead = getattr(s, "lead", (0, 0))
    buf, offs = ti.pack(s.reads, lead[0])
    q, qo = (None, None) if s.quals is None else ti.pack(s.quals, lead[1])
    return trim.trim_packed(buf, offs, q, qo, s.adapters, trim.TrimParams(**mode))


def _gpu_pairs(s, mode):
    from poly_amd import trim
    b1, o1 = ti.pack(s.reads1)
    b2, o2 = ti.pack(s.reads2, 3)
    q1, qo1 = (None, None) if s.quals1 is None else ti.pack(s.quals1, 2)
    q2, qo2 = (None, None) if s.quals2 is None else ti.pack(s.quals2)
    return trim.trim_pairs_packed(b1, o1, b2, o2, q1, qo1, q2, qo2, s.adapters, trim.TrimParams(**mode))


# ---------------------------------------------------------------- 1. parity with the oracle on every hand-built set
@pytest.mark.parametrize("s", ti.single_sets(), ids=lambda s: s.name)
def test_parity_reads(s):
    for mode in s.modes:
        _assert_equal(_gpu(s, mode), to.trim_reads(s.reads, s.quals, s.adapters, **mode))


@pytest.mark.parametrize("s", ti.pair_sets(), ids=lambda s: s.name)
def test_parity_pairs(s):
    for mode in s.modes:
        _assert_equal(_gpu_pairs(s, mode), to.trim_pairs(s.reads1, s.reads2, s.quals1, s.quals2, s.adapters, **mode), paired=True)


def test_parity_many_small_reads():
    """70,000 reads of 5 bytes: more reads than resident waves, more than one tile of the scan"""
    s = ti.many_small()
    _assert_equal(_gpu(s, s.modes[0]), to.trim_reads(s.reads, s.quals, s.adapters, **s.modes[0]))


def test_single_reads_as_pairs():
    """with step P off a pair call is two read calls whose entries interleave"""
    s = ti.lengths()
    half = len(s.reads) // 2
    mode = s.modes[0]
    from poly_amd import trim
    a = trim.trim_packed(*ti.pack(s.reads[:half]), *ti.pack(s.quals[:half]), s.adapters, trim.TrimParams(**mode))
    b = trim.trim_packed(*ti.pack(s.reads[half:]), *ti.pack(s.quals[half:]), s.adapters, trim.TrimParams(**mode))
    both = trim.trim_pairs_packed(*ti.pack(s.reads[:half]), *ti.pack(s.reads[half:]), *ti.pack(s.quals[:half]), *ti.pack(s.quals[half:]),
                                  s.adapters, trim.TrimParams(**mode))
    for f in ("start", "end", "flags", "err"):
        _same_bytes(f, getattr(both, f)[0::2], getattr(a, f))
        _same_bytes(f, getattr(both, f)[1::2], getattr(b, f))
    for q, one in enumerate((a, b)):
        _same_bytes("seqs", both.seqs[q], one.seqs)
        _same_bytes("quals", both.quals[q], one.quals)
        _same_bytes("offsets", both.offsets[q], one.offsets)


# ---------------------------------------------------------------- 2. properties of the call
def test_same_call_twice_gives_the_same_bytes():
    from poly_amd import trim
    s = ti.pairs()
    first = _gpu_pairs(s, s.modes[0])
    info = trim.last_info()
    again = _gpu_pairs(s, s.modes[0])
    assert trim.last_info() == info
    for f in ("start", "end", "flags", "err"):
        assert getattr(first, f).tobytes() == getattr(again, f).tobytes()
    for q in range(2):
        assert first.seqs[q].tobytes() == again.seqs[q].tobytes() and first.quals[q].tobytes() == again.quals[q].tobytes()
        assert first.offsets[q].tobytes() == again.offsets[q].tobytes()


def test_every_switch_off_returns_the_packed_batch():
    """no cut-off, no adapter, min_len 0: the output is pack_qual's batch byte for byte, through trim_fastq as well"""
    from poly_amd import fastq, trim
    s = ti.lengths()
    keep = [i for i, r in enumerate(s.reads) if len(r) > 0]            # a FASTQ record has no empty sequence
    image = ti.fastq_image([s.reads[i] for i in keep], [s.quals[i] for i in keep])
    seqs, offs, quals, qoffs, rec, perr = fastq.pack_qual(image)
    assert perr is None and len(rec) == len(keep)
    got = trim.trim_packed(seqs, offs, quals, qoffs)
    assert got.seqs.tobytes() == seqs.tobytes() and got.quals.tobytes() == quals.tobytes()
    assert got.offsets.tobytes() == offs.tobytes() == qoffs.tobytes()
    assert not got.flags.any() and not got.err.any() and not got.start.any() and (got.end == np.diff(offs.astype(np.int64))).all()
    info = trim.last_info()
    assert info["bytes_in"] == info["bytes_out"] == len(seqs) and info["reads"] == len(keep)
    via, rec2, perr2 = trim.trim_fastq(image)
    assert perr2 is None and rec2.tobytes() == rec.tobytes() and via.seqs.tobytes() == seqs.tobytes() and via.quals.tobytes() == quals.tobytes()
    cut, _, _ = trim.trim_fastq(image, [ti.ADAPTER], trim.TrimParams(min_qual_3p=20, min_qual_5p=20))
    want = to.trim_reads([s.reads[i] for i in keep], [s.quals[i] for i in keep], [ti.ADAPTER], min_qual_3p=20, min_qual_5p=20)
    _assert_equal(cut, want)


# ---------------------------------------------------------------- 3. end to end: FASTQ image -> trimmed pairs -> the mapper
def test_end_to_end_fastq_trim_map_pairs(nuc4_scoring):
    """Pairs drawn from a small text, more than half of the inserts shorter than the reads, adapters planted behind them
    (tests/trim_inputs.py::planted; the share the definition recovers is asserted in tests/test_trim_cpu.py).  The trimmed
    lengths equal the oracle's, and the mapper gives on the trimmed batch what it gives on the batch the oracle trimmed."""
    from poly_amd import bwt, fastq, mapper, trim
    d = ti.planted()
    p1, p2 = fastq.pack_qual(ti.fastq_image(d["reads1"], d["quals1"], "a")), fastq.pack_qual(ti.fastq_image(d["reads2"], d["quals2"], "b"))
    assert p1[5] is None and p2[5] is None and len(p1[4]) == len(p2[4]) == ti.PLANTED_N
    adapters = [ti.ADAPTER, ti.ADAPTER2]
    got = trim.trim_pairs_packed(p1[0], p1[1], p2[0], p2[1], p1[2], p1[3], p2[2], p2[3], adapters, trim.TrimParams(**ti.PLANTED_PARAMS))
    want = to.trim_pairs(d["reads1"], d["reads2"], d["quals1"], d["quals2"], adapters, **ti.PLANTED_PARAMS)
    for q in range(2):
        assert np.diff(got.offsets[q].astype(np.int64)).tolist() == np.diff(want.offsets[q].astype(np.int64)).tolist()
    _assert_equal(got, want, paired=True)
    index = bwt.New(d["T"])
    params = mapper.MapParams(seed_len=16, seed_stride=8, max_occ=8, band=16, max_cand=4, both_strands=True, min_score=40)
    pair_params = mapper.PairParams(20, 400, True)

    def run(t):
        return mapper.map_pairs_packed(index, nuc4_scoring, -5, -2, np.array(t.seqs[0]), t.offsets[0], np.array(t.seqs[1]), t.offsets[1],
                                       params, pair_params, max_len=ti.PLANTED_READ)
    a, b = run(got), run(want)
    for f in FIELDS + ["tlen"]:
        _same_bytes(f, getattr(a, f), getattr(b, f))
    assert a.alignA == b.alignA and a.alignB == b.alignB
    mapped = (a.flags & 1).astype(bool)
    print(f"mapped {mapped.mean():.3f} of the trimmed mates, proper {(a.flags[0::2] & mapper.FLAG_PROPER).astype(bool).mean():.3f} of the pairs")
    assert mapped.mean() > 0.5                                          # the comparison above is not one of two empty results
