"""polyhip_demux_reads and polyhip_demux_pairs on the GPU against their CPU oracle (tests/demux_oracle.py): barcode / bstart / mism
/ flags / err of every entry, sample, order, sample_start, the grouped bytes, offsets and qualities and all counters are compared
exactly.  Inputs: tests/demux_inputs.py (what they hold is asserted in tests/test_demux_cpu.py)."""
import functools
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import demux_inputs as di  # noqa: E402
import demux_oracle as do  # noqa: E402
import map_inputs as mi  # noqa: E402
import map_oracle as mo  # noqa: E402
from map_check import FIELDS, _assert_equal as _assert_hits, nuc4_scoring  # noqa: E402,F401

pytestmark = pytest.mark.gpu

SINGLE = {s.name: s for s in di.single_sets()}
PAIRS = {s.name: s for s in di.pair_sets()}


def _same_bytes(name, got, want):
    if want is None:
        assert got is None, name
        return
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, f"{name}: {got.shape} values, want {want.shape}"
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, f"{name}: {bad.size} values differ, first at {bad[0]}: got {got[bad[0]]}, want {want[bad[0]]}"


def _assert_equal(got, want, paired=False):
    from poly_amd import demux
    assert got.nsamples == want.nsamples
    for f in ("err", "flags", "barcode", "bstart", "mism", "sample", "order", "sample_start"):
        _same_bytes(f, getattr(got, f), getattr(want, f))
    for q in range(2 if paired else 1):
        pick = (lambda x: x[q]) if paired else (lambda x: x)
        _same_bytes(f"offsets[{q}]", pick(got.offsets), pick(want.offsets))
        _same_bytes(f"seqs[{q}]", pick(got.seqs), pick(want.seqs))
        _same_bytes(f"quals[{q}]", pick(got.quals), pick(want.quals))
    assert demux.last_info() == want.info


@functools.lru_cache(maxsize=None)
def _want(name, k):
    """the oracle's answer for mode k of a set, computed once; callers leave it unchanged"""
    if name == "random_many":
        s = di.random_many()
        return do.demux_reads(s.reads, s.barcodes, s.quals, **s.modes[k])
    if name in PAIRS:
        s = PAIRS[name]
        return do.demux_pairs(s.reads1, s.reads2, s.barcodes1, s.barcodes2, s.pair_sample, s.nsamples, s.quals1, s.quals2, **s.modes[k])
    s = SINGLE[name]
    return do.demux_reads(s.reads, s.barcodes, s.quals, **s.modes[k])


def _gpu(s, mode):
    from poly_amd import demux
    buf, offs = di.pack(s.reads, s.lead)
    q, qo = (None, None) if s.quals is None else di.pack(s.quals, s.lead + 2)
    return demux.demux_packed(buf, offs, s.barcodes, q, qo, demux.DemuxParams(**mode))


def _gpu_pairs(s, mode):
    from poly_amd import demux
    b1, o1 = di.pack(s.reads1, s.lead)
    b2, o2 = di.pack(s.reads2, 3)
    q1, qo1 = (None, None) if s.quals1 is None else di.pack(s.quals1, 2)
    q2, qo2 = (None, None) if s.quals2 is None else di.pack(s.quals2)
    return demux.demux_pairs_packed(b1, o1, b2, o2, s.barcodes1, s.barcodes2, s.pair_sample, s.nsamples, q1, qo1, q2, qo2,
                                    demux.DemuxParams(**mode))


# ---------------------------------------------------------------- 1. parity with the oracle on every hand-built set
@pytest.mark.parametrize("name", list(SINGLE))
def test_parity_reads(name):
    s = SINGLE[name]
    for k, mode in enumerate(s.modes):
        _assert_equal(_gpu(s, mode), _want(name, k))


@pytest.mark.parametrize("name", list(PAIRS))
def test_parity_pairs(name):
    s = PAIRS[name]
    for k, mode in enumerate(s.modes):
        _assert_equal(_gpu_pairs(s, mode), _want(name, k), paired=True)


def test_parity_random_many():
    """20,000 reads: more reads than resident waves of the match, five tiles of the sort and of the scans"""
    s = di.random_many()
    _assert_equal(_gpu(s, s.modes[0]), _want("random_many", 0))


def test_single_reads_as_pairs_without_a_second_set():
    """with nbarcodes2 == 0 a pair call decides as the read call on mate 1 does, and moves mate 2 along untouched"""
    from poly_amd import demux
    s = SINGLE["empty_samples"]
    one = _gpu(s, s.modes[0])
    mates = [r[::-1] for r in s.reads]
    both = demux.demux_pairs_packed(*di.pack(s.reads), *di.pack(mates), s.barcodes, None, None, None, *di.pack(s.quals),
                                    *di.pack([q[::-1] for q in s.quals]), demux.DemuxParams(**s.modes[0]))
    for f in ("barcode", "bstart", "mism", "flags", "err"):
        _same_bytes(f, getattr(both, f)[0::2], getattr(one, f))
    assert (both.barcode[1::2] == do.NONE).all() and not both.flags[1::2].any()
    for f in ("sample", "order", "sample_start"):
        _same_bytes(f, getattr(both, f), getattr(one, f))
    _same_bytes("seqs", both.seqs[0], one.seqs)
    _same_bytes("quals", both.quals[0], one.quals)
    assert both.seqs[1].tobytes() == b"".join(mates[i] for i in one.order)


# ---------------------------------------------------------------- 2. properties of the call
def test_same_call_twice_gives_the_same_bytes():
    from poly_amd import demux
    s = PAIRS["pairs_holes"]
    first = _gpu_pairs(s, s.modes[2])
    info = demux.last_info()
    again = _gpu_pairs(s, s.modes[2])
    assert demux.last_info() == info
    for f in ("barcode", "bstart", "mism", "flags", "err", "sample", "order", "sample_start"):
        assert getattr(first, f).tobytes() == getattr(again, f).tobytes()
    for q in range(2):
        assert first.seqs[q].tobytes() == again.seqs[q].tobytes() and first.quals[q].tobytes() == again.quals[q].tobytes()
        assert first.offsets[q].tobytes() == again.offsets[q].tobytes()
    s = di.random_many()
    a, b = _gpu(s, s.modes[0]), _gpu(s, s.modes[0])
    assert a.order.tobytes() == b.order.tobytes() and a.seqs.tobytes() == b.seqs.tobytes() and a.quals.tobytes() == b.quals.tobytes()


@pytest.mark.parametrize("name", ["lengths", "clip_edges", "random_many"])
def test_clip_off_returns_the_batch_permuted_by_order(name):
    """clip = 0: output read j is input read order[j] byte for byte, qualities too, and the decisions are those of clip = 1"""
    s = di.random_many() if name == "random_many" else SINGLE[name]
    on, off = _gpu(s, dict(s.modes[0], clip=1)), _gpu(s, dict(s.modes[0], clip=0))
    for f in ("barcode", "bstart", "mism", "flags", "err", "sample", "order", "sample_start"):
        _same_bytes(f, getattr(off, f), getattr(on, f))
    order = off.order.tolist()
    assert sorted(order) == list(range(len(s.reads)))
    assert off.seqs.tobytes() == b"".join(s.reads[i] for i in order) and off.quals.tobytes() == b"".join(s.quals[i] for i in order)
    assert np.diff(off.offsets.astype(np.int64)).tolist() == [len(s.reads[i]) for i in order]
    # the samples are runs of `order`, in input order within each
    for k in range(off.nsamples + 1):
        run = order[int(off.sample_start[k]):int(off.sample_start[k + 1])]
        assert run == sorted(run) and all((off.sample[i] if off.sample[i] != do.NONE else off.nsamples) == k for i in run)


# ---------------------------------------------------------------- 3. end to end: FASTQ image -> samples -> trimmer -> mapper
def test_end_to_end_fastq_demux_trim_map(nuc4_scoring):
    """Three constructs pooled in one FASTQ image (tests/demux_inputs.py::pooled; that every tagged read must reach its sample
    is derived and asserted on the oracle in tests/test_demux_cpu.py).  demux_fastq splits it, each sample's view goes through
    the trimmer into the mapper on its own construct: every read sits in its sample's batch, and the mapper gives on each
    batch what its CPU oracle gives on the same reads."""
    from poly_amd import bwt, demux, mapper, trim
    d = di.pooled()
    got, rec, perr = demux.demux_fastq(d["fastq"], d["barcodes"], demux.DemuxParams(**di.POOL_PARAMS))
    assert perr is None and len(rec) == len(d["reads"])
    _assert_equal(got, do.demux_reads(d["reads"], d["barcodes"], d["quals"], **di.POOL_PARAMS))
    where = np.empty(len(d["reads"]), np.int64)
    where[got.order] = np.arange(len(d["reads"]))
    P = mo.Params(seed_len=16, seed_stride=8, max_occ=8, band=16, max_cand=2, both_strands=True, min_score=40)
    for k in range(3):
        seqs, offs, quals = got.sample_batch(k)
        lo, hi = int(got.sample_start[k]), int(got.sample_start[k + 1])
        assert len(offs) == hi - lo + 1 and offs[0] == got.offsets[lo] and (k == 0) == (offs[0] == 0)
        mine = [i for i, t in enumerate(d["truth"]) if t == k]
        assert len(mine) > 200 and all(lo <= where[i] < hi for i in mine) and hi - lo == len(mine)
        assert [seqs[offs[j]:offs[j + 1]].tobytes() for j in range(hi - lo)] == [d["reads"][i][8:] for i in mine]
        t = trim.trim_packed(seqs, offs, quals, offs, None, trim.TrimParams(min_qual_3p=22, min_len=30))
        assert len(t.start) == len(mine) and not t.err.any()
        batch = [t.seqs[t.offsets[j]:t.offsets[j + 1]].tobytes() for j in range(len(mine))]
        hits, info = mo.map_reads(d["constructs"][k], batch, mi.nuc4(), mi.GAP, P)
        res = mapper.map_reads_packed(bwt.New(d["constructs"][k]), nuc4_scoring, np.array(t.seqs), t.offsets,
                                      mapper.MapParams(**vars(P)), max_len=di.POOL_READ)
        _assert_hits(res, hits)
        frac, frac_want = float((res.flags & 1).astype(bool).mean()), info["reads_mapped"] / len(mine)
        print(f"sample {k}: {len(mine)} reads, mapped {frac:.3f}")
        assert frac == frac_want and frac > 0.9                         # not a comparison of two empty results
    useqs, uoffs, _ = got.unassigned()
    assert len(uoffs) - 1 == d["truth"].count(do.NONE) and uoffs[-1] == len(useqs)
