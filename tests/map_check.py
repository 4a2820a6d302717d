"""What the read mapper's GPU test modules share (tests/test_map_gpu.py, tests/test_map_shapes_gpu.py): the exact comparison
of a result with the CPU oracle's (tests/map_oracle.py) -- all nine arrays, both strings of every read, the six counters --
the device flavour's outputs as numpy arrays, and the two fixtures (a test module imports them by name)."""
import dataclasses

import numpy as np
import pytest

import map_inputs as mi
import map_oracle as mo

FIELDS = ["score", "second", "flags", "votes", "ref_start", "ref_end", "read_start", "read_end", "err"]
COUNTERS = ["seeds", "seeds_over_max_occ", "hits", "clusters", "pairs_aligned", "reads_mapped"]


@pytest.fixture(params=["auto", "general"])
def layout(request, monkeypatch):
    if request.param == "general":
        monkeypatch.setenv("POLYHIP_BWT_GENERAL", "1")
    else:
        monkeypatch.delenv("POLYHIP_BWT_GENERAL", raising=False)
    return request.param


@pytest.fixture(scope="module")
def nuc4_scoring():
    from poly_amd import align, alphabet, matrix
    a = alphabet.NewAlphabet(list("-ACGT"))
    return align.NewScoring(matrix.NewSubstitutionMatrix(a, a, matrix.NUC_4), mi.GAP)


def _params(P: mo.Params):
    from poly_amd import mapper
    return mapper.MapParams(**dataclasses.asdict(P))


def _pack(reads):
    offs = np.zeros(len(reads) + 1, np.uint64)
    offs[1:] = np.cumsum([len(r) for r in reads])
    return np.frombuffer(b"".join(reads), np.uint8).copy(), offs


def _assert_equal(got, hits, strings=True):
    """got: anything with the FIELDS as arrays (+ alignA / alignB lists)"""
    for f in FIELDS:
        want = np.array([getattr(h, f) for h in hits], dtype=np.int64)
        have = np.asarray(getattr(got, f)).astype(np.int64)
        bad = np.nonzero(want != have)[0]
        assert bad.size == 0, f"{f}: {bad.size} reads differ, first {bad[0]}: got {have[bad[0]]}, want {want[bad[0]]}"
    if strings:
        for i, h in enumerate(hits):
            assert got.alignA[i] == h.alignA and got.alignB[i] == h.alignB, f"aligned strings of read {i}"


def _assert_info(info):
    from poly_amd import mapper
    got = mapper.last_info()
    assert {k: got[k] for k in COUNTERS} == {k: info[k] for k in COUNTERS}
    return got


class _Dev:
    """the device flavour's outputs as numpy arrays.  packed: (buf, offs) instead of packing `reads` (offs need not start
    at 0); max_len: instead of the longest read's length"""

    def __init__(self, index, scoring, reads, P, work_bytes=None, strings=True, capacity=None, max_len=None, packed=None):
        import torch
        from poly_amd import mapper
        dev = torch.device("cuda")
        buf, offs = _pack(reads) if packed is None else packed
        n = len(reads)
        self.max_len = max((len(r) for r in reads), default=0) if max_len is None else max_len
        rt = torch.from_numpy(buf).to(dev) if len(buf) else torch.zeros(1, dtype=torch.uint8, device=dev)
        ot = torch.from_numpy(offs.astype(np.int64)).to(dev)
        i64 = [torch.full((max(n, 1),), -7, dtype=torch.int64, device=dev) for _ in range(2)]
        i32 = [torch.full((max(n, 1),), -7, dtype=torch.int32, device=dev) for _ in range(7)]
        cap = capacity if capacity is not None else sum(len(r) for r in reads) * 2 + 1024
        sa = torch.zeros(max(cap, 1), dtype=torch.uint8, device=dev)[:cap] if strings else None
        sb = torch.zeros(max(cap, 1), dtype=torch.uint8, device=dev)[:cap] if strings else None
        so = torch.zeros(n + 1, dtype=torch.int64, device=dev) if strings else None
        p = _params(P)
        self.full = mapper.workspace_bytes(index, scoring, p, n, self.max_len)
        wt = None if work_bytes is None else torch.empty(max(work_bytes(self.full), 1), dtype=torch.uint8, device=dev)
        self.status = mapper.map_reads_dev(index, scoring, rt, ot, self.max_len, p, *i64, *i32, sa, sb, so, wt)
        torch.cuda.synchronize()
        self.score, self.second = (t.cpu().numpy()[:n] for t in i64)
        (self.flags, self.votes, self.ref_start, self.ref_end, self.read_start, self.read_end,
         self.err) = (t.cpu().numpy().view(np.uint32)[:n] for t in i32)
        self.alignA = self.alignB = None
        if strings:
            self.aln_off = so.cpu().numpy()
            if self.status == 0:
                a, b, o = sa.cpu().numpy(), sb.cpu().numpy(), self.aln_off
                self.alignA = [a[o[i]:o[i + 1]].tobytes() for i in range(n)]
                self.alignB = [b[o[i]:o[i + 1]].tobytes() for i in range(n)]
