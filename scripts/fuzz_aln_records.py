"""Randomised sweep of polyhip_aln_records against tests/aln_records_oracle.py (run on the GPU box, not part of the suite):
batches of random size whose entries are random strings of column classes with random run lengths -- short runs, runs
around the 64-column step, long match runs for the MD's digit counts -- random clips, scores, unmapped entries, invalid
columns and coordinates that do not fit; eqx and paired at random.  Seeded by iteration number alone.

    python scripts/fuzz_aln_records.py [seconds] [first seed]
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import aln_records_inputs as ari  # noqa: E402
import aln_records_oracle as aro  # noqa: E402
from poly_amd import sam  # noqa: E402

budget = float(sys.argv[1]) if len(sys.argv) > 1 else 120.0
seed0 = int(sys.argv[2]) if len(sys.argv) > 2 else 1
INPUTS = ("flags", "score", "second", "read_start", "read_end", "read_len", "alnA", "alnB", "aln_off")
ARRAYS = ("cigar_off", "cigar", "md_off", "md", "nm", "mapq", "sam_flag", "err")


def classes(rng):
    kind = int(rng.integers(0, 5))
    top = (3, 40, 70, 200, 1200)[kind]                # the longest run of this entry
    weights = ("===XID", "=XID", "====XXID", "==========X", "=====ID")[int(rng.integers(0, 5))]
    out = ""
    for _ in range(int(rng.integers(1, 40))):
        out += weights[int(rng.integers(0, len(weights)))] * int(rng.integers(1, top + 1))
    return out[:int(rng.integers(1, 12_000))]


def entry(rng, k):
    u = rng.random()
    if u < 0.15:
        return ari.unmapped(k)
    cl = classes(rng)
    if u < 0.20:
        at = int(rng.integers(0, len(cl)))
        cl = cl[:at] + "?" + cl[at + 1:]
    c = ari.case(f"f{k}", cl, rng, left=int(rng.integers(0, 3)) * int(rng.integers(0, 50)), right=int(rng.integers(0, 3)) * int(rng.integers(0, 50)),
                 flags=1 | int(rng.integers(0, 4)) << 1, score=int(rng.integers(1, 800)), second=int(rng.integers(-20, 800)))
    if 0.20 <= u < 0.25:                              # coordinates that do not fit the strings
        return ari.Case(c.name, c.classes, c.A, c.B, c.read_start + int(rng.integers(1, 3)), c.read_end, c.read_len, c.flags, c.score, c.second)
    if 0.25 <= u < 0.27:
        return ari.Case(c.name, "", b"", b"", c.read_start, c.read_start, c.read_len, c.flags, c.score, c.second)
    return c


t_end = time.time() + budget
it = entries = 0
while time.time() < t_end:
    rng = np.random.default_rng(seed0 + it)
    it += 1
    n = int(rng.choice([1, 2, 7, 64, 255, 256, 257, 600])) if rng.random() < 0.5 else int(rng.integers(1, 300))
    cs = [entry(rng, k) for k in range(n)]
    p = ari.pack(cs)
    eqx, paired = bool(rng.integers(0, 2)), bool(rng.integers(0, 2)) and n % 2 == 0
    want = aro.records(*[p[k] for k in INPUTS], eqx, paired)
    got = sam.records_packed(**p, eqx=eqx, paired=paired)
    for f in ARRAYS:
        assert np.array_equal(getattr(got, f), getattr(want, f)), (seed0 + it - 1, n, eqx, paired, f)
    assert sam.last_info() == want.info, (seed0 + it - 1, "info")
    entries += n
print(f"fuzz_aln_records: {it} batches, {entries} entries equal the oracle (seeds {seed0}..{seed0 + it - 1})")
