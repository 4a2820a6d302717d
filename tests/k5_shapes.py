"""Least-rotation (K5, least_rotation.hip) inputs aimed at the data-dependent paths of its three kernels -- the wave kernel,
the workgroup kernel with the sequence in LDS, the workgroup kernel reading global memory -- on both strands
(tests/test_k5_shapes_cpu.py asserts that each input has the property it is named for, tests/test_k5_shapes_gpu.py compares
the GPU with the oracle on them).  Builders only: DNA letters ACGT, fixed seeds, no GPU, every list cached.

Also here: candidates() / period() / equal_bytes(), a numpy restatement of what a K5 kernel sees of a sequence -- how many
positions hold the least first word, whether the sequence is a repetition of a shorter block, for how many bytes the best
candidates stay equal.  What the kernels do with them:

  candidates > 1024 (LIST_CAP, WLIST), not a closed repeat    the two-pointer search
  candidates evenly spread over a closed repeat               the search restarts on one block (ne = d)
  65..1024 candidates that stay equal                         rounds over the list until they stall (wave kernel: three
                                                              rounds without a loss; workgroup kernels: 64 rounds)
  2..64 candidates that stay equal for > 260 bytes            one candidate per lane, 64 rounds of 4 bytes behind the first
                                                              word, then the two-pointer search (`wserial`)
  the least word is four equal bytes                          one candidate per run; none at all in a homopolymer

Every input comes with its reverse complement, which carries the same period and a candidate count of its own (Member.rc_cand):
the second strand of seqhash.Hash(circular, double-stranded) is searched on the reverse complement of what is passed in, so
feeding revcomp(t) puts t's properties on that search."""
from __future__ import annotations

import dataclasses
import functools

import numpy as np

import oracle as orc

LIST_CAP = 1024       # candidates a kernel keeps (least_rotation.hip LIST_CAP, WLIST)
LANES = 64            # at most this many candidates: one per lane
MAX_ROUNDS = 64       # rounds of 4 bytes before the two-pointer search takes over
STALL_BYTES = 4 + 4 * MAX_ROUNDS   # 260: the compared depth at which the rounds give up
WAVE_SEQ_MAX = 7168   # the longest sequence a wave takes by default
GLOBAL_MIN = 120 * 1024 - 24 + 1   # 122,857: n + 24 > 120 KiB, LDS cannot hold it
WAVE_STRIDE = 8192    # sequences between two that one wave takes in turn (2048 workgroups of four waves)


# inputs named for a property they do not have (test_k5_shapes_cpu.py records what they are instead)
ONE_CANDIDATE_IN_NAME_OF_MANY = ((b"AAAC" * 1500)[:-1], b"CGT" * 2000 + b"A" + b"CGT" * 30 + b"AA")
STALLED_IN_NAME_ONLY = b"GATTACA" * 700 + b"GAT"


def revcomp(s: bytes) -> bytes:
    return orc.reverse_complement(s)


# ---------------------------------------------------------------- what a kernel sees
def words(s: bytes) -> np.ndarray:
    """the big-endian word of the 4 bytes at every cyclic position"""
    a = np.frombuffer(s, np.uint8).astype(np.uint32)
    return (a << 24) | (np.roll(a, -1) << 16) | (np.roll(a, -2) << 8) | np.roll(a, -3)


def candidate_positions(s: bytes) -> np.ndarray:
    """the cyclic positions whose word is the least one; when that word is four equal bytes only the first position of
    each run (a homopolymer has none)"""
    if not s:
        return np.zeros(0, np.int64)
    w = words(s)
    m = int(w.min())
    hit = w == m
    if len(s) >= 4 and len({(m >> sh) & 0xFF for sh in (0, 8, 16, 24)}) == 1:
        hit &= ~np.roll(hit, 1)
    return np.flatnonzero(hit)


def candidates(s: bytes) -> int:
    return len(candidate_positions(s))


def period(s: bytes) -> int:
    """the smallest d dividing n with s == s[d:] + s[:d]"""
    return (s + s).find(s, 1) if s else 0


def equal_bytes(s: bytes, cap: int = STALL_BYTES + 64) -> int:
    """for how many leading bytes at least two of the best candidates are identical, in the kernels' steps of four (0:
    fewer than two candidates; capped, and never more than the length rounded up to a step)"""
    p = candidate_positions(s)
    if len(p) < 2:
        return 0
    w, n, depth = words(s), len(s), 4
    while depth < min(n, cap):
        nxt = w[(p + depth) % n]
        keep = p[nxt == nxt.min()]
        if len(keep) < 2:
            break
        p = keep
        depth += 4
    return depth


# ---------------------------------------------------------------- families
@dataclasses.dataclass(frozen=True)
class Family:
    cand: tuple            # candidates of the strand the family is built on (lo, hi), per size where they differ
    closed: bool | None    # period < n (None: either)
    stalls: bool | None    # equal_bytes > 260 (None: either)
    what: str


INF = 1 << 30
FAMILIES = {
    "closed_full": Family(((LIST_CAP + 1, INF),) * 2, True, None, "closed repeat, full list"),
    "open_full": Family(((LIST_CAP + 1, INF),) * 2, False, None, "open repeat, full list"),
    "brim": Family(((LIST_CAP, LIST_CAP),) * 2, None, None, "exactly as many candidates as the list holds"),
    "random_full": Family(((150, 400), (LIST_CAP + 1, INF)), False, False, "full list without structure (random AC)"),
    "blocks_full": Family(((LIST_CAP + 1, INF),) * 2, False, False, "full list without structure (random blocks)"),
    "stalled": Family(((LANES + 1, LIST_CAP),) * 2, False, True, "stalled rounds over the list"),
    "stalled_wave": Family(((2, LANES),) * 2, False, True, "stalled rounds of one candidate per lane"),
    "closed_block": Family(((2, LANES),) * 2, True, None, "closed repeat of a long block"),
    "run_single": Family(((1, 1),) * 2, False, None, "one run of the least byte"),
    "run_origin": Family(((1, 1),) * 2, False, None, "a run of the least byte across the origin"),
    "run_two": Family(((2, 2),) * 2, False, None, "two equal runs of the least byte"),
    "homopolymer": Family(((0, 0),) * 2, True, None, "one byte throughout"),
    "run_other": Family(((1, INF),) * 2, False, None, "a long run of a byte that is not the least"),
    "edge": Family(((1, INF),) * 2, False, False, "random, on both sides of the LDS limit"),
}


@dataclasses.dataclass(frozen=True)
class Member:
    family: str
    size: int          # 1: the wave kernel takes it by default; 2: only the global-memory kernel does
    seq: bytes
    rc_cand: tuple     # candidates of the reverse complement (lo, hi)
    loses: bool = False   # seq is the LARGER strand of the two (every other member is the smaller one: fed as its reverse
                          # complement, the second strand's search meets the family's property and decides the hash)

    @property
    def cand(self):
        return FAMILIES[self.family].cand[self.size - 1]


def rand(rng, letters: bytes, n: int) -> bytes:
    return bytes(np.frombuffer(letters, np.uint8)[rng.integers(0, len(letters), n)].tolist())


def _blocks(rng, count: int) -> bytes:
    """AAAC and AAACC in random order: the least word AAAC once per block, no period"""
    return b"".join((b"AAAC", b"AAACC")[int(k)] for k in rng.integers(0, 2, count))


FULL, ONE, ANY = (LIST_CAP + 1, INF), (1, 1), (1, INF)


def _winner(s: bytes) -> bytes:
    """of s and its reverse complement the strand with the smaller least rotation (for inputs built on random ACGT, whose
    two strands are alike)"""
    r = revcomp(s)
    return s if orc.rotate_sequence(s) < orc.rotate_sequence(r) else r


@functools.lru_cache(maxsize=None)
def members() -> tuple:
    rng = np.random.default_rng(0x4B35)
    big = GLOBAL_MIN // 4 + 1          # 30,715 blocks of four: 122,860 bytes
    m = []

    def add(family, size, seq, rc_cand, loses=False):
        m.append(Member(family, size, seq, rc_cand, loses))

    # closed repeat, full list: the candidates are evenly spread and the repeat closes -- the search restarts on AAAC
    add("closed_full", 1, b"AAAC" * (LIST_CAP + 1), FULL)
    add("closed_full", 2, b"AAAC" * big, FULL)
    # open repeat, full list: the seam breaks the period, nothing thins the list out.  The reverse complement C GTTT GTTT ...
    # has the one word CGTT.  GTTT ... T is the same on the other letters: its reverse complement A AAAC AAAC ... has one
    # run AAAA and is the smaller strand
    add("open_full", 1, b"AAAC" * (LIST_CAP + 1) + b"G", ONE)
    add("open_full", 2, b"AAAC" * big + b"G", ONE)
    add("open_full", 1, b"GTTT" * (LIST_CAP + 1) + b"T", ONE, loses=True)
    add("open_full", 2, b"GTTT" * big + b"T", ONE, loses=True)
    # the list exactly full: nothing is dropped, no two-pointer search for the count's sake
    add("brim", 1, b"AAAC" * LIST_CAP, (LIST_CAP, LIST_CAP))
    add("brim", 1, b"AAAC" * LIST_CAP + b"G", ONE)
    add("brim", 2, (b"AAAC" + rand(rng, b"CGT", 116)) * LIST_CAP + b"G", ANY)
    # random AC + CCCC: the least word is AAAA, one candidate per run of four or more (one position in 32).  The reverse
    # complement is GGGG + random GT: as many runs of G
    add("random_full", 1, rand(rng, b"AC", 7100) + b"CCCC", (150, 400))
    add("random_full", 2, rand(rng, b"AC", 126_000) + b"CCCC", FULL)
    # AAAC / AAACC in random order: one candidate per block; the reverse complement's least word GGTT once per long block
    add("blocks_full", 1, _blocks(rng, 1100), (400, 700))
    add("blocks_full", 2, _blocks(rng, 27_400), FULL)
    # stalled rounds: every period holds one candidate and the candidates agree up to the seam, where the T loses to the
    # period's A (a seam that WINS there ends the rounds at once: STALLED_IN_NAME_ONLY).  Size two: 820 blocks of 150 bytes,
    # each with one run of A longer than any in its reverse complement (random ACG + G TTTT...)
    run = b"A" * 12 + b"C"
    add("stalled", 1, b"AACGT" * 700 + b"T", ONE)
    add("stalled", 2, (run + rand(rng, b"CGT", 137)) * 820 + b"T", ANY)
    # the same with few candidates: ten copies of a block (size one: no T in it, so the seam loses whatever the block)
    add("stalled_wave", 1, rand(rng, b"ACG", 400) * 10 + b"T", ANY)
    add("stalled_wave", 2, (run + rand(rng, b"CGT", 12_287)) * 10 + b"T", ANY)
    # closed repeat of a long block: with one candidate per copy the search restarts on the block (d = 2000, 30,720), with
    # more the candidates are not one block apart and the copies stay equal until the rounds give up
    add("closed_block", 1, _winner(rand(rng, b"ACGT", 2000) * 3), (2, LANES))
    add("closed_block", 1, (run + rand(rng, b"CGT", 1987)) * 3, ANY)
    add("closed_block", 2, (run + rand(rng, b"CGT", 30_707)) * 4, ANY)
    add("closed_block", 2, (run + rand(rng, b"CGT", 10_000) + run + rand(rng, b"CGT", 20_694)) * 4, ANY)
    # runs of the least byte
    add("run_single", 1, b"CGT" * 100 + b"A" * 200 + b"GTC" * 100, ANY)
    add("run_single", 2, rand(rng, b"CGT", 11_000) + b"A" * 100_000 + rand(rng, b"CGT", 12_000), ANY)
    add("run_origin", 1, b"A" * 60 + rand(rng, b"CGT", 500) + b"A" * 40, ANY)
    add("run_origin", 2, b"A" * 60_000 + rand(rng, b"CGT", 23_000) + b"A" * 40_000, ANY)
    add("run_two", 1, b"A" * 100 + b"C" * 50 + b"A" * 100 + b"G" * 70, ANY)
    add("run_two", 2, b"A" * 50_000 + b"C" * 10_000 + b"A" * 50_000 + b"G" * 12_880, ANY)
    add("homopolymer", 1, b"A" * 1000, (0, 0))
    add("homopolymer", 2, b"A" * GLOBAL_MIN, (0, 0))
    add("run_other", 1, _winner(b"C" * 300 + rand(rng, b"ACGT", 500)), ANY)
    add("run_other", 2, _winner(b"C" * 100_000 + rand(rng, b"ACGT", 23_000)), ANY)
    # the longest sequence LDS holds and the shortest it does not
    add("edge", 1, _winner(rand(rng, b"ACGT", WAVE_SEQ_MAX)), ANY)
    add("edge", 2, _winner(rand(rng, b"ACGT", GLOBAL_MIN)), ANY)
    return tuple(m)


@functools.lru_cache(maxsize=None)
def edge_below() -> bytes:
    """122,856 bytes: with its 24 wrapped bytes exactly the 120 KiB the LDS workgroup kernel stages"""
    return rand(np.random.default_rng(0x4B36), b"ACGT", GLOBAL_MIN - 1)


@functools.lru_cache(maxsize=None)
def inputs(size: int) -> tuple:
    """every member of that size and its reverse complement, as (name, bytes); size two: also the 122,856-byte pair"""
    out, seen = [], {}
    for mb in members():
        if mb.size == size:
            k = seen[mb.family] = seen.get(mb.family, 0) + 1
            out.append((f"{mb.family}.{k}", mb.seq))
            out.append((f"{mb.family}.{k}.rc", revcomp(mb.seq)))
    if size == 2:
        out += [("edge_below", edge_below()), ("edge_below.rc", revcomp(edge_below()))]
    return tuple(out)


def forward_wins_full_reverse(size: int):
    """the full-list inputs whose own strand is the smaller one while their reverse complement has more than 1,024
    candidates: the second strand's search is the hard one and its result does not reach the hash -- unless the input is
    fed as its reverse complement as well, which must give the same double-stranded hash"""
    return tuple((name, t) for name, t in inputs(size) if name.split(".")[0] in ("open_full", "closed_full", "blocks_full")
                 and candidates(revcomp(t)) > LIST_CAP and orc.rotate_sequence(t) < orc.rotate_sequence(revcomp(t)))


def batches(size: int):
    """the inputs of a size as batches of (names, sequences): size one in one batch, size two by family"""
    ins = inputs(size)
    if size == 1:
        return [tuple(zip(*ins))]
    fams = []
    for name, _ in ins:
        f = name.split(".")[0]
        if f not in fams:
            fams.append(f)
    return [tuple(zip(*[(n, s) for n, s in ins if n.split(".")[0] == f])) for f in fams]


# ---------------------------------------------------------------- many short sequences
SMALL = ("closed", "closed_block", "open", "stalled_wave", "random_ac", "run", "homopolymer")


def small_kind(s: bytes) -> set:
    """the small families a sequence of up to 300 bytes belongs to"""
    c, closed, eq = candidates(s), 0 < period(s) < len(s), equal_bytes(s)
    k = set()
    if c == 0 and len(s) >= 4:
        k.add("homopolymer")
    if closed and c > LANES:
        k.add("closed")
    if closed and 2 <= c <= LANES:
        k.add("closed_block")
    if not closed and c > LANES and eq > 12:       # three rounds without a loss and more: the wave kernel's stall
        k.add("open")
    if not closed and 2 <= c <= LANES and eq > STALL_BYTES:
        k.add("stalled_wave")
    if not closed and c >= 2 and set(s) <= set(b"AC") and eq <= 64:
        k.add("random_ac")
    if c == 1 and len(s) >= 4 and int(words(s).min()) == 0x41414141:
        k.add("run")
    return k


def _small(rng, kind: str, n: int) -> bytes:
    """a member of a small family in at most max(n, 8) bytes (closed, open, stalled_wave: whatever n, 130 to 300 bytes)"""
    n = max(n, 8)
    if kind == "closed":
        unit = (b"AC", b"AAC", b"ACG")[int(rng.integers(0, 3))]
        return unit * min(300 // len(unit), max(66, n // len(unit)))
    if kind == "closed_block":
        blk = rand(rng, b"ACGT", max(4, n // int(rng.integers(2, 5))))
        return blk * max(2, n // len(blk))
    if kind == "open":
        return b"AC" * int(rng.integers(70, 148)) + (b"G", b"CT", b"T")[int(rng.integers(0, 3))]
    if kind == "stalled_wave":
        blk = b"AAC" + rand(rng, b"CGT", int(rng.integers(3, 12)))
        return blk * (298 // len(blk)) + b"G"
    if kind == "random_ac":
        return rand(rng, b"AC", n - 4) + b"CCCC"
    if kind == "run":
        body = rand(rng, b"CGT", n // 2)
        cut = int(rng.integers(0, len(body)))
        return body[:cut] + b"A" * (n // 2) + body[cut:]
    return rand(rng, b"ACGT", 1) * n   # homopolymer


SMALL_SHORT = ("closed_block", "random_ac", "run", "homopolymer")   # the families that fit a short slot


def _next_letter(c: int) -> bytes:
    return b"CGTA"[b"ACGT".index(c): b"ACGT".index(c) + 1]


@functools.lru_cache(maxsize=None)
def many_short(n_seq: int):
    """(sequences, kinds): n_seq sequences of 2 to 300 bytes, a few of 0 and 1; kinds[i] names the small family sequence i
    was drawn from ("" for random ACGT), about a tenth of them.  Long (150..300) and short (2..40) lengths alternate, in batch
    order -- what a workgroup's chunk of consecutive sequences sees -- and, by swapping the roles every 8,192 sequences,
    also between the sequences one wave of the persistent grid takes in turn.  No sequence of two or more bytes has equal
    strands (such a hash would not depend on the second strand's search)."""
    rng = np.random.default_rng(n_seq + 0x4B37)
    seqs, kinds = [], []
    for q in range(n_seq):
        long = (q + q // WAVE_STRIDE) % 2 == 0
        n = int(rng.integers(150, 301)) if long else int(rng.integers(2, 41))
        kind = ""
        if q % 997 == 13:
            n = q // 997 % 2                                   # 0 and 1
        elif rng.random() < 0.1:
            pool = SMALL if long else SMALL_SHORT
            kind = pool[int(rng.integers(0, len(pool)))]
        s = _small(rng, kind, n) if kind else rand(rng, b"ACGT", n)
        while len(s) >= 2 and orc.rotate_sequence(s) == orc.rotate_sequence(revcomp(s)):
            s, kind = s[:-1] + _next_letter(s[-1]), ""
        seqs.append(s)
        kinds.append(kind)
    return tuple(seqs), tuple(kinds)
