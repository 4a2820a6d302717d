"""polyhip_demux_reads / polyhip_demux_pairs in plain Python loops: the definition in the comment above the calls in
include/polyhip.h, step by step, one byte at a time.  Nothing here is vectorised; numpy only holds the results."""
from types import SimpleNamespace

import numpy as np

NONE = 0xFFFFFFFF
F_NO_BARCODE, F_AMBIGUOUS, F_NOT_IN_SHEET = 1, 2, 4
INFO_FIELDS = ("reads", "assigned", "exact", "no_barcode", "ambiguous", "not_in_sheet", "bad", "bytes_in", "bytes_out")
DEFAULTS = dict(max_shift=0, max_mismatches=1, min_margin=1, clip=1, clip_extra=0)


def upper(c):
    return c - 32 if ord("a") <= c <= ord("z") else c


def distance(r, t, max_shift):
    """step 2: (d_t, s_t) of barcode t on read r, or None if no start fits"""
    best = None
    for s in range(max_shift + 1):
        if s + len(t) > len(r):
            break
        d = 0
        for k in range(len(t)):
            if upper(r[s + k]) != t[k]:      # t is upper-case ACGT: every other read byte differs from it
                d += 1
        if best is None or d < best[0]:
            best = (d, s)
    return best


def choose(r, barcodes, max_shift, max_mismatches, min_margin):
    """step 3: (barcode, bstart, mism, flags)"""
    dist = [distance(r, t, max_shift) for t in barcodes]
    t1 = None
    for t, x in enumerate(dist):
        if x is not None and (t1 is None or x[0] < dist[t1][0]):
            t1 = t
    if t1 is None or dist[t1][0] > max_mismatches:
        return NONE, NONE, NONE, F_NO_BARCODE
    d2 = None
    for t, x in enumerate(dist):
        if t != t1 and x is not None and (d2 is None or x[0] < d2):
            d2 = x[0]
    if d2 is not None and d2 - dist[t1][0] < min_margin:
        return NONE, NONE, NONE, F_AMBIGUOUS
    return t1, dist[t1][1], dist[t1][0], 0


def _entry(r, q, barcodes, P):
    """steps 1-3 of one entry: [barcode, bstart, mism, flags, err]; barcodes None: not judged against a set"""
    if q is not None and len(q) != len(r):
        return [NONE, NONE, NONE, 0, 1]
    if barcodes is None:
        return [NONE, NONE, NONE, 0, 0]
    return list(choose(r, barcodes, P["max_shift"], P["max_mismatches"], P["min_margin"])) + [0]


def _params(kw):
    unknown = set(kw) - set(DEFAULTS)
    assert not unknown, unknown
    return dict(DEFAULTS, **kw)


def _finish(units, samples, nsamples, reads, quals, sets, P):
    """steps 5 and 6.  units[i]: the entries of read or pair i; samples[i]: its sample or NONE; reads / quals / sets: per mate"""
    n, nb = len(units), len(reads)
    group = [nsamples if samples[i] == NONE else samples[i] for i in range(n)]
    order = sorted(range(n), key=lambda i: group[i])                   # sorted() is stable
    sample_start = [sum(1 for g in group if g < k) for k in range(nsamples + 2)] if nsamples <= 300 else None
    if sample_start is None:                                           # the same numbers without the n * nsamples loop
        count = [0] * (nsamples + 2)
        for g in group:
            count[g + 1] += 1
        sample_start = [0] * (nsamples + 2)
        for k in range(1, nsamples + 2):
            sample_start[k] = sample_start[k - 1] + count[k]
    info = dict.fromkeys(INFO_FIELDS, 0)
    info["reads"] = n * nb
    out = [dict(seqs=bytearray(), quals=bytearray() if quals[q] is not None else None, offsets=[0]) for q in range(nb)]
    for i in order:
        for q in range(nb):
            r, (b, s, _, _, er) = reads[q][i], units[i][q]
            a = 0
            if b != NONE and samples[i] != NONE and P["clip"]:
                a = min(len(r), s + len(sets[q][b]) + P["clip_extra"])
            if er:
                a = len(r)
            o = out[q]
            o["seqs"] += r[a:]
            if o["quals"] is not None:
                o["quals"] += quals[q][i][a:len(r)] if not er else b""
            o["offsets"].append(len(o["seqs"]))
    for i in range(n):
        info["assigned"] += nb if samples[i] != NONE else 0
        for q in range(nb):
            b, _, d, f, er = units[i][q]
            info["exact"] += b != NONE and d == 0
            info["no_barcode"] += bool(f & F_NO_BARCODE)
            info["ambiguous"] += bool(f & F_AMBIGUOUS)
            info["not_in_sheet"] += bool(f & F_NOT_IN_SHEET)
            info["bad"] += bool(er)
            info["bytes_in"] += len(reads[q][i])
    info["bytes_out"] = sum(len(o["seqs"]) for o in out)
    flat = [e for u in units for e in u]
    col = lambda k: np.array([e[k] for e in flat], np.uint32)          # noqa: E731
    conv = [(np.frombuffer(bytes(o["seqs"]), np.uint8), np.array(o["offsets"], np.uint64),
             None if o["quals"] is None else np.frombuffer(bytes(o["quals"]), np.uint8)) for o in out]
    return SimpleNamespace(barcode=col(0), bstart=col(1), mism=col(2), flags=col(3), err=col(4), sample=np.array(samples, np.uint32),
                           order=np.array(order, np.uint32), sample_start=np.array(sample_start, np.uint64), nsamples=nsamples,
                           info=info), conv


def demux_reads(reads, barcodes, quals=None, **kw):
    """reads: list of bytes; quals: list of bytes or None -> the fields of demux.Demuxed, and info"""
    P = _params(kw)
    barcodes = [bytes(b) for b in barcodes]
    units = [[_entry(reads[i], None if quals is None else quals[i], barcodes, P)] for i in range(len(reads))]
    samples = [u[0][0] for u in units]                                 # step 4: the barcode is the sample
    res, conv = _finish(units, samples, len(barcodes), [reads], [quals], [barcodes], P)
    res.seqs, res.offsets, res.quals = conv[0]
    return res


def demux_pairs(reads1, reads2, barcodes1, barcodes2=(), pair_sample=None, nsamples=None, quals1=None, quals2=None, **kw):
    """pair_sample: a flat list of len(barcodes1) * len(barcodes2) samples, NONE for a hole"""
    P = _params(kw)
    assert len(reads1) == len(reads2)
    set1, set2 = [bytes(b) for b in barcodes1], [bytes(b) for b in barcodes2]
    if not set2:
        nsamples = len(set1)
    units, samples = [], []
    for i in range(len(reads1)):
        u = [_entry(reads1[i], None if quals1 is None else quals1[i], set1, P),
             _entry(reads2[i], None if quals2 is None else quals2[i], set2 if set2 else None, P)]
        smp = NONE
        if not u[0][4] and not u[1][4] and u[0][0] != NONE and (not set2 or u[1][0] != NONE):
            if set2:
                smp = pair_sample[u[0][0] * len(set2) + u[1][0]]
                if smp == NONE:
                    u[0][3] |= F_NOT_IN_SHEET
                    u[1][3] |= F_NOT_IN_SHEET
            else:
                smp = u[0][0]
        units.append(u)
        samples.append(smp)
    res, conv = _finish(units, samples, nsamples, [reads1, reads2], [quals1, quals2], [set1, set2], P)
    res.seqs, res.offsets, res.quals = (conv[0][0], conv[1][0]), (conv[0][1], conv[1][1]), (conv[0][2], conv[1][2])
    return res
