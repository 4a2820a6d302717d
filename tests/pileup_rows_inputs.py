"""Inputs of polyhip_pileup_rows (tests/test_pileup_rows_cpu.py and tests/test_pileup_rows_gpu.py share them): every set of
tests/pileup_qual_inputs.py (which holds those of tests/pileup_inputs.py) at its regions and min_mapq values, and sets of
their own for what only the text rows can get wrong: the decimal numbers, the order of the reads within a row, the '^' byte,
the name, runs across the region's edge.  What they hold is asserted in tests/test_pileup_rows_cpu.py.  Callers leave what
they get unchanged."""
from __future__ import annotations

import functools
from dataclasses import dataclass

import numpy as np

import pileup_inputs as pi
import pileup_qual_inputs as qi
from aln_records_inputs import runs

SEED = 909
RUN_LENGTHS = (9, 10, 99, 100)
DEPTHS = ((5, 9), (10, 10), (15, 99), (20, 100), (25, 300))       # (position, reads on it)
MAPQS = (0, 93, 94, 255)
DEFAULTS = dict(region=None, pos_origin=0, min_mapq=0, qual_offset=33, all_positions=0, order=None, name=b"seq1", mapq_null=False, rebase=0)


@dataclass(frozen=True)
class RowsSet:
    name: str
    qs: qi.QualSet          # entries, read_start, quals, ref
    settings: tuple         # dicts over DEFAULTS


def _settings(*changes):
    return tuple(dict(DEFAULTS, **c) for c in changes)


def _qualset(name, ents, text, seed) -> qi.QualSet:
    return qi.attach(pi.InputSet(name, tuple(ents), text, ()), seed)


# ---- the sets of the counts, at their regions and min_mapq values -------------------------------------------------------------------
def from_qual(s: qi.QualSet) -> RowsSet:
    seen, out = set(), []
    for st in s.settings:
        k = (st["region"], st["min_mapq"])
        if k not in seen:
            seen.add(k)
            out += [dict(region=k[0], min_mapq=k[1], all_positions=a) for a in (0, 1)]
    return RowsSet(s.name, s, _settings(*out))


# ---- run lengths whose decimal gains a digit --------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def run_lengths() -> RowsSet:
    rng = np.random.default_rng(SEED + 1)
    text = pi.random_text(rng, 1500)
    ents, at = [], 3
    for k in RUN_LENGTHS:
        for strand in (0, pi.REVERSE):
            cl = runs(("=", 5), ("I", k), ("=", 3), ("D", k), ("=", 4), ("I", k), ("D", k), ("=", 2))
            e = pi.on_text(f"runs{k}_{'reverse' if strand else 'forward'}", cl, text, at, rng, flags=pi.MAPPED | strand, mapq=30 + k % 7)
            ents.append(e)
            at = e.ref_end - k // 2                                           # the next entry overlaps the end of this one
    return RowsSet("run_lengths", _qualset("run_lengths", ents, text, 1), _settings({}, dict(all_positions=1), dict(region=(100, 400))))


# ---- positions where the printed number gains a digit ---------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def digits() -> RowsSet:
    rng = np.random.default_rng(SEED + 2)
    text = pi.random_text(rng, 1100)
    ents = [pi.on_text("at_9_10", "=" * 6, text, 6, rng), pi.on_text("at_99_100", "==X===", text, 96, rng, flags=pi.MAPPED | pi.REVERSE),
            pi.on_text("at_999_1000", "=" * 8, text, 994, rng), pi.on_text("to_the_end", "=" * 5, text, 1095, rng)]
    sets = [{}, dict(all_positions=1), dict(region=(990, 1010), all_positions=1), dict(region=(905, 1010), pos_origin=900),     # 99 -> 100 at 998 / 999
            dict(region=(995, 1005), pos_origin=990, all_positions=1),                                                         # 9 -> 10 at 998 / 999
            dict(region=(994, 1002), pos_origin=994)]                                                                         # pos_origin == region_lo: 1 ..
    return RowsSet("digits", _qualset("digits", ents, text, 2), _settings(*sets))


# ---- depths: every read of a row distinguishable, so a wrong order shows -------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def depths() -> RowsSet:
    rng = np.random.default_rng(SEED + 3)
    text = pi.random_text(rng, 40)
    ents = []
    for p, d in DEPTHS:
        for k in range(d):                                                     # (mapq, strand, class) differs between any two reads of a row
            ents.append(pi.on_text(f"p{p}_{k}", "X" if k // 180 else "=", text, p, rng, flags=pi.MAPPED | (pi.REVERSE if k // 90 % 2 else 0),
                                   mapq=k % 90))
    ents = [ents[int(k)] for k in rng.permutation(len(ents))]
    n = len(ents)
    orders = (tuple(int(x) for x in rng.permutation(n)), tuple(range(n)), tuple(range(n - 1, -1, -1)))
    return RowsSet("depths", _qualset("depths", ents, text, 3), _settings({}, *[dict(order=o) for o in orders], dict(order=orders[0], all_positions=1)))


# ---- tokens: head and tail in one, D columns only, runs across the region's edge, names, mapq bytes, another Phred offset ----------
@functools.lru_cache(maxsize=None)
def tokens() -> RowsSet:
    rng = np.random.default_rng(SEED + 4)
    text = pi.random_text(rng, 80)
    ents = [pi.on_text("one_column", "=", text, 3, rng, mapq=80), pi.on_text("one_column_reverse", "X", text, 3, rng, flags=pi.MAPPED | pi.REVERSE),
            pi.on_text("d_only", "DDD", text, 5, rng), pi.on_text("d_only_reverse", "DD", text, 6, rng, flags=pi.MAPPED | pi.REVERSE),
            pi.on_text("del", "====DDD===", text, 10, rng),                                   # anchor 13, deleted 14..16
            pi.on_text("ins", "====II====", text, 30, rng, flags=pi.MAPPED | pi.REVERSE),    # anchor 33
            pi.on_text("ins_then_del", "==IID==", text, 40, rng),                             # .+2xx-1x on 41
            pi.on_text("del_then_ins", "==DI==", text, 50, rng),                              # *+1x on 52
            pi.on_text("d_i_d", "===DID===", text, 60, rng, flags=pi.MAPPED | pi.REVERSE),
            pi.on_text("tail_ins", "===II", text, 70, rng), pi.on_text("tail_del", "===DD", text, 72, rng)]
    ents += [pi.on_text(f"mapq{m}", "===", text, 20, rng, mapq=m) for m in MAPQS]
    sets = [{}, dict(all_positions=1), dict(region=(13, 14)), dict(region=(14, 17)), dict(region=(33, 34)), dict(region=(34, 40)),
            dict(name=b"c"), dict(name=bytes(33 + k % 94 for k in range(255)), all_positions=1), dict(mapq_null=True),
            dict(qual_offset=64, rebase=31), dict(min_mapq=94), dict(region=(0, 0)), dict(region=(78, 80)), dict(region=(78, 80), all_positions=1)]
    return RowsSet("tokens", _qualset("tokens", ents, text, 4), _settings(*sets))


@functools.lru_cache(maxsize=None)
def own_sets() -> tuple:
    return (run_lengths(), digits(), depths(), tokens())


@functools.lru_cache(maxsize=None)
def existing_sets() -> tuple:
    return tuple(from_qual(s) for s in qi.all_sets())


def all_sets() -> tuple:
    return existing_sets() + own_sets()


@functools.lru_cache(maxsize=None)
def _packed(name: str, rebase: int):
    s = {x.name: x for x in all_sets()}[name]
    return qi.pack(s.qs, rebase=rebase)


def arguments(s: RowsSet, st: dict, with_qual: bool) -> tuple:
    """-> (the packed arrays with what the setting switches off set to None, keywords of the oracle)"""
    p = dict(_packed(s.name, st["rebase"]))
    if st["mapq_null"]:
        p["mapq"] = None
    if not with_qual:
        p.update(read_start=None, qual=None, qual_off=None)
    p["order"] = None if st["order"] is None else np.array(st["order"], np.uint32)
    kw = {k: st[k] for k in ("region", "pos_origin", "min_mapq", "qual_offset", "all_positions")}
    return p, kw
