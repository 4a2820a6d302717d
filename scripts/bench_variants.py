"""polyhip_call_variants on one MI355X beside polyhip_pileup_qual, in one run.

    python scripts/bench_variants.py [--genome 5000000] [--reads 1000000] [--reps 5] [--only-variants]
                                     [--out profiles/variants_bench.json]
    python scripts/bench_variants.py --summarise-db x_results.db > profiles/variants_kernel_stats.md  (no GPU)
    python scripts/bench_variants.py --merge-trace profiles/variants_kernel_stats.md --out profiles/variants_bench.json

- workload: scripts/bench_pileup_rows.py's, with a sample that differs from the text: a synthetic genome with a short repeat
  (a unit of 1..3 bases, 4..8 copies) planted behind every second indel site, a sample with one planted variant about every
  2 kb (two thirds SNVs, the rest insertions and deletions of 1..8 bases, in a repeat one unit of it), reads of 150 bp drawn
  from the sample with 5 % substitutions and 1 % indels, mapped once by polyhip_map_reads_affine, the records made once, 150
  quality bytes per read with about a tenth of the bases below 20;
- polyhip_pileup_qual and polyhip_call_variants (with the qualities, left_align = 1) over the whole text, the same settings,
  alternate --reps times after a warm-up round, through the host-pointer calls; a host clock around each call, which includes
  the uploads, the device allocations and the copies back; medians.  The record and allele buffers have the exact sizes, asked
  for once before the clock starts;
- recovery: a planted variant counts when a record has its position, kind and allele exactly, the position being the
  leftmost one the text allows; counted with left_align = 1 and with left_align = 0;
- checks: the SNV records equal polyhip_pileup_qual's SNV sites of the same run; a window of 4,000 positions, run as a region of
  its own, equals tests/variants_oracle.py;
- the kernels' own time is not taken here: run the script under a kernel trace in a run of its own (--only-variants --reps 1),
  never together with counters, summarise its database with --summarise-db and hand the table back with --merge-trace.
Prints one JSON object (and writes it to --out).  Nothing here has a speed threshold.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

VARIANTS_KERNELS = ("walk_kernel", "snv_kernel", "event_kernel", "wordkey_kernel", "mainkey_kernel", "head_kernel",
                    "start_kernel", "allele_kernel", "radix_hist_kernel", "radix_scatter_kernel")      # and the scan_* kernels
SPACING = 2000


def plant(rng, text):
    """-> (text with the repeats planted, sample, [(leftmost position or anchor, kind, bytes or deleted length)])"""
    text = text.copy()
    n = len(text)
    sites = []
    for p in range(SPACING // 2, n - SPACING // 2, SPACING):
        p += int(rng.integers(0, SPACING // 4))
        kind = 1 if rng.random() < 2 / 3 else int(rng.integers(2, 4))
        unit = None
        if kind != 1 and rng.random() < 0.5:
            unit = text[p + 1:p + 1 + int(rng.integers(1, 4))].copy()
            copies = int(rng.integers(4, 9))
            text[p + 1:p + 1 + len(unit) * copies] = np.tile(unit, copies)
        sites.append((p, kind, unit))
    T = text.tobytes()
    parts, planted, at = [], [], 0
    for p, kind, unit in sites:
        if kind == 1:
            alt = b"CGTA"[b"ACGT".index(T[p])]
            parts += [T[at:p], bytes([alt])]
            at = p + 1
            planted.append((p, 1, bytes([alt])))
            continue
        body = unit.tobytes() if unit is not None else None
        if kind == 2:
            body = body or bytes(b"ACGT"[int(x)] for x in rng.integers(0, 4, int(rng.integers(1, 9))))
            parts += [T[at:p + 1], body]
            at = p + 1
            a = p
            while a >= 0 and T[a] == body[-1]:                    # the leftmost spelling of the same sample
                body = bytes([T[a]]) + body[:-1]
                a -= 1
            planted.append((a, 2, body))
        else:
            l = len(body) if body else int(rng.integers(1, 9))
            parts += [T[at:p + 1]]
            at = p + 1 + l
            a = p
            while a >= 0 and T[a] == T[a + l]:
                a -= 1
            planted.append((a, 3, l))
    sample = np.frombuffer(b"".join(parts + [T[at:]]), np.uint8)
    return text, sample, planted


def found(records, alleles):
    out = set()
    for r in records:
        k = int(r["kind"])
        o, l = int(r["allele_off"]), int(r["allele_len"])
        out.add((int(r["pos"]), k, bytes([int(r["alt"])]) if k == 1 else alleles[o:o + l].tobytes() if k == 2 else l))
    return out


def run(dev, n, N, reps, only_variants):
    import torch
    from bench_map import make_reads
    from bench_pileup_rows import _alternate
    from poly_amd import _lib, align, alphabet, bwt, mapper, mash, matrix, pileup, sam, variants
    import variants_oracle as vo
    rng = np.random.default_rng(17)
    m = 150
    P = mapper.MapParams()
    ab = alphabet.NewAlphabet(list("-ACGT"))
    sc = align.NewScoring(matrix.NewSubstitutionMatrix(ab, ab, matrix.NUC_4), -2)
    g_t = torch.empty(n, dtype=torch.uint8, device=dev)
    mash.synth_dna_dev(0x5EED + n, g_t)
    text, sample, planted = plant(rng, np.ascontiguousarray(g_t.cpu().numpy()))
    g_t = torch.from_numpy(text).to(dev)
    idx = bwt.new_dev(g_t)
    reads = make_reads(rng, sample, N, m)
    buf = reads.reshape(-1)
    offs = np.arange(0, N * m + 1, m, dtype=np.uint64)
    cap = 2 * N * m
    lib, p = _lib.lib(), P._c()
    score, second = np.zeros(N, np.int64), np.zeros(N, np.int64)
    u32 = [np.zeros(N, np.uint32) for _ in range(7)]
    flags, votes, ref_start, ref_end, read_start, read_end, err = u32
    alnA, alnB, aoff = np.zeros(cap, np.uint8), np.zeros(cap, np.uint8), np.zeros(N + 1, np.uint64)
    _lib.check(lib.polyhip_map_reads_affine(idx.handle(), sc.handle(), C.byref(p), -5, -2, buf.ctypes.data, offs.ctypes.data, N, m, 0,
                                            score.ctypes.data, second.ctypes.data, *[x.ctypes.data for x in u32], alnA.ctypes.data,
                                            alnB.ctypes.data, aoff.ctypes.data, cap))
    read_len = np.full(N, m, np.uint32)
    rp = sam._CParams(0, 0)
    coff, moff = np.zeros(N + 1, np.uint64), np.zeros(N + 1, np.uint64)
    nm, sf, rerr, mapq = np.zeros(N, np.uint32), np.zeros(N, np.uint32), np.zeros(N, np.uint32), np.zeros(N, np.uint8)
    rc = lib.polyhip_aln_records(C.byref(rp), N, flags.ctypes.data, score.ctypes.data, second.ctypes.data, read_start.ctypes.data,
                                 read_end.ctypes.data, read_len.ctypes.data, alnA.ctypes.data, alnB.ctypes.data, aoff.ctypes.data,
                                 coff.ctypes.data, None, 0, moff.ctypes.data, None, 0, nm.ctypes.data, mapq.ctypes.data, sf.ctypes.data,
                                 rerr.ctypes.data)                  # the sizes: mapq is filled either way
    assert rc in (_lib.OK, _lib.ERR_INVALID)
    qual = np.where(rng.random(N * m) < 0.1, rng.integers(2, 20, N * m), rng.integers(20, 42, N * m)).astype(np.uint8) + np.uint8(33)
    qoff = offs
    settings = dict(min_mapq=20, min_depth=4, min_alt_count=2, min_alt_permille=300)
    base = pileup._CParams(0, n, *[settings[k] for k in ("min_mapq", "min_depth", "min_alt_count", "min_alt_permille")])

    qerr, nsites = np.zeros(N, np.uint32), C.c_uint64(0)
    qcounts, qsum, qcons = np.zeros((pileup.CHANNELS, n), np.uint32), np.zeros((pileup.QSUM_PLANES, n), np.uint32), np.zeros(n, np.uint8)
    scap = 1 << 21
    qsites = np.zeros(scap, pileup.SITE_DTYPE)

    def with_qual():
        qp = pileup._CQualParams(base, 20, 33)
        _lib.check(lib.polyhip_pileup_qual(C.byref(qp), N, flags.ctypes.data, mapq.ctypes.data, ref_start.ctypes.data, ref_end.ctypes.data,
                                           read_start.ctypes.data, alnA.ctypes.data, alnB.ctypes.data, aoff.ctypes.data, qual.ctypes.data,
                                           qoff.ctypes.data, text.ctypes.data, n, qcounts.ctypes.data, qsum.ctypes.data, qcons.ctypes.data,
                                           C.byref(nsites), qsites.ctypes.data, scap, qerr.ctypes.data))

    verr, nvar, nbytes = np.zeros(N, np.uint32), C.c_uint64(0), C.c_uint64(0)

    def var_call(lo, hi, left_align, rec, rcap, pool, pcap, cparams=None):
        b = pileup._CParams(lo, hi, *[settings[k] for k in ("min_mapq", "min_depth", "min_alt_count", "min_alt_permille")]) if cparams is None \
            else cparams
        cp = variants._CVarParams(pileup._CQualParams(b, 20, 33), left_align, 800, 0, 0)
        return lib.polyhip_call_variants(C.byref(cp), N, flags.ctypes.data, mapq.ctypes.data, ref_start.ctypes.data, ref_end.ctypes.data,
                                         read_start.ctypes.data, alnA.ctypes.data, alnB.ctypes.data, aoff.ctypes.data, qual.ctypes.data,
                                         qoff.ctypes.data, text.ctypes.data, n, C.byref(nvar), None if rec is None else rec.ctypes.data, rcap,
                                         C.byref(nbytes), None if pool is None else pool.ctypes.data, pcap, verr.ctypes.data)

    def sized(left_align, cparams=None, lo=0, hi=n):
        assert var_call(lo, hi, left_align, None, 0, None, 0, cparams) in (_lib.OK, _lib.ERR_INVALID)          # the sizes
        nv, nb = int(nvar.value), int(nbytes.value)
        rec, pool = np.zeros(max(nv, 1), variants.VARIANT_DTYPE), np.zeros(max(nb, 1), np.uint8)
        _lib.check(var_call(lo, hi, left_align, rec, nv, pool, nb, cparams))
        return rec[:nv], pool[:nb]

    rec, pool = sized(1)
    nv, nb = len(rec), len(pool)
    calls = {"call_variants": lambda: _lib.check(var_call(0, n, 1, rec, nv, pool, nb))}
    if not only_variants:
        calls = {"pileup_qual": with_qual, **calls}
    med, times = _alternate(calls, reps, torch.cuda.synchronize)
    info = variants.last_info()
    key_bits = 9 + max(n - 1, 1).bit_length()
    result = {"genome": n, "reads": N, "read_len": m, "settings": dict(settings, min_base_qual=20, left_align=1, hom_permille=800, max_indel=255),
              "seconds": med, "seconds_all": times, "info": info, "events": info["events"], "alleles": info["alleles"], "records": nv,
              "allele_bytes": nb, "sort_key_bits": key_bits, "sort_passes_main_key": (key_bits + 7) // 8}
    strings = int(aoff[N])
    bytes_in = 2 * strings + n + 8 * (N + 1) + N * (3 * 4 + 1) + N * m + 8 * (N + 1) + 4 * N
    result.update(bytes_in=bytes_in, bytes_out=40 * nv + nb + 4 * N, planes_not_returned_bytes=(pileup.CHANNELS + pileup.QSUM_PLANES) * 4 * n)
    if only_variants:
        return result
    result["variants_over_pileup_qual"] = med["call_variants"] / med["pileup_qual"]
    # the longest insertion among the covered positions: what the byte passes of the sort are sized by
    every, every_pool = sized(1, pileup._CParams(0, n, settings["min_mapq"], 1, 1, 0))
    longest = int(every["allele_len"][every["kind"] == 2].max(initial=0))
    result.update(longest_insertion=longest, sort_word_passes=(longest + 7) // 8, sort_passes_bytes=8 * ((longest + 7) // 8))
    # recovery of the planted variants, with and without left alignment
    want = set(planted)
    for la in (1, 0):
        r, a = (rec, pool) if la else sized(0)
        got = found(r, a)
        hit = {k: sum(1 for v in want if v[1] == k and v in got) for k in (1, 2, 3)}
        total = {k: sum(1 for v in want if v[1] == k) for k in (1, 2, 3)}
        # what became of the missed ones: by length, and how many have a record of their kind within 20 positions (another spelling)
        missed = sorted(v for v in want if v not in got)
        length = lambda v: len(v[2]) if v[1] == 2 else v[2] if v[1] == 3 else 1      # noqa: E731
        by_len = {}
        for v in missed:
            by_len[f"{v[1]}:{length(v)}"] = by_len.get(f"{v[1]}:{length(v)}", 0) + 1
        pos_of = {k: np.sort(r["pos"][r["kind"] == k].astype(np.int64)) for k in (1, 2, 3)}
        near_miss = sum(1 for v in missed if len(pos_of[v[1]]) and np.abs(pos_of[v[1]] - v[0]).min() <= 20)
        result[f"recovered_left_align_{la}"] = dict(planted=len(want), recovered=sum(hit.values()), share=sum(hit.values()) / len(want),
                                                    by_kind={str(k): [hit[k], total[k]] for k in (1, 2, 3)}, records=len(r),
                                                    records_not_planted=len(got - want), missed_by_kind_and_length=by_len,
                                                    missed_with_a_record_nearby=near_miss,
                                                    missed_examples=[(v[0], v[1], v[2].decode() if v[1] != 3 else v[2]) for v in missed[:6]],
                                                    unplanted_examples=[(v[0], v[1], v[2].decode() if v[1] != 3 else v[2])
                                                                        for v in sorted(got - want)[:6]])
    # around the first missed indels: the text and every allele the reads show there, whatever its count
    context = []
    for v in [v for v in sorted(want - found(rec, pool)) if v[1] != 1][:4]:
        near = every[(every["pos"].astype(np.int64) >= v[0] - 12) & (every["pos"].astype(np.int64) <= v[0] + 30) & (every["kind"] != 1)]
        context.append(dict(planted=(v[0], v[1], v[2].decode() if v[1] == 2 else v[2]), text=text[v[0] - 12:v[0] + 40].tobytes().decode(),
                            alleles=[(int(x["pos"]), int(x["kind"]), int(x["allele_len"]), int(x["count"]), int(x["depth"]),
                                      every_pool[int(x["allele_off"]):int(x["allele_off"]) + int(x["allele_len"])].tobytes().decode()
                                      if x["kind"] == 2 else "") for x in near]))
    result["missed_context"] = context
    # the SNV records against polyhip_pileup_qual's SNV sites of the same run
    with_qual()
    sites = qsites[:int(nsites.value)]
    snv, ssnv = rec[rec["kind"] == 1], sites[sites["kind"] == 1]
    result["snv_equal_sites"] = len(snv) == len(ssnv) and all(bool((snv[f] == ssnv[f]).all()) for f in ("pos", "depth", "count", "count_fwd", "alt"))
    # a window, run as a region of its own, against the oracle on the entries that touch it
    lo, hi = n // 5, n // 5 + 4000
    near = np.nonzero(((flags & 1) == 1) & (ref_start <= hi) & (ref_end >= lo))[0]
    cols = np.diff(aoff.astype(np.int64))
    a_all, b_all, q_all = alnA.tobytes(), alnB.tobytes(), qual.tobytes()
    sub_off = np.zeros(len(near) + 1, np.uint64)
    sub_off[1:] = np.cumsum(cols[near])
    sub_q = np.arange(0, len(near) * m + 1, m, dtype=np.uint64)
    expect = vo.call_variants(flags[near], mapq[near], ref_start[near], ref_end[near], read_start[near],
                              b"".join(a_all[int(aoff[i]):int(aoff[i + 1])] for i in near),
                              b"".join(b_all[int(aoff[i]):int(aoff[i + 1])] for i in near), sub_off,
                              b"".join(q_all[int(i) * m:(int(i) + 1) * m] for i in near), sub_q, text.tobytes(), region=(lo, hi), min_base_qual=20,
                              left_align=1, hom_permille=800, **settings)
    wrec, wpool = sized(1, lo=lo, hi=hi)
    inside = rec[(rec["pos"] >= lo) & (rec["pos"] < hi)]
    plain = [f for f in variants.VARIANT_DTYPE.names if f != "allele_off"]
    result["spot_check"] = wrec.tobytes() == expect.records.tobytes() and wpool.tobytes() == expect.alleles.tobytes() and \
        len(inside) == len(wrec) and all(bool((inside[f] == wrec[f]).all()) for f in plain)
    result["spot_entries"], result["spot_records"] = int(len(near)), int(len(wrec))
    return result


def merge_trace(stats_path, out_path):
    """adds the kernels' time per polyhip_call_variants call, from the table --summarise-db wrote for a run of --only-variants, to
    the JSON of the timing run"""
    with open(out_path) as f:
        out = json.load(f)
    kernels, total_ms = {}, 0.0
    with open(stats_path) as f:
        for line in f:
            mt = re.match(r"\| `([^`]+)` \| (\d+) \| ([0-9.]+) \| ([0-9.]+) \|", line)
            base = mt.group(1).split("::")[-1].split("<")[0] if mt else ""
            if mt and (base in VARIANTS_KERNELS or base.startswith("scan_")):
                kernels[mt.group(1)] = {"calls": int(mt.group(2)), "total_ms": float(mt.group(3))}
                total_ms += float(mt.group(3))
    calls = next((v["calls"] for k, v in kernels.items() if "head_kernel" in k), 0)
    assert calls, "the table holds no head_kernel: it is not a trace of polyhip_call_variants"
    # an upper bound: the sort and scan kernels of the run's set-up (index build, mapping) carry the same names and are counted in,
    # and so is the size call, which runs everything but the two emit kernels
    per_call = total_ms / calls
    out["variants"]["kernel_trace"] = {"source": os.path.basename(stats_path), "calls_traced": calls, "kernels": kernels,
                                       "kernel_ms_per_call_upper_bound": per_call,
                                       "kernel_share_of_call": per_call / 1e3 / out["variants"]["seconds"]["call_variants"]}
    with open(out_path, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out["variants"]["kernel_trace"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genome", type=int, default=5_000_000)
    ap.add_argument("--reads", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only-variants", action="store_true", help="polyhip_call_variants alone and no checks: for a kernel trace")
    ap.add_argument("--merge-trace", default=None, help="a table of --summarise-db to add to --out; runs nothing")
    ap.add_argument("--summarise-db", default=None, help="a rocprofv3 results.db: prints its kernel table; runs nothing")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.summarise_db:
        from bench_pileup_rows import summarise_db
        return summarise_db(args.summarise_db, "polyhip_call_variants alone (--only-variants --reps 1), kernel trace of a run of its own")
    if args.merge_trace:
        return merge_trace(args.merge_trace, args.out)
    import torch
    assert torch.cuda.is_available(), "bench_variants.py measures on the GPU; there is no CPU path"
    dev = torch.device("cuda:0")
    out = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "workloads_measured": 1, "runs": 1,
           "variants": run(dev, args.genome, args.reads, args.reps, args.only_variants)}
    print(json.dumps(out))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")
    r = out["variants"]
    assert all(r.get(k, True) for k in ("snv_equal_sites", "spot_check")), "the records differ"


if __name__ == "__main__":
    main()
