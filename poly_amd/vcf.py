"""VCF text from the records of ``poly_amd.variants``: a writer, a parser of what the writer produces, and ``apply``, which puts
called variants into a text.  Host work only: the records come from polyhip_call_variants, nothing is called here.

One line per record and allele, VCFv4.2.  POS is 1-based; for an insertion and a deletion it is the anchor, the base in front of
the event, and REF and ALT are spelled with that base: ``A -> ATG`` inserts TG behind it, ``ACG -> A`` deletes CG.  QUAL is
``.``; INFO carries DP, the sample column GT (0/1 or 1/1), AD (reads without an event of the kind, reads with the allele) and
ADF (the allele's reads on the forward strand).
"""
from __future__ import annotations

from typing import NamedTuple

KIND_SNV, KIND_INS, KIND_DEL = 1, 2, 3
HEADER_FIELDS = ("##INFO=<ID=DP,Number=1,Type=Integer,Description=\"Reads covering the position\">",
                 "##FORMAT=<ID=GT,Number=1,Type=String,Description=\"Genotype\">",
                 "##FORMAT=<ID=AD,Number=R,Type=Integer,Description=\"Reads for the reference and for the allele\">",
                 "##FORMAT=<ID=ADF,Number=A,Type=Integer,Description=\"Reads for the allele on the forward strand\">")


class Row(NamedTuple):
    """one VCF line: ``pos`` 0-based (the anchor for an indel), ``ref`` and ``alt`` as the line spells them, ``gt`` 1 = 0/1, 2 = 1/1"""
    chrom: str
    pos: int
    ref: bytes
    alt: bytes
    depth: int
    ref_count: int
    count: int
    count_fwd: int
    gt: int


def _bytes(x) -> bytes:
    return x.encode("latin-1") if isinstance(x, str) else bytes(x)


def rows(variants, ref, name) -> list:
    """the records of a ``variants.Variants`` as Rows, REF spelled from the text ``ref`` the positions count in"""
    ref = _bytes(ref)
    name = name if isinstance(name, str) else bytes(name).decode("latin-1")
    if variants.records is None:
        raise ValueError("vcf.rows: the call delivered no records")
    out = []
    for i, r in enumerate(variants.records):
        p, kind, l = int(r["pos"]), int(r["kind"]), int(r["allele_len"])
        if kind == KIND_SNV:
            ref_allele, alt = ref[p:p + 1], bytes([int(r["alt"])])
        elif kind == KIND_INS:
            ref_allele, alt = ref[p:p + 1], ref[p:p + 1] + variants.inserted(i)
        elif kind == KIND_DEL:
            ref_allele, alt = ref[p:p + 1 + l], ref[p:p + 1]
        else:
            raise ValueError(f"vcf.rows: record {i} has kind {kind}")
        if len(ref_allele) != (1 + l if kind == KIND_DEL else 1):
            raise ValueError(f"vcf.rows: record {i} at {p} reaches beyond the text of {len(ref)} bytes")
        out.append(Row(name, p, ref_allele, alt, int(r["depth"]), int(r["ref_count"]), int(r["count"]), int(r["count_fwd"]), int(r["gt"])))
    return out


def _header(contigs, sample: str) -> list:
    lines = ["##fileformat=VCFv4.2"] + [f"##contig=<ID={n},length={length}>" for n, length in contigs] + list(HEADER_FIELDS)
    return lines + ["#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t" + sample]


def _line(r: Row) -> str:
    return "\t".join((r.chrom, str(r.pos + 1), ".", r.ref.decode("latin-1"), r.alt.decode("latin-1"), ".", ".", f"DP={r.depth}", "GT:AD:ADF",
                      f"{'1/1' if r.gt == 2 else '0/1'}:{r.ref_count},{r.count}:{r.count_fwd}"))


def write(variants, ref, name, sample: str = "sample") -> bytes:
    """the VCF text of one ``variants.Variants`` on the text ``ref`` named ``name``"""
    name = name if isinstance(name, str) else bytes(name).decode("latin-1")
    lines = _header([(name, len(_bytes(ref)))], sample) + [_line(r) for r in rows(variants, ref, name)]
    return ("\n".join(lines) + "\n").encode("latin-1")


def write_refs(per_contig: dict, refs, sample: str = "sample") -> bytes:
    """one header naming every contig of the ``refs.RefSet`` and, in contig order, the lines of each ``variants.call_refs`` result
    in ``per_contig`` (contig index -> Variants)"""
    lines = _header([(n, int(length)) for n, length in zip(refs.names, refs.lengths)], sample)
    for c in sorted(per_contig):
        v = per_contig[c]
        lines += [_line(r) for r in rows(v, v.ref.tobytes(), refs.names[c])]
    return ("\n".join(lines) + "\n").encode("latin-1")


def parse(text) -> list:
    """the Rows of a text that ``write`` or ``write_refs`` produced"""
    out = []
    for k, line in enumerate(_bytes(text).decode("latin-1").split("\n")):
        if not line or line.startswith("#"):
            continue
        f = line.split("\t")
        if len(f) != 10 or f[8] != "GT:AD:ADF" or not f[7].startswith("DP="):
            raise ValueError(f"vcf.parse: line {k + 1} is not one that vcf.write produces")
        gt, ad, adf = f[9].split(":")
        if gt not in ("0/1", "1/1"):
            raise ValueError(f"vcf.parse: line {k + 1} has the genotype {gt}")
        ref_count, count = ad.split(",")
        out.append(Row(f[0], int(f[1]) - 1, f[3].encode("latin-1"), f[4].encode("latin-1"), int(f[7][3:]), int(ref_count), int(count),
                       int(adf), 2 if gt == "1/1" else 1))
    return out


def apply(ref, variants, min_gt: int = 2, name: str = "") -> bytes:
    """``ref`` with the variants of genotype ``min_gt`` or above put in: ``variants`` is a ``variants.Variants`` or a list of Rows
    (of one sequence).  Two of them that touch the same text bytes are a ValueError."""
    ref = _bytes(ref)
    todo = rows(variants, ref, name) if hasattr(variants, "records") else list(variants)
    todo = sorted((r for r in todo if r.gt >= min_gt), key=lambda r: r.pos)
    out, at = [], 0
    for r in todo:
        if r.pos < at:
            raise ValueError(f"vcf.apply: the variant at {r.pos} overlaps the one before it")
        if ref[r.pos:r.pos + len(r.ref)] != r.ref:
            raise ValueError(f"vcf.apply: REF of the variant at {r.pos} is not what the text holds there")
        out += [ref[at:r.pos], r.alt]
        at = r.pos + len(r.ref)
    return b"".join(out + [ref[at:]])
