#!/usr/bin/env python3
"""Regenerates the fixture files in tests/golden/ from the reference checkout.

Run in the authoring container only (needs /root/reference); the outputs are
committed so that nothing at test/bench time reads /root/reference.

  phix174.seq  <- data/phix174.gb   (BASELINE config 1 input; 5,386 bp, lower case)
  puc19.seq    <- data/puc19.gbk    (seqhash_test.go:68-91 rotation fixture)
  fastq/*.fastq <- io/fastq/data/*.fastq  (verbatim copies of the reference's own parser fixtures:
                   fastq_test.go:59-66, example_test.go:16-66)
  fasta/base.fasta <- io/fasta/data/base.fasta  (example_test.go:18-36,100-114)
  clone_goldengate_rotated.seq <- the `// Output:` line of clone/example_test.go:11-31 (ExampleGoldenGate prints
                   seqhash.RotateSequence(Clones[0])): a 4.4 kb circular construct already at its least rotation

  clone_parts.json <- the clone.Part literals of clone/clone_test.go and clone/example_test.go
  matrices.json <- search/align/matrix/matrices.go: every canned table as {name: {"alphabet", "scores"}}

Extraction follows io/genbank/genbank.go:125,627-633: every line between
ORIGIN and // with all non-letters removed, case preserved.
"""
import os
import re
import sys

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))


def genbank_sequence(path: str) -> str:
    seq, on = [], False
    with open(path) as f:
        for line in f:
            if line.startswith("ORIGIN"):
                on = True
                continue
            if on:
                if line.startswith("//"):
                    break
                seq.append(re.sub(r"[^a-zA-Z]+", "", line))
    return "".join(seq)


def main() -> int:
    for src, dst in (("data/phix174.gb", "phix174.seq"), ("data/puc19.gbk", "puc19.seq")):
        s = genbank_sequence(os.path.join(REF, src))
        with open(os.path.join(HERE, dst), "w") as f:
            f.write(s + "\n")
        print(dst, len(s))
    return 0


def copy_fastq():
    import glob
    import shutil
    dst = os.path.join(HERE, "fastq")
    os.makedirs(dst, exist_ok=True)
    for f in sorted(glob.glob(os.path.join(REF, "io", "fastq", "data", "*.fastq"))):
        shutil.copy(f, dst)
    os.makedirs(os.path.join(HERE, "fasta"), exist_ok=True)
    shutil.copy(os.path.join(REF, "io", "fasta", "data", "base.fasta"), os.path.join(HERE, "fasta"))


def matrices():
    """every table of search/align/matrix/matrices.go -> matrices.json: {name: {"alphabet": "-ACGT", "scores": [[...]]}}.
    A table's alphabet is its `/*  - A C G T */` header comment (rows and columns in that order); only names, alphabets
    and integers are kept."""
    import json
    with open(os.path.join(REF, "search", "align", "matrix", "matrices.go")) as f:
        src = f.read()
    out = {}
    for m in re.finditer(r"^\t(\w+) = \[\]\[\]int\{\n(.*?)^\t\}", src, flags=re.M | re.S):
        name, body = m.group(1), m.group(2).split("\n")
        alphabet = "".join(re.fullmatch(r"\s*/\*\s*(.*?)\s*\*/\s*", body[0]).group(1).split())
        rows = []
        for line in body[1:]:
            r = re.fullmatch(r"\s*/\* (\S) \*/ \{([-\d, ]*)\},\s*", line)
            if r is None:
                assert not line.strip(), (name, line)
                continue
            assert r.group(1) == alphabet[len(rows)], (name, line)
            rows.append([int(v) for v in r.group(2).split(",")])
        assert len(rows) == len(alphabet) and all(len(r) == len(alphabet) for r in rows), name
        out[name] = {"alphabet": alphabet, "scores": rows}
    assert len(out) == 78, len(out)
    with open(os.path.join(HERE, "matrices.json"), "w") as f:
        json.dump(out, f, separators=(",", ":"))
        f.write("\n")
    print("matrices.json", len(out))


def clone_example_output():
    """the expected output of ExampleGoldenGate (clone/example_test.go:30-31)"""
    with open(os.path.join(REF, "clone", "example_test.go")) as f:
        src = f.read()
    at = src.index("fmt.Println(seqhash.RotateSequence(Clones[0]))")
    out = re.search(r"// Output: ([A-Za-z]+)", src[at:]).group(1)
    with open(os.path.join(HERE, "clone_goldengate_rotated.seq"), "w") as f:
        f.write(out + "\n")
    print("clone_goldengate_rotated.seq", len(out))


def clone_parts():
    """the clone.Part literals of the reference's own clone tests (clone/clone_test.go, clone/example_test.go):
    the inputs of TestSignalKilledGoldenGate (:167-194: 1 clone + 4 looping constructs), TestPanicGoldenGate
    (:196-214), TestCircularCutRegression (:216-228) and ExampleGoldenGate (example_test.go:11-31)"""
    import json

    def parts_of(path, start, end):
        with open(os.path.join(REF, "clone", path)) as f:
            lines = f.read().split("\n")[start - 1:end]
        return [[m.group(1), m.group(2) == "true"] for ln in lines for m in re.finditer(r'Part\{"([A-Za-z]+)", (true|false)\}', ln)]

    out = {
        "popen": parts_of("clone_test.go", 8, 8)[0],
        "signal_killed": parts_of("clone_test.go", 167, 179),
        "panic": parts_of("clone_test.go", 196, 206),
        "circular_cut_regression": parts_of("clone_test.go", 216, 222),
        "example_golden_gate": parts_of("example_test.go", 11, 24),
    }
    assert len(out["signal_killed"]) == 9 and len(out["panic"]) == 5 and len(out["example_golden_gate"]) == 3
    with open(os.path.join(HERE, "clone_parts.json"), "w") as f:
        json.dump(out, f, indent=0)
    print("clone_parts.json", {k: len(v) for k, v in out.items()})


def fork_declarations():
    """for every rename of go/fork.sh: the 1-based numbers of the lines of the reference file that start with the
    declaration prefix it renames (tests/test_go_binding_cpu.py checks fork.sh against these)"""
    import json
    fork = open(os.path.join(HERE, "..", "..", "go", "fork.sh")).read()
    out = {}
    for m in re.finditer(r"^ren\s+(\S+)\s+'([^']*)'\s+'([^']*)'", fork, flags=re.M):
        path, old = m.group(1), m.group(2).replace("\\*", "*")
        with open(os.path.join(REF, path)) as f:
            hits = [i + 1 for i, line in enumerate(f) if line.startswith(old)]
        assert hits, f"{path}: no line starts with `{old}`"
        out.setdefault(path, {})[old] = hits
    with open(os.path.join(HERE, "fork_declarations.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("fork_declarations.json", sum(len(v) for v in out.values()))


if __name__ == "__main__":
    copy_fastq()
    clone_example_output()
    clone_parts()
    fork_declarations()
    matrices()
    sys.exit(main())
