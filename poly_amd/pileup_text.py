"""Parser and writer of the six-column pileup text format: the Python mirror of the reference's ``io/pileup`` package.

A row is ``sequence \\t position \\t reference base \\t read count \\t read results \\t quality \\n``.  ``pileup.rows`` /
``rows_packed`` / ``rows_refs`` (polyhip_pileup_rows) write this text on the GPU from the mapper's output; this module reads it
back and writes it again, on the CPU, with the reference's observable behaviour kept, quirks included:

* ``^`` takes three bytes (itself, the mapping quality and the base) as one read result;
* ``$`` is appended to the read result before it;
* a ``+n...`` or ``-n...`` run is a read result of its own, so ``len(read_results)`` is the read count plus the runs printed;
  the reference slices ``n + 2`` bytes for it from the sign on, which is the whole run only while n has one digit: a run of
  10 or more loses its last letters in ``read_results`` (it is skipped in full all the same), so such a row does not
  round-trip;
* the read results hold ``^ $ . , * A T G C N a t g c n - +`` and, inside a run, digits and the ten letters;
* a last line without a newline is dropped without error;
* a line longer than ``max_line_size`` bytes, newline included, is an error (``polyhip_pileup_rows_last_info``'s
  ``max_row_bytes`` says beforehand whether a row will fit).
"""
from __future__ import annotations

import io
from dataclasses import dataclass, field

MAX_LINE_SIZE = 2 * 32 * 1024          # the reference's Parse: twice the 32 kB the Go standard library likes
_SINGLE = set(".,*ATGCNatgcn")
_IN_RUN = set("0123456789ATGCNatgcn-+")


class PileupError(ValueError):
    """a row the parser refuses; ``rows`` holds the rows parsed before it (the reference returns them beside the error)"""

    def __init__(self, message: str, rows=None):
        super().__init__(message)
        self.rows = [] if rows is None else rows


@dataclass
class Pileup:
    """one position of a pileup file"""
    sequence: str = ""
    position: int = 0
    reference_base: str = ""
    read_count: int = 0
    read_results: list = field(default_factory=list)
    quality: str = ""


def _atoi(s: str) -> int:
    """strconv.Atoi: an optional sign and decimal digits that fit an int64"""
    digits = s[1:] if s[:1] in ("+", "-") else s
    if not digits or not all("0" <= c <= "9" for c in digits) or not -(1 << 63) <= int(s) < 1 << 63:
        why = "invalid syntax" if not digits or not all("0" <= c <= "9" for c in digits) else "value out of range"
        raise ValueError(f'strconv.Atoi: parsing "{s}": {why}')
    return int(s)


class Parser:
    """a pileup parser over bytes, a str or a binary / text file object"""

    def __init__(self, source, max_line_size: int = MAX_LINE_SIZE):
        if hasattr(source, "read"):
            source = source.read()
        if isinstance(source, str):
            source = source.encode("latin-1")
        self._data = bytes(source)
        self._at = 0
        self._max = max(int(max_line_size), 16)      # bufio.NewReaderSize never goes below 16
        self.line = 0

    def parse_next(self) -> Pileup | None:
        """the next row, or None at the end of the data (a last line without a newline is the end too)"""
        if self._at >= len(self._data):
            return None
        end = self._data.find(b"\n", self._at, self._at + self._max)
        if end < 0:
            if len(self._data) - self._at >= self._max:
                raise PileupError("bufio: buffer full")
            self._at = len(self._data)
            return None
        line = self._data[self._at:end].decode("latin-1")
        self._at = end + 1
        self.line += 1
        values = line.split("\t")
        if len(values) != 6:
            raise PileupError(f"Error on line {self.line}: Got {len(values)} values, expected 6.")
        try:
            position = _atoi(values[1])
            read_count = _atoi(values[3])
        except ValueError as e:
            raise PileupError(f"Error on line {self.line}. Got error: {e}") from None
        results, s, skip = [], values[4], 0
        for k, c in enumerate(s):
            if skip:
                skip -= 1
                continue
            if c == "^":
                skip += 2
                results.append(s[k:k + 3])
            elif c == "$":
                if not results:
                    raise PileupError(f"Error on line {self.line}: '$' without a read result before it")
                results[-1] += "$"
            elif c in _SINGLE:
                results.append(c)
            elif c in "+-":
                number = ""
                for d in range(len(s) - k):
                    if k + d + 1 >= len(s):
                        raise PileupError(f"Error on line {self.line}: the read results end inside a {c} run")
                    if s[k + d + 1].isdigit():
                        number += s[k + d + 1]
                        continue
                    break
                count = int(number) if number else 0
                if k + count + 2 > len(s):
                    raise PileupError(f"Error on line {self.line}: the read results end inside a {c} run")
                run = s[k:k + count + 2]
                for x in run:
                    if x not in _IN_RUN:
                        raise PileupError(f"Rune within +,- not found on line {self.line}. Got {x}: only runes allowed are: "
                                          "[0 1 2 3 4 5 6 7 8 9 A T G C N a t g c n - +]")
                results.append(run)
                skip += count + len(number)
            else:
                raise PileupError(f"Rune not found on line {self.line}. Got {c}: only runes allowed are: "
                                  "[^ $ . , * A T G C N a t g c n - +]")
        return Pileup(values[0], position, values[2], read_count, results, values[5])

    def parse_n(self, max_rows: int) -> list:
        """up to ``max_rows`` rows; the end of the data is no error"""
        rows = []
        while len(rows) < max_rows:
            try:
                row = self.parse_next()
            except PileupError as e:
                e.rows = rows
                raise
            if row is None:
                break
            rows.append(row)
        return rows

    def parse_all(self) -> list:
        return self.parse_n(1 << 62)


def parse(source, max_line_size: int = MAX_LINE_SIZE) -> list:
    """every row of a pileup text (bytes, str or a file object)"""
    return Parser(source, max_line_size).parse_all()


def parse_n(source, max_rows: int, max_line_size: int = MAX_LINE_SIZE) -> list:
    return Parser(source, max_line_size).parse_n(max_rows)


def write_pileups(pileups, w=None) -> bytes:
    """the rows as text; also written to the binary file object ``w`` when one is given"""
    out = io.BytesIO()
    for p in pileups:
        out.write(("\t".join([p.sequence, str(int(p.position)), p.reference_base, str(int(p.read_count)), "".join(p.read_results),
                              p.quality]) + "\n").encode("latin-1"))
    data = out.getvalue()
    if w is not None:
        w.write(data)
    return data


def read(path) -> list:
    with open(path, "rb") as fh:
        return parse(fh)


def write(pileups, path) -> None:
    data = write_pileups(pileups)
    with open(path, "wb") as fh:
        fh.write(data)
