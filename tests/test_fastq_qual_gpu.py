"""polyhip_fastq_pack_qual: the device feeder that also packs the Quality field, against the CPU restatement of io/fastq
(oracle/fastq_ref.parse_all, which returns the quality) and against polyhip_fastq_pack on the same image: the same records,
sequences, offsets, error code and line, plus every record's quality bytes, their offsets and the two new result words."""
import glob
import os

import numpy as np
import pytest

from oracle import fastq_ref as fr

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden", "fastq")


def _raw(data: bytes, max_records=None):
    """polyhip_fastq_pack_qual on buffers pre-filled with 0xAB -> (result words, seqs, offsets, quals, qual_offsets, rec_start)"""
    from poly_amd import _lib
    buf = np.frombuffer(data, np.uint8)
    nb = len(buf)
    most = nb // 7 + 1
    cap = most if max_records is None else max_records
    seqs, quals = np.full(nb + 8, 0xAB, np.uint8), np.full(nb + 8, 0xAB, np.uint8)
    offs, qoffs, rec = (np.full(most + 2, 0xABABABABABABABAB, np.uint64) for _ in range(3))
    res = np.full(6, 0xAB, np.uint64)
    _lib.check(_lib.lib().polyhip_fastq_pack_qual(buf.ctypes.data if nb else None, nb, seqs.ctypes.data, offs.ctypes.data, quals.ctypes.data,
                                                  qoffs.ctypes.data, rec.ctypes.data, cap, res.ctypes.data))
    return [int(x) for x in res], seqs, offs, quals, qoffs, rec


def _check(data: bytes):
    """-> the records' qualities; everything compared with the restated parser and with polyhip_fastq_pack"""
    from poly_amd import fastq
    want, code, line = fr.parse_all(data)
    seqs, offs, quals, qoffs, rec, err = fastq.pack_qual(data)
    n = len(want)
    assert len(offs) == len(qoffs) == n + 1 and len(rec) == n
    got_q = [quals[int(qoffs[i]): int(qoffs[i + 1])].tobytes() for i in range(n)]
    got_s = [seqs[int(offs[i]): int(offs[i + 1])].tobytes() for i in range(n)]
    assert got_s == [w[1] for w in want]
    assert got_q == [w[2] for w in want]
    assert (err is None) == (code == 0) and (code == 0 or str(err) == fastq.ERRORS[code].format(line=line)), (code, line, err)
    res, rseqs, roffs, rquals, rqoffs, rrec = _raw(data)
    assert res == [n, code, line, sum(len(w[1]) for w in want), sum(len(w[2]) for w in want), sum(len(w[1]) != len(w[2]) for w in want)]
    assert fastq.pack_qual(data, with_mismatch=True)[6] == res[5]
    assert (rquals[res[4]:] == 0xAB).all() and (rqoffs[n + 1:] == 0xABABABABABABABAB).all()      # nothing beyond the kept records
    s0, o0, r0, e0 = fastq.pack(data)                                                             # polyhip_fastq_pack on the same image
    assert (s0 == seqs).all() and (o0 == offs).all() and (r0 == rec).all() and str(e0) == str(err)
    return got_q


def test_reference_fixtures():
    from poly_amd import fastq
    files = sorted(glob.glob(os.path.join(GOLD, "*.fastq")))
    assert len(files) == 7
    for f in files:
        data = open(f, "rb").read()
        _check(data)
        want, code, _ = fr.parse_all(data)
        assert (code == 0) == (os.path.basename(f) == "nanosavseq.fastq")
        if code:
            with pytest.raises(fastq.FastqError):
                fastq.qualities(data)
    data = open(os.path.join(GOLD, "nanosavseq.fastq"), "rb").read()
    q = fastq.qualities(data)
    assert len(q) == 4 and q == [w[2] for w in fr.parse_all(data)[0]] and all(len(x) > 100 for x in q)


def test_hand_written_images():
    from poly_amd import fastq
    # a quality shorter and one longer than its sequence: counted, and the offsets part ways
    data = b"@a\nACGT\n+\nII\n@b\nAC\n+\nIIIII\n@c\nACG\n+\nIII\n"
    assert _check(data) == [b"II", b"IIIII", b"III"]
    res, _, offs, _, qoffs, _ = _raw(data)
    assert res[4:] == [10, 2] and offs[:4].tolist() == [0, 4, 6, 9] and qoffs[:4].tolist() == [0, 2, 7, 10]
    # a quality that starts with '@', and one that is "+"
    assert _check(b"@a\nACGT\n+\n@III\n@b\nA\n+\n+\n@c\nAC\n+\n@@\n") == [b"@III", b"+", b"@@"]
    assert _check(b"@r\r\nACGT\r\n+\r\nIIII\r\n") == [b"IIII\r"]                  # the '\r' stays
    assert _check(b"@r\nACGT\n+\n!\n") == [b"!"]                                    # one byte
    assert _check(b"@\nA\n\nI\n") == [b"I"]                                         # the 7-byte record
    assert _check(b"@\nA\n\nI\n" * 3) == [b"I"] * 3
    assert _check(b"") == []
    assert _raw(b"")[0] == [0, 0, 0, 0, 0, 0]
    assert _check(b"@a\nAC\n+\nII\n@b\nACG\n+\nIII") == [b"II"]                    # a last line without '\n': code 4
    assert _check(b"@a\nAC\n+\nII") == []
    # an error in record 2: the qualities of records 0 and 1 are kept, [4] and [5] are over those only
    bad = b"@a\nACGT\n+\nIII\n@b\nAC\n+\nJJ\n@c\nACG\n+\n\n@d\nACGTA\n+\nI\n"
    assert _check(bad) == [b"III", b"JJ"]
    assert _raw(bad)[0] == [2, 3, 12, 6, 5, 1]
    assert _check(b"@a\nACGT\n+\nIII\n" + b"b\nAC\n+\nJJJ\n" + b"@c\nAC\n+\nK\n") == [b"III"]      # no '@' in record 1
    assert _check(b"@a x\nACGT\n+\nIII\n") == [] and fastq.pack_qual(b"@a x\nACGT\n+\nIII\n", with_mismatch=True)[6] == 0               # the panic, record 0


def test_max_records_cuts_the_file():
    from poly_amd import fastq
    data = b"".join(b"@r%d\n%s\n+\n%s\n" % (i, b"A" * (i % 5 + 1), b"I" * (i % 3 + 1)) for i in range(40))
    want = fr.parse_all(data)[0]
    for cap in (1, 7, 39):
        res, seqs, offs, quals, qoffs, rec = _raw(data, max_records=cap)
        qtotal = sum(len(w[2]) for w in want[:cap])
        assert res == [cap, 7, 0, sum(len(w[1]) for w in want[:cap]), qtotal, sum(len(w[1]) != len(w[2]) for w in want[:cap])]
        assert qoffs[:cap + 1].tolist() == np.cumsum([0] + [len(w[2]) for w in want[:cap]]).tolist()
        assert (qoffs[cap + 1:] == 0xABABABABABABABAB).all() and (offs[cap + 1:] == 0xABABABABABABABAB).all()
        assert (rec[cap:] == 0xABABABABABABABAB).all()
        assert quals[:qtotal].tobytes() == b"".join(w[2] for w in want[:cap]) and (quals[qtotal:] == 0xAB).all()
    out = fastq.pack_qual(data, max_records=7)
    assert len(out[3]) == 8 and "more records" in str(out[5])
    assert _raw(data, max_records=40)[0][:2] == [40, 0]


def _random_image(rng, count, longest):
    """records whose sequence and quality lengths are drawn apart, 1..longest: quality starts and lengths fall on every
    residue of 16 bytes and cross the 64-lane steps of the copy"""
    recs = []
    for i in range(count):
        ls, lq = int(rng.integers(1, longest + 1)), int(rng.integers(1, longest + 1))
        if i % 4:
            lq = ls                                                      # most records are well-formed
        seq = bytes(rng.choice(list(b"ACGTN"), ls).astype(np.uint8))
        qual = bytes(rng.integers(33, 127, lq, dtype=np.uint8))         # any printable byte: '@' and '+' come first now and then
        recs.append(b"@read%d ch=%d\n" % (i, i % 7) + seq + b"\n+\n" + qual + b"\n")
    return b"".join(recs)


def test_random_image():
    rng = np.random.default_rng(77)
    data = _random_image(rng, 1000, 300)
    want = fr.parse_all(data)[0]
    assert len(want) == 1000
    got = _check(data)
    starts = np.cumsum([0] + [len(q) for q in got[:-1]])
    assert len({int(s) % 16 for s in starts}) == 16 and len({len(q) % 16 for q in got}) == 16
    assert any(len(q) > 256 for q in got) and any(len(q) < 4 for q in got) and any(64 < len(q) < 128 for q in got)
    assert _raw(data)[0][5] > 100


def test_larger_image_takes_the_segmented_scan_twice():
    rng = np.random.default_rng(78)
    data = _random_image(rng, 5500, 50)
    assert len(data) // 7 + 1 > 32768                    # the bound the host picks the scan by
    _check(data)
    cut = data.index(b"@read3000 ")
    _check(data[:cut] + b"@r\nACGT\n+\n\n" + data[cut:])     # an empty quality deep inside: the qualities before it stay

