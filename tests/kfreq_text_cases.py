"""`poregen kmer_freq` on a FASTQ: the inputs the CPU and GPU edge tests share. The oracle is tests/kfreq_ref.py; nothing here calls the
product, except that levels() asks the host build for the kernels' sizes.

K lists the k-mer sizes the tests use: both histogram paths (k <= 6 in LDS, above in global memory) and their border, the first k whose
odd key needs its high word (9), and the largest. SPAN / TILE / UNIT are the kernels' sizes (pg_kfreq_text.h): bytes per thread, per
workgroup and per launch.
"""
import ctypes as C
import functools

import numpy as np

import dumptext_cases
from kfreq_fasta_cases import SPAN, TILE, UNIT, rand_seq

K = (1, 2, 5, 6, 7, 9, 12)
KINDS = ("seq_end", "seq_start", "n", "short")


@functools.lru_cache(maxsize=None)
def levels():
    """(span, tile, unit, max k, LDS max k, odd windows staged per workgroup) of the kernels"""
    out = (C.c_uint64 * 6)()
    dumptext_cases.hosttest().pgt_kfreq_levels(out)
    return tuple(int(x) for x in out)


def line_index(data: bytes, at: int) -> int:
    """Index of the line that holds byte `at` (a newline belongs to the line it ends)."""
    return data.count(b"\n", 0, at)


def edge_stream(rng, k: int, step: int, what: str, reach: int = 0) -> bytes:
    """One FASTQ of whole records with an edge at every multiple of `step`, one per delta in -(k + 1) .. k + 1, and at edge + delta
    "seq_end":   the newline that ends a sequence line,
    "seq_start": the first byte of a sequence line (the header's newline is at edge + delta - 1),
    "n":         an N inside a sequence line that runs at least k bytes on both sides,
    "short":     the middle of a sequence line of k - 1, k or k + 1 bytes (three edges per delta, one per length).
    The sequence lines run `reach` bytes from the placed byte (reach = 0: as far as the step allows); the stretch between two of them is
    the quality line of the one and the header line of the next, both made of ACGT letters: a walk that takes them for sequence counts
    them. The placement is asserted here."""
    assert what in KINDS
    r = reach or step // 2 - k - 6
    assert k <= r <= step // 2 - k - 6
    lines = []                                                   # (start, bytes without the newline, offset of the placed byte)
    deltas = [d for d in range(-(k + 1), k + 2) for _ in range(3 if what == "short" else 1)]
    for i, d in enumerate(deltas):
        at = step * (i + 1) + d
        if what == "seq_end":
            lines.append((at - r, rand_seq(rng, r), at))
        elif what == "seq_start":
            lines.append((at, rand_seq(rng, r), at))
        elif what == "n":
            lines.append((at - r, rand_seq(rng, r) + b"N" + rand_seq(rng, r), at))
        else:
            n = k - 1 + i % 3
            lines.append((at - n // 2, rand_seq(rng, n), at))
    out, pos = bytearray(), 0
    for i, (start, seq, at) in enumerate(lines):
        gap = start - pos - (5 if i else 2)                      # "+\n" qual "\n" "@" header "\n" (the first record: "@" header "\n")
        assert gap >= 0
        q = int(rng.integers(0, gap + 1)) if i else 0
        if i:
            out += b"+\n" + rand_seq(rng, q) + b"\n"
        out += b"@" + rand_seq(rng, gap - q) + b"\n"
        assert len(out) == start
        out += seq + b"\n"
        pos = len(out)
    out += b"+\n" + rand_seq(rng, 7) + b"\n"
    data = bytes(out)
    assert data.count(b"\n") % 4 == 0
    for start, seq, at in lines:                                 # the placement: the byte, and that its line is a sequence line
        assert line_index(data, at) % 4 == 1 and data[start:start + len(seq)] == seq and data[start + len(seq)] == 10
        if what == "seq_end":
            assert data[at] == 10 and data[at - 1] != 10
        elif what == "seq_start":
            assert data[at - 1] == 10 and data[at] != 10
        elif what == "n":
            assert data[at] == ord("N") and b"\n" not in data[at - k:at + k + 1]
        else:
            assert start <= at <= start + len(seq) and len(seq) in (k - 1, k, k + 1)
    return data


def tiles_stream(rng, n_bytes: int) -> bytes:
    """n_bytes of records whose header and quality lines hold 1 .. 20 000 ACGT letters and whose sequence lines 0 .. 200 bytes over ACGTN:
    neighbouring tiles hold different numbers of newlines. The last record is cut where the stream ends. (Built line by line: no array
    of the stream's size is made.)"""
    out, n = [], 0
    while n < n_bytes:
        h, s, q = (int(x) for x in rng.integers((1, 0, 1), (20001, 201, 20001)))
        out += [b"@", rand_seq(rng, h), b"\n", rand_seq(rng, s, b"ACGTN"), b"\n+\n", rand_seq(rng, q), b"\n"]
        n += h + s + q + 6
    return b"".join(out)[:n_bytes]


# at least four records, below 300 bytes: N, an empty sequence line, lines of k - 1 bytes (4: k = 5, 11: k = 12), lower case, a CRLF
# record, quality lines made of letters
SMALL = (b"@r1\nACGTNACGTACGTAGCTAGCTAGGATCC\n+\nIIIIIIIIIIIIIIIIIIIIIIIIIIII\n"
         b"@r2\n\n+\n\n"
         b"@r3 x\nACGT\n+\nACGT\n"
         b"@r4\r\nacgTTGCATGCATGCAAGT\r\n+\r\nIIIIIIIIIIIIIIIIIII\r\n"
         b"@r5\nTTAGGCATCGATCGGATTACAGATTACA\n+\nTTAGGCATCGATCGGATTACAGATTACA\n"
         b"@r6\nACGTACGTACG\n+\nIIIIIIIIIII\n")
SMALL_SEQ_OPEN = SMALL + b"@r7\nGATTACAGGCNTTGACAGATTAC"             # ends inside a sequence line: its last byte is dropped
SMALL_QUAL_OPEN = SMALL + b"@r7\nGATTACAGGCNTTGACAGATTAC\n+\nIIII"   # ends inside a quality line
SMALLS = (SMALL, SMALL_SEQ_OPEN, SMALL_QUAL_OPEN)


def boundary_cuts(data: bytes, k: int):
    """Every offset within k + 1 bytes of the first and of the last byte of a sequence line."""
    cuts, at = set(), 0
    for i, line in enumerate(data.split(b"\n")):
        if i % 4 == 1:
            for b in (at, at + max(len(line) - 1, 0)):
                cuts.update(range(max(0, b - k - 1), min(len(data), b + k + 1) + 1))
        at += len(line) + 1
    return sorted(cuts)


def records_file(rng, n_records: int = 3, mean: int = 500) -> bytes:
    out = []
    for i in range(n_records):
        s = rand_seq(rng, int(rng.integers(mean // 2, 2 * mean)), b"ACGT" * 8 + b"N")
        out.append(b"@rec%d some text\n" % i + s + b"\n+\n" + rand_seq(rng, len(s)) + b"\n")
    return b"".join(out)


def dirty(rng, n: int) -> bytes:
    """n bytes of sequence over ACGTNacgtRY\\r in lines of about 700: nearly every window is an odd one and nearly all are distinct, so
    one tile stages more than the 512 odd windows its LDS holds."""
    out, left, i = [], n, 0
    while left > 0:
        m = min(left, int(rng.integers(500, 900)))
        out.append(b"@d%d\n" % i + rand_seq(rng, m, b"ACGTNacgtRY\r") + b"\n+\n" + rand_seq(rng, m) + b"\n")
        left -= m; i += 1
    return b"".join(out)


def one_line(seq: bytes, header: bytes = b"@h") -> bytes:
    """One record whose sequence line is seq, its quality line made of the letters of seq."""
    return header + b"\n" + seq + b"\n+\n" + seq + b"\n"
