"""`poregen kmer_freq` on a FASTA: the rules restated in plain Python (the test oracle) and the inputs the CPU and GPU tests share.

The rules (include/pgmove.h, pg_kfreq_submit_fasta): lines end at a newline byte and nowhere else, the last one may be unterminated. A line
whose first byte is '>' is a header line, every other line a sequence line. A record is a maximal run of sequence lines with no header
line between them; its sequence is their bytes joined. Every run of k consecutive bytes of a record's sequence is a key. Nothing is
dropped at the end of the stream. A NUL byte in a sequence line is refused.

K lists the k-mer sizes the tests use: both histogram paths (k <= 6 in LDS, above in global memory), their border and the largest key.
SPAN / TILE / UNIT are the kernel's sizes (pg_kfreq.hip): bytes per thread, per workgroup and per launch.
"""
from collections import Counter

import numpy as np

K = (1, 2, 5, 6, 7, 12)
SPAN, TILE, UNIT = 128, 32768, 16 << 20


class NulInSequence(ValueError):
    """A sequence line holds a zero byte: the product refuses such input."""


# ---- the oracle -------------------------------------------------------------------------------------------------------------------

def split_lines(data: bytes):
    """The lines without their newline; no line behind a final newline."""
    out = data.split(b"\n")
    if out and out[-1] == b"":
        out.pop()
    return out


def records(data: bytes):
    """The sequence of every record, in order (rules 1-3). An empty record in front of a leading header is left out."""
    recs, cur, seen = [], [], False
    for line in split_lines(data):
        if line[:1] == b">":
            if seen or cur:
                recs.append(b"".join(cur))
            cur, seen = [], True
        else:
            if b"\0" in line:
                raise NulInSequence()
            cur.append(line)
    if seen or cur:
        recs.append(b"".join(cur))
    return recs


def count_seqs(seqs, k: int) -> Counter:
    c = Counter()
    for s in seqs:
        if len(s) - k + 1 > 20000:   # the same windows, counted by numpy: a Counter over a megabyte of them takes seconds
            w = np.lib.stride_tricks.sliding_window_view(np.frombuffer(s, np.uint8), k)
            keys, n = np.unique(np.ascontiguousarray(w).view(np.dtype((np.void, k))).ravel(), return_counts=True)
            for key, m in zip(keys.tolist(), n.tolist()):
                c[bytes(key)] += m
        else:
            for j in range(len(s) - k + 1):
                c[s[j:j + k]] += 1
    return c


def count(data: bytes, k: int) -> Counter:
    return count_seqs(records(data), k)


def as_fastq(data: bytes) -> bytes:
    """Q(X): the FASTQ whose sequence lines are the records of the FASTA X."""
    return b"".join(b"@\n" + s + b"\n+\n\n" for s in records(data))


_DIGIT = {65: 0, 67: 1, 71: 2, 84: 3}


def split_counter(c: Counter, k: int):
    """({code: count} of the ACGT keys, sorted other keys, their counts)."""
    dense, odd = {}, {}
    for key, n in c.items():
        if all(b in _DIGIT for b in key):
            i = 0
            for b in key:
                i = i * 4 + _DIGIT[b]
            dense[i] = n
        else:
            odd[key] = n
    keys = sorted(odd)
    return dense, keys, [odd[x] for x in keys]


def assert_result(res, c: Counter, k: int):
    """A KmerFreqResult against a Counter: the dense counts and the odd keys and counts, exactly."""
    dense, keys, counts = split_counter(c, k)
    want = np.zeros(4 ** k, np.uint64)
    if dense:
        want[np.fromiter(dense.keys(), np.int64)] = np.fromiter(dense.values(), np.uint64)
    assert np.array_equal(res.counts, want)
    assert res.odd_keys == keys and [int(x) for x in res.odd_counts] == counts


# ---- inputs -----------------------------------------------------------------------------------------------------------------------

def rand_seq(rng, n: int, alphabet: bytes = b"ACGT") -> bytes:
    return np.frombuffer(alphabet, np.uint8)[rng.integers(0, len(alphabet), n, dtype=np.uint8)].tobytes()


def wrap(seq: bytes, width: int, nl: bytes = b"\n") -> bytes:
    return b"".join(seq[i:i + width] + nl for i in range(0, len(seq), width))


def line_widths(k: int):
    return sorted({w for w in (1, 2, k - 1, k, k + 1, 60, 61, 127, 128, 129) if w >= 1})


def mixed(rng, k: int, width: int, terminated: bool = True) -> bytes:
    """Records wrapped at `width`: sequence in front of the first header, records shorter than k, of exactly k, empty ones, an empty
    line inside a record, a one-byte header, '>' inside a sequence line, headers made of ACGT letters."""
    out = [wrap(rand_seq(rng, 2 * width + k), width)]                   # no header in front
    out += [b">ACGTACGTACGTACGT\n", wrap(rand_seq(rng, max(k - 1, 0)), width)]
    out += [b">\n", wrap(rand_seq(rng, k), width)]
    out += [b">empty\n", b">GATTACA again empty\n", b">\n"]
    out += [b">r3\n", wrap(rand_seq(rng, k + 1), width), b"\n\n", wrap(rand_seq(rng, 3 * width + 5), width)]   # empty lines inside
    out += [b">r4\n", wrap(rand_seq(rng, width + 3) + b">" + rand_seq(rng, k + 2) + b"AC>GT" + rand_seq(rng, 5), width)]
    out += [b">TTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTT\n", wrap(rand_seq(rng, 700), width)]
    data = b"".join(out)
    return data if terminated else data[:-1]


def edge_stream(rng, k: int, step: int, what: str, reach: int = 0) -> bytes:
    """A '\\n' (what = "nl") or the '>' of a short header line (what = "header") at every offset within k + 1 bytes of an edge that
    lies at a multiple of `step`, one offset per edge, inside one random record. reach > 0: the record is kept for `reach` bytes on
    either side of every edge only and the stretch between two edges is one long header line, whose bytes are never keys (a
    reference over a megabyte of distinct 12-byte keys takes far longer than the run under test)."""
    deltas = list(range(-(k + 1), k + 2))
    buf = bytearray(b">r\n" + rand_seq(rng, step * (len(deltas) + 1)))
    for i, d in enumerate(deltas):
        at = step * (i + 1) + d
        if what == "nl":
            buf[at] = 10
        else:
            buf[at - 1:at + 5] = b"\n>AC \n"
        if reach:
            lo = step * i + reach if i else 3
            buf[lo] = 10; buf[lo + 1] = ord(">"); buf[step * (i + 1) - reach] = 10
    return bytes(buf)


def long_header(rng, k: int, n_header: int) -> bytes:
    """A header line of n_header bytes made of ACGT letters between two records: nothing of it may be counted, and the record behind it
    starts anew."""
    text = rand_seq(rng, min(n_header - 1, 4099))
    header = (text * (n_header // len(text) + 1))[:n_header - 1]                # letters all the way, without a large random draw
    return b">a\n" + wrap(rand_seq(rng, 200), 60) + b">" + header + b"\n" + wrap(rand_seq(rng, 300), 60)


def short_lines(rng, k: int, one_byte: bool, n_lines: int = 10000) -> bytes:
    """n_lines empty lines (or one-byte lines) between the two halves of a record: the windows run across them."""
    mid = wrap(rand_seq(rng, n_lines), 1) if one_byte else b"\n" * n_lines
    return b">x\n" + rand_seq(rng, 90) + b"\n" + mid + rand_seq(rng, 90) + b"\n"


def homopolymer(n: int = 5000) -> bytes:
    return b">poly\n" + wrap(b"A" * n, 60)


SMALL = (b"ACGTAC\n>h1 x\nACGTNACGTACGTAGCTAGCTA\nGGATCCATGCAT\n\nTTGACA\n>h2\nAC\n>\n>ACGTACGTACGTACGT\nacgTTGCATGCATGCAAGT\r\n"
         b"TTAGGCATCGATCGGATTACAGATTACA")   # two and more headers, unterminated, below 300 bytes


def boundary_cuts(data: bytes, k: int):
    """Every offset within k + 1 bytes of the first byte of a header line or of the first byte behind one."""
    cuts = set()
    at = 0
    for line in data.split(b"\n"):
        if line[:1] == b">":
            for b in (at, at + len(line) + 1):
                cuts.update(range(max(0, b - k - 1), min(len(data), b + k + 1) + 1))
        at += len(line) + 1
    return sorted(cuts)


def records_file(rng, n_records: int = 4, mean: int = 500, width: int = 60) -> bytes:
    return b"".join(b">rec%d some text\n" % i + wrap(rand_seq(rng, int(rng.integers(mean // 2, 2 * mean))), width) for i in range(n_records))


def random_x(rng, max_bytes: int = 4096) -> bytes:
    """A random FASTA-like byte string: headers, sequence lines over a dirty alphabet, empty lines, sometimes unterminated."""
    out, n = [], 0
    limit = int(rng.integers(1, max_bytes))
    while n < limit:
        r = rng.random()
        if r < 0.2:
            line = b">" + rand_seq(rng, int(rng.integers(0, 40)), b"ACGT >xyz0123")
        elif r < 0.3:
            line = b""
        else:
            line = rand_seq(rng, int(rng.integers(1, 150)), b"ACGT" * 12 + b"Nacgt>\r")
        out.append(line + b"\n")
        n += len(line) + 1
    data = b"".join(out)[:limit]
    return data
