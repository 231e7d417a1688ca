"""Shared by the tests of `poregen kmer_freq` on SAM/BAM input: packed reads as a BAM record stores them, the read `samtools fastq`
prints from one (by its documented rules, restated here), a plain Counter over printed reads, and writers for small BAM / SAM / FASTQ
files. Nothing here calls the product."""
import gzip
import struct
import zlib
from collections import Counter

import numpy as np

LETTERS = b"=ACMGRSVTWYHKDBN"                       # SAM specification 4.2.3: the letter of each 4-bit code
#            =  A  C  M   G  R   S  V   T  W  Y  H   K  D   B  N
COMPLEMENT = [0, 8, 4, 12, 2, 10, 6, 14, 1, 9, 5, 13, 3, 11, 7, 15]   # A<->T C<->G M<->K R<->Y V<->B H<->D; = S W N stay
A, C_, G, T, N = 1, 2, 4, 8, 15


def code_of_byte(b: int) -> int:
    """htslib's packing of a byte of a SAM SEQ column, as the issue states it: the letters in either case, anything else N."""
    i = LETTERS.find(bytes([b]).upper())
    return i if i >= 0 else 15


def codes_of(text: bytes) -> np.ndarray:
    return np.array([code_of_byte(b) for b in text], np.uint8)


def pack(codes, pad=0xF) -> bytes:
    """Two codes per byte, high nibble first; an odd read's last low nibble is `pad` (never a base)."""
    c = [int(x) for x in codes]
    if len(c) & 1:
        c.append(pad)
    return bytes(c[i] << 4 | c[i + 1] for i in range(0, len(c), 2))


def printed(codes, reverse=False, n_to_t=False) -> bytes:
    """The sequence line `samtools fastq` prints: with flag 0x10 reversed and complemented; then sed's N -> T."""
    c = [int(x) for x in codes]
    if reverse:
        c = [COMPLEMENT[x] for x in reversed(c)]
    s = bytes(LETTERS[x] for x in c)
    return s.replace(b"N", b"T") if n_to_t else s


def count_printed(lines, k) -> Counter:
    c = Counter()
    for s in lines:
        for j in range(len(s) - k + 1):
            c[s[j:j + k]] += 1
    return c


def split_counter(c: Counter, k):
    """(dense uint64[4^k], sorted odd keys, their counts) of a Counter of k-byte keys."""
    dense = np.zeros(4 ** k, np.uint64)
    odd = {}
    digit = {65: 0, 67: 1, 71: 2, 84: 3}
    for key, n in c.items():
        if all(b in digit for b in key):
            i = 0
            for b in key:
                i = i * 4 + digit[b]
            dense[i] = n
        else:
            odd[key] = n
    keys = sorted(odd)
    return dense, keys, [odd[x] for x in keys]


def layout(reads, gaps=(0,), pad=0xF, lead=0):
    """seq_bytes / byte_off / l_seq / reverse of [(codes, reverse)], with gaps[i % len] bytes of 0xFF in front of read i."""
    buf = bytearray(b"\xff" * lead)
    off, ln, rv = [], [], []
    for i, (codes, rev) in enumerate(reads):
        buf += b"\xff" * gaps[i % len(gaps)]
        off.append(len(buf)); ln.append(len(codes)); rv.append(1 if rev else 0)
        buf += pack(codes, pad)
    return (np.frombuffer(bytes(buf), np.uint8), np.array(off, np.uint64), np.array(ln, np.uint32), np.array(rv, np.uint8))


def fastq(lines) -> bytes:
    return b"".join(b"@r%d\n%s\n+\n%s\n" % (i, s, b"I" * len(s)) for i, s in enumerate(lines))


# ---- files ----------------------------------------------------------------------------------------------------------------------

def bam_record(name: bytes, flag: int, codes) -> bytes:
    n = len(codes)
    body = struct.pack("<iiBBHHHiiii", -1, -1, len(name) + 1, 0, 4680, 0, flag, n, -1, -1, 0) + name + b"\0" + pack(codes, 0xF) + b"\xff" * n
    return struct.pack("<i", len(body)) + body


def bgzf_block(data: bytes) -> bytes:
    co = zlib.compressobj(6, zlib.DEFLATED, -15)
    comp = co.compress(data) + co.flush()
    bsize = 12 + 6 + len(comp) + 8
    return (b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0" + struct.pack("<H", bsize - 1) + comp +
            struct.pack("<II", zlib.crc32(data) & 0xffffffff, len(data)))


def bam_file(records, cut=None, magic=b"BAM\1") -> bytes:
    """records: [(name, flag, codes)]. Two data blocks cut at byte `cut` of the stream (default: inside the second record), then the
    empty end-of-file block."""
    text = b"@HD\tVN:1.6\tSO:unknown\n"
    stream = magic + struct.pack("<i", len(text)) + text + struct.pack("<i", 0)
    recs = [bam_record(*r) for r in records]
    if cut is None:
        cut = len(stream) + len(recs[0]) + len(recs[1]) // 2
    stream += b"".join(recs)
    return bgzf_block(stream[:cut]) + bgzf_block(stream[cut:]) + bgzf_block(b"")


def sam_file(records, header: bool) -> bytes:
    """records: [(name, flag, SEQ text)]"""
    out = b"@HD\tVN:1.6\tSO:unknown\n@PG\tID:basecaller\n" if header else b""
    for name, flag, seq in records:
        out += b"\t".join([name, b"%d" % flag, b"*", b"0", b"0", b"*", b"*", b"0", b"0", seq, b"*", b"mv:B:c,5,1,0,1"]) + b"\n"
    return out


def bam_reads(path):
    """[(flag, codes)] of every record of a BAM file, parsed here with gzip and struct."""
    d = gzip.decompress(open(path, "rb").read())
    assert d[:4] == b"BAM\1"
    l_text, = struct.unpack_from("<i", d, 4)
    p = 8 + l_text
    n_ref, = struct.unpack_from("<i", d, p)
    p += 4
    for _ in range(n_ref):
        l_name, = struct.unpack_from("<i", d, p)
        p += 8 + l_name
    out = []
    while p < len(d):
        block_size, = struct.unpack_from("<i", d, p)
        l_read_name, = struct.unpack_from("<B", d, p + 12)
        n_cigar, flag, l_seq = struct.unpack_from("<HHi", d, p + 16)
        s = p + 36 + l_read_name + 4 * n_cigar
        b = np.frombuffer(d, np.uint8, (l_seq + 1) // 2, s)
        codes = np.stack([b >> 4, b & 15], 1).reshape(-1)[:l_seq]
        out.append((flag, codes))
        p += 4 + block_size
    return out
