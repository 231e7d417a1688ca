"""Reverse-strand records by the one rule "a reverse-strand record is a forward record on the reverse complement of its contig", reduced to
the merged forward rule of tests/refops_ref.py and restating nothing of it; and the reference slice of a read -- the clamp of
`gmove --reform --ref` (htslib's faidx_adjust_position behind the PAF front-end's unsigned min / max) and the complement -- in plain
Python. Nothing here calls the product."""
import refops_ref as R

NO_CONTIG_LEN = 8
U32 = 0xffffffff
_COMP = bytes.maketrans(b"ACGTUacgtu", b"TGCAAtgcaa")


def _ref_len(words):
    return sum(w >> 4 for w in words if (w & 15) in (0, 2, 3, 7, 8)) & U32


def project(o, query_start, status_in, words, pos, rna=False, reverse=False, contig_len=0):
    """A forward read: R.project. A reverse read: R.project of the words in reverse order at the mirrored position; status 8 (no contig
    length) stands behind every status R.project returns."""
    if not reverse:
        return R.project(o, query_start, status_in, words, pos, rna)
    p = R.project(o, query_start, status_in, list(reversed(words)), (contig_len - pos - _ref_len(words)) & U32, rna)
    if p.status == 0 and contig_len <= 0:
        return R.Projected(NO_CONTIG_LEN, query_start)
    return p


def _i32(x):
    x &= U32
    return x - (1 << 32) if x >> 31 else x


def clamp(pos, ref_len, contig_len):
    """(beg, n): the bases [beg, beg + n) of a contig of contig_len bases (None: no such contig) that the slice of a read at pos with
    ref_len holds. st_k / end_k are the smaller / larger of the two target columns compared as unsigned numbers; the fetch is
    faidx_fetch_seq(st_k, end_k - 1), both cut to an int."""
    if contig_len is None:
        return 0, 0
    a, b = _i32(pos), _i32(pos + ref_len)
    st_k, end_k = (b, a) if (a & 0xffffffffffffffff) > (b & 0xffffffffffffffff) else (a, b)
    beg, end = _i32(st_k), _i32(end_k - 1)
    if end < beg:
        beg = end
    beg = 0 if beg < 0 else min(beg, contig_len)
    end = 0 if end < 0 else (contig_len - 1 if contig_len <= end else end)
    n = min(end + 1 - beg, contig_len - beg)                # (a contig of no bases has none to give, whatever the adjustment says)
    return (beg, n) if n > 0 else (0, 0)


def complement(b):
    return bytes(b).translate(_COMP)


def revcomp(b):
    return complement(b)[::-1]


def ref_slice(contig, pos, ref_len, reverse=False):
    """contig: bytes, or None for a name the FASTA lacks."""
    if contig is None:
        return b""
    beg, n = clamp(pos, ref_len, len(contig))
    s = bytes(contig[beg:beg + n])
    return revcomp(s) if reverse else s


def mirror(contigs, suffix="_rc"):
    """[(name, bases)] -> the same list followed by every contig's reverse complement under name + suffix."""
    out = list(contigs)
    for name, s in contigs:
        out.append((name + suffix, revcomp(s.encode()).decode() if isinstance(s, str) else revcomp(s)))
    return out
