"""The rule of `poregen reform -c --to_ref` / pg_mvops_project in plain Python, written from the issue's table and not from the product's
code: a read's ss ops (one per base, in signal order) carried through its CIGAR onto the reference, and the PAF line of the result.
Nothing here calls the product."""
import re

OPS = "MIDNSHP=X"
NO_CIGAR, LENGTH, BAD_OP = 5, 6, 7
U32 = 0xffffffff


def _i32(x):
    x &= U32
    return x - (1 << 32) if x >> 31 else x


def words_of(cigar):
    """'2S3M1I' -> [2 << 4 | 4, 3 << 4 | 0, 1 << 4 | 1]; '*' -> []."""
    if cigar == "*":
        return []
    return [int(n) << 4 | OPS.index(c) for n, c in re.findall(r"(\d+)([MIDNSHP=X])", cigar)]


def text_of(words):
    return "".join(f"{w >> 4}{OPS[w & 15]}" for w in words) or "*"


class Projected:
    def __init__(self, status, query_start):
        self.status, self.query_start, self.query_end = status, query_start, query_start
        self.ops = []                                        # [(value, 0 match | 1 I | 2 D)]
        self.ref_len = self.n_match = self.target_start = self.target_end = 0


def project(o, query_start, status_in, words, pos, rna=False):
    """o: the read's ops in signal order (status_in: what the expansion said of it, 0 = accepted); words: the CIGAR as BAM stores it."""
    L = len(o)
    if status_in:
        return Projected(status_in, query_start)
    if not words:
        return Projected(NO_CIGAR, query_start)
    if sum(w >> 4 for w in words if (w & 15) < 9 and OPS[w & 15] in "MIS=X") != L:
        return Projected(LENGTH, query_start)
    if any((w & 15) > 8 for w in words):
        return Projected(BAD_OP, query_start)
    p = Projected(0, query_start)
    q, lead, written, in_front = 0, 0, 0, True
    for w in (reversed(words) if rna else words):
        n, c = w >> 4, OPS[w & 15]
        if n == 0:
            continue
        if c in "M=X":
            p.ops += [(v, 0) for v in o[q:q + n]]; written += sum(o[q:q + n]); p.n_match += n; p.ref_len += n; q += n
        elif c == "I":
            s = sum(o[q:q + n]) & U32
            p.ops.append((s, 1)); written += s; q += n
        elif c in "DN":
            p.ops.append((n, 2)); p.ref_len += n
        elif c == "S":
            if in_front:
                lead += sum(o[q:q + n])
            q += n
        if c in "M=XIDN":
            in_front = False
    p.ref_len &= U32
    p.query_start = _i32(query_start + lead)
    p.query_end = _i32(p.query_start + written)
    a, b = _i32(pos), _i32(pos + p.ref_len)
    p.target_start, p.target_end = (b, a) if rna else (a, b)
    return p


def ss_of(ops):
    return "".join(f"{v}{',ID'[t]}" for v, t in ops)


def paf_line(qname, ns, p, rname, ref_total):
    return (f"{qname}\t{ns}\t{p.query_start}\t{p.query_end}\t+\t{rname}\t{ref_total}\t{p.target_start}\t{p.target_end}\t{p.n_match}\t{p.ref_len}\t255\t"
            f"ss:Z:{ss_of(p.ops)}\n")
