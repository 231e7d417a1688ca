"""Shared by the tests of reverse-strand records (pg_refops.h with a strand, pg_mvops_project_stranded, `reform --to_ref --both_strands`,
`gmove --reform --ref --both_strands`): the cases of tests/refops_cases.py, each read in both directions, and mapped SAM / BAM files in
two forms -- A: half the records on the reverse strand of REF.fa; B: the same reads as forward records on BOTH.fa, which holds every
contig and its reverse complement. B needs nothing a reverse-strand path adds. Nothing here calls the product."""
import copy

import numpy as np

import refops_cases as X
import refops_ref as R
import strand_ref as S


class SCase:
    """A refops_cases.Case with a strand and the length of its contig; X.layout and X.expected take it as they take a Case."""

    def __init__(self, case, reverse, contig_len, label=None):
        self.label = label or f"{case.label}{'-' if reverse else '+'}"
        self.o, self.words, self.qs, self.status, self.pos = case.o, case.words, case.qs, case.status, case.pos
        self.reverse, self.contig_len = bool(reverse), int(contig_len)

    def ref(self, rna=False):
        return S.project(self.o, self.qs, self.status, self.words, self.pos, rna, self.reverse, self.contig_len)


def _ref_len(words):
    return sum(w >> 4 for w in words if (w & 15) in (0, 2, 3, 7, 8)) & 0xffffffff


def _some_len(c):
    """A positive int32 that lies behind the read where the numbers allow it."""
    return 1 + ((c.pos + _ref_len(c.words) + 36) & 0x7ffffffe)


def both_ways(cases):
    """Every case forward, then reversed: the strands alternate along the batch."""
    out = []
    for c in cases:
        out += [SCase(c, False, _some_len(c)), SCase(c, True, _some_len(c))]
    return out


def edge_cases():
    return both_ways(X.edge_cases())


def random_batch(n, seed=3):
    """n reads: those of refops_cases.random_batch(n / 2), each in both directions."""
    return both_ways(X.random_batch((n + 1) // 2, seed))[:n]


def rule_cases(seed=5):
    """What the strand adds to the rule: status 8 and where it stands among the others, and the mirrored position at and past the end of
    the contig."""
    rng = np.random.default_rng(seed)
    ok = lambda label, **kw: X.from_text(rng, label, "3S20M2D5M1I4M", **kw)
    c = [SCase(ok("ok_in_front"), True, 5000),
         SCase(ok("no_len_0"), True, 0), SCase(ok("ok_between"), False, 0, "forward_needs_no_len"), SCase(ok("no_len_negative"), True, -5),
         SCase(ok("ok_behind"), True, 1031),
         SCase(X.Case("no_cigar", X._ops(rng, 10), []), True, 0, "no_cigar_decides_first"),
         SCase(X.Case("too_short", X._ops(rng, 10), R.words_of("4M1D5M")), True, 0, "length_decides_first"),
         SCase(X.Case("op9", X._ops(rng, 10), [4 << 4 | 0, 0 << 4 | 9, 6 << 4 | 0]), True, 0, "bad_op_decides_first"),
         SCase(X.Case("refused", [], R.words_of("10M"), status=3, qs=0), True, 0, "expansion_decides_first"),
         SCase(ok("flush", pos=1000), True, 1031, "ends_at_contig_end"),      # ref_len 31: mirrored pos 0
         SCase(ok("beyond", pos=1000), True, 1020, "runs_past_contig_end"),   # mirrored pos -11: carried, not refused
         SCase(ok("at0", pos=0), True, 31, "whole_contig"),
         SCase(ok("big", pos=0x7ffffff0), True, 0x7fffffff, "near_int32_max")]
    return c


def layout(cases, cigar_lead=0):
    a = X.layout(cases, cigar_lead)
    a["reverse"] = np.array([c.reverse for c in cases], np.uint8)
    a["contig_len"] = np.array([c.contig_len for c in cases], np.int64).astype(np.int32)
    return a


expected = X.expected


# ---- mapped SAM / BAM in two forms ------------------------------------------------------------------------------------------------

class StrandedSet:
    """refops_cases.MappedSet, whose reads all lie forward on contigs built from them, turned into A and B. Every second read (r % 2)
    becomes a reverse-strand read: its slice of the contig is replaced by the slice's reverse complement, so that the read's own reverse
    complement aligns there with its CIGAR in reverse order.
      a: a MappedSet whose odd records carry flag 0x10, SEQ reversed and complemented, the CIGAR in reference order -- against ref.fa
      b: the same reads as forward records (flag 0): the odd ones on contig NAME + suffix at the mirrored position -- against both.fa"""

    def __init__(self, kind, seed, n_reads=300, suffix="_rc", unmapped=False, **kw):
        base = X.MappedSet(kind, seed, n_reads=n_reads, **kw)
        self.suffix = suffix
        contigs = {n: bytearray(s.encode()) for n, s in base.contigs}
        a_recs, b_recs = [], []
        for x in base.recs:
            if unmapped and x["r"] % 40 == 7:
                u = dict(name=f"u{x['r']}", flag=4, rname="*", pos=-1, words=[], seq=x["seq"], r=x["r"])
                a_recs.append(u); b_recs.append(u)
            if x["r"] % 2:
                ctg, p, n = contigs[x["rname"]], x["pos"], _ref_len(x["words"])
                ctg[p:p + n] = S.revcomp(ctg[p:p + n])
                a_recs.append(dict(x, flag=0x10, words=list(reversed(x["words"])), seq=S.revcomp(x["seq"].encode()).decode()))
                b_recs.append(dict(x, rname=x["rname"] + suffix, pos=len(ctg) - p - n))
            else:
                a_recs.append(x); b_recs.append(x)
        fwd = [(n, contigs[n].decode()) for n, _ in base.contigs]
        in_fasta = [c for c in fwd if c[0] != "ctgX"]
        self.a, self.b = copy.copy(base), copy.copy(base)
        self.a.recs, self.a.contigs, self.a.in_fasta = a_recs, fwd, in_fasta
        self.b.recs, self.b.contigs, self.b.in_fasta = b_recs, S.mirror(fwd, suffix), S.mirror(in_fasta, suffix)
        self.batch, self.rna = base.b, base.rna
        self.n_reverse = sum(1 for x in a_recs if x["flag"] & 0x10)
        self.n_unmapped = sum(1 for x in a_recs if x["flag"] & 0x4)
        self.n_mapped = len(a_recs) - self.n_unmapped

    def write(self, d, trim=0):
        """a.sam a.bam ref.fa b.sam b.bam both.fa in directory d."""
        self.a.write_sam(d / "a.sam", trim=trim); self.a.write_bam(d / "a.bam", trim=trim); self.a.write_fasta(d / "ref.fa")
        self.b.write_sam(d / "b.sam", trim=trim); self.b.write_bam(d / "b.bam", trim=trim); self.b.write_fasta(d / "both.fa")
