"""The rule of `poregen eventalign` restated in Python: integers and Fractions for the mean, the spread, z and the text, Python floats for
the two conversions (the same operations in the same order, round() for ties to even). The pairing and the solve are fit_ref's and
fitgap_ref's. Nothing here calls the product.

Per event of n raw samples r_i under its read's fit (a, b) and its k-mer's level L and spread SD in 1e-3 pA:
  u_i = 1000 r_i;  m_raw = floor(mean(u) + 1/2);  s_raw = floor(sqrt(sum (u_i - mean)^2 / (n - 1)) + 1/2) for n >= 2, else 0
  A = 1000.0 * a, G = (1.0 / b) / 1000.0;  mean_u = round(cut((m_raw - A) * G)), stdv_u = round(cut(s_raw * G)), cut to +-2^21
  z_c = floor((mean_u - L) / SD * 100 + 1/2)"""
import math
from fractions import Fraction

import fit_ref as R
import fitgap_ref as G

HEADER = "\t".join(["contig", "position", "reference_kmer", "read_index", "strand", "event_index", "event_level_mean", "event_stdv", "event_length", "model_kmer", "model_mean",
                    "model_stdv", "standardized_level", "start_idx", "end_idx"]) + "\n"
CUT = float(1 << 21)
MAX_DUR = 4096


def half_up(x):
    """The integer nearest to the rational x, halves up."""
    return math.floor(Fraction(x) + Fraction(1, 2))


def isqrt_half_up(x):
    """The integer nearest to sqrt(x) for a rational x >= 0, halves up: the largest s with (2 s - 1)^2 <= 4 x."""
    t = math.isqrt(math.floor(4 * Fraction(x)))        # t <= 2 sqrt(x) < t + 1
    return (t + 1) // 2


def event_stats(samples):
    """(m_raw, s_raw) in 1e-3 raw counts."""
    u = [1000 * int(r) for r in samples]
    n = len(u)
    mean = Fraction(sum(u), n)
    if n < 2:
        return half_up(mean), 0
    var = sum((x - mean) ** 2 for x in u) / (n - 1)
    return half_up(mean), isqrt_half_up(var)


def cut(x):
    return CUT if x > CUT else -CUT if x < -CUT else x


def convert(m_raw, s_raw, a, b):
    A = 1000.0 * a
    Gn = (1.0 / b) / 1000.0
    return round(cut((float(m_raw) - A) * Gn)), round(cut(float(s_raw) * Gn))


def z_hundredths(mean_u, L, SD):
    return half_up(Fraction(100 * (mean_u - L), SD))


def event_row(samples, a, b, L, SD):
    m_raw, s_raw = event_stats(samples)
    mean_u, stdv_u = convert(m_raw, s_raw, a, b)
    return mean_u, stdv_u, z_hundredths(mean_u, L, SD)


def walk(seq, ops, q, sig, levels, stdvs, k, m, rna, min_dur, max_dur, a, b, types=None):
    """The rows of one fitted read: [(event, start, n, slot, first, mean_u, stdv_u, z_c)]; sig a list of ints."""
    rows = []
    if types is None:
        lb = len(seq)
        cand = [(i + m, seq_kmer, lo, hi, (lb - i - k) if rna else i) for i, (seq_kmer, lo, hi) in enumerate(R.pairing(seq, ops, q, k, m, rna))]
    else:
        _, cols = G.layout(ops, types, q)
        S = len(seq)
        cand = [(j, kmer, lo, hi, (S - (cols[j] - m) - k) if rna else cols[j] - m) for j, kmer, lo, hi in G.pairing(seq, ops, types, q, k, m, rna)]
    for e, kmer, lo, hi, first in cand:
        if not min_dur <= hi - lo <= max_dur or any(c not in "ACGT" for c in kmer):
            continue
        s = R.slot_of(kmer)
        if levels[s] is None:
            continue
        assert seq[first:first + k] == kmer
        rows.append((e, lo, hi - lo, s, first) + event_row(sig[lo:hi], a, b, levels[s], stdvs[s]))
    return rows


def dec_text(v, digits):
    p = 10 ** digits
    return f"{'-' if v < 0 else ''}{abs(v) // p}.{abs(v) % p:0{digits}d}"


def revcomp(kmer):
    return "".join({"A": "T", "C": "G", "G": "C", "T": "A"}[c] for c in reversed(kmer))


def length_text(n, rate):
    return str(n) if not rate else dec_text(math.floor(Fraction(n, rate) * 100000 + Fraction(1, 2)), 5)


def row_text(row, seq, k, levels, stdvs, contig="", label="0", ref_start=0, reverse=False, rate=0):
    e, start, n, s, first, mean_u, stdv_u, z = row
    kmer = seq[first:first + k]
    pos = ref_start + (len(seq) - first - k if reverse else first)
    return "\t".join([contig, str(pos), revcomp(kmer) if reverse else kmer, label, "t", str(e), dec_text(mean_u, 3), dec_text(stdv_u, 3), length_text(n, rate), kmer,
                      dec_text(levels[s], 3), dec_text(stdvs[s], 3), dec_text(z, 2), str(start), str(start + n)]) + "\n"


# ---- worked cases ---------------------------------------------------------------------------------------------------------------------------
assert event_stats([3]) == (3000, 0) and event_stats([1, 2]) == (1500, 707) and event_stats([-1, -2]) == (-1500, 707)
assert event_stats([0, 0, 1]) == (333, 577) and event_stats([0, 0, 0, 1]) == (250, 500)
assert half_up(Fraction(-3, 2)) == -1 and half_up(Fraction(5, 2)) == 3
assert z_hundredths(1005, 1000, 1000) == 1 and z_hundredths(995, 1000, 1000) == 0 and z_hundredths(985, 1000, 1000) == -1 and z_hundredths(984, 1000, 1000) == -2
assert dec_text(-1, 2) == "-0.01" and dec_text(-1, 3) == "-0.001" and dec_text(12345, 3) == "12.345"
assert length_text(10, 4000) == "0.00250" and length_text(1, 1000000) == "0.00000" and length_text(1, 200000) == "0.00001" and length_text(7, 1) == "7.00000"
assert revcomp("ACG") == "CGT"
