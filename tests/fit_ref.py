"""The rule of `poregen fit` restated in Python integers, Fractions and floats, independently of csrc/pg_fit.h. Nothing here calls the product.

Model: levels in 1e-3 pA per slot (rank of the k-mer in ACGT order), None for a k-mer the file does not hold.
Events: event e of a read (seq, ops, q) is the samples [q + sum ops[:e], + ops[e]); for i = 0 .. Lb - k the event e = i + m (if e < Lb)
carries seq[i:i + k], with rna seq[Lb - i - k:Lb - i]; it counts when min_dur <= ops[e] <= max_dur, its letters are ACGT and it has a level."""
import math
import re
from fractions import Fraction

STATUS = {0: "ok", 1: "out_of_signal", 2: "too_long", 3: "few_events", 4: "flat", 5: "negative_scale"}
OK, OUT_OF_SIGNAL, TOO_LONG, FEW_EVENTS, FLAT, NEGATIVE_SCALE, SKIPPED = 0, 1, 2, 3, 4, 5, 16
MAX_N = 1 << 24
MAX_LEVEL = 1 << 18
CLAMP = (1 << 18) - 1
_NUMBER = re.compile(r"-?(\d+\.?\d*|\.\d+)\Z")


class ModelRefused(ValueError):
    def __init__(self, line, why):
        super().__init__(f"line {line}: {why}")
        self.line = line


def slot_of(kmer):
    s = 0
    for c in kmer:
        s = s * 4 + "ACGT".index("T" if c == "U" else c)
    return s


def parse_model(text, want_k=0):
    """(k, levels[4^k] with None for a missing k-mer, uses_u); ModelRefused names the line."""
    k, levels, uses_u = 0, None, False
    for no, line in enumerate(text.split("\n"), 1):
        line = line.rstrip("\r")
        if not line or line.startswith("#") or line.startswith("kmer\t"):
            continue
        f = line.split("\t")
        if len(f) < 2:
            raise ModelRefused(no, "fewer than two fields")
        kmer = f[0]
        if not 1 <= len(kmer) <= 9 or (k and len(kmer) != k) or (not k and want_k and len(kmer) != want_k):
            raise ModelRefused(no, "k-mer length")
        if any(c not in "ACGTU" for c in kmer):
            raise ModelRefused(no, "letter outside ACGTU")
        if not k:
            k, levels = len(kmer), [None] * 4 ** len(kmer)
        for field in f[1:3]:
            if not _NUMBER.match(field):
                raise ModelRefused(no, "a field that is no number")
        level = math.floor(Fraction(f[1]) * 1000 + Fraction(1, 2))   # nearest 1e-3 pA, halves up, on the decimal text
        if not 0 < level < MAX_LEVEL:
            raise ModelRefused(no, "level out of range")
        uses_u = uses_u or "U" in kmer
        s = slot_of(kmer)
        if levels[s] is not None:
            raise ModelRefused(no, "duplicate k-mer")
        levels[s] = level
    if not k:
        raise ModelRefused(0, "no k-mer")
    return k, levels, uses_u


def pairing(seq, ops, q, k, m, rna=False):
    """[(k-mer, first sample, one past the last)] of every event that carries a k-mer, whatever its length or letters."""
    lb, out = len(seq), []
    starts = [q]
    for n in ops:
        starts.append(starts[-1] + n)
    for i in range(0, lb - k + 1):
        e = i + m
        if e >= lb:
            continue
        kmer = seq[lb - i - k:lb - i] if rna else seq[i:i + k]
        out.append((kmer, starts[e], starts[e + 1]))
    return out


# the worked case: seq = ACGTA, k = 2, m = 1, ops 3,4,5,6,7, q = 10
WORKED_DNA = [("AC", 13, 17), ("CG", 17, 22), ("GT", 22, 28), ("TA", 28, 35)]
WORKED_RNA = [("TA", 13, 17), ("GT", 17, 22), ("CG", 22, 28), ("AC", 28, 35)]
assert pairing("ACGTA", [3, 4, 5, 6, 7], 10, 2, 1) == WORKED_DNA and pairing("ACGTA", [3, 4, 5, 6, 7], 10, 2, 1, rna=True) == WORKED_RNA


def walk(seq, ops, q, n_sig, levels, k, m, rna, min_dur, max_dur):
    """The counted events [(first sample, samples, slot)], or None: out_of_signal."""
    if q < 0 or q + sum(ops) > n_sig:
        return None
    out = []
    for kmer, lo, hi in pairing(seq, ops, q, k, m, rna):
        if not min_dur <= hi - lo <= max_dur or any(c not in "ACGT" for c in kmer):
            continue
        s = slot_of(kmer)
        if levels[s] is None:
            continue
        out.append((lo, hi - lo, s))
    return out


def sums(sig, events, levels):
    """(N, SL, SLL, SR, SRL, SRR, E) over the samples of the counted events; sig a list of ints."""
    n = sl = sll = sr = srl = srr = 0
    for lo, cnt, s in events:
        l = levels[s]
        seg = sig[lo:lo + cnt]
        t = sum(seg)
        n += cnt; sl += cnt * l; sll += cnt * l * l; sr += t; srl += t * l; srr += sum(x * x for x in seg)
    return (n, sl, sll, sr, srl, srr, len(events))


def parts(su):
    n, sl, sll, sr, srl, srr, _ = su
    return n * sll - sl * sl, n * srl - sl * sr, sr * sll - sl * srl, n * srr - sr * sr   # den, numb, numa, Syy


def solve(su, min_events):
    """(status, a, b): a, b floats (None unless ok), each conversion and division one correctly rounded operation."""
    n, e = su[0], su[6]
    if n > MAX_N:
        return TOO_LONG, None, None
    if e < min_events:
        return FEW_EVENTS, None, None
    den, numb, numa, _ = parts(su)
    if den == 0:
        return FLAT, None, None
    if numb <= 0:
        return NEGATIVE_SCALE, None, None
    return OK, float(numa) / float(den), float(numb) / float(den)


def report_exact(su, digitisation, offset, range_):
    """(shift, scale, rms^2) as exact rationals, in pA (rms itself is irrational: compare squares)."""
    den, numb, numa, syy = parts(su)
    g = Fraction(range_) / Fraction(digitisation)
    return g * (Fraction(numa, den) + Fraction(offset)), 1000 * g * Fraction(numb, den), g * g * (Fraction(syy) - Fraction(numb * numb, den)) / (su[0] * su[0])


def one_minus_r2(su):
    den, numb, _, syy = parts(su)
    return 1 - Fraction(numb * numb, den * syy)


def residual(r, a, inv_b, l):
    """(d, clamped) of one sample."""
    d = round((float(r) - a) * inv_b) - l
    return max(-CLAMP, min(CLAMP, d)), abs(d) > CLAMP


def residuals(sig, events, levels, a, b, slots):
    """Adds the read's events to slots: slot -> [n_samples, n_events, sum d, sum d^2]; returns the clamped samples."""
    inv_b, clamped = 1.0 / b, 0
    for lo, cnt, s in events:
        l, acc = levels[s], slots.setdefault(s, [0, 0, 0, 0])
        acc[0] += cnt; acc[1] += 1
        for r in sig[lo:lo + cnt]:
            d, c = residual(r, a, inv_b, l)
            acc[2] += d; acc[3] += d * d; clamped += c
    return clamped


def units_text(v):
    return f"{'-' if v < 0 else ''}{abs(v) // 1000}.{abs(v) % 1000:03d}"


def mean_resid(n, sum_d):
    return (2 * sum_d + n) // (2 * n)


def rms_resid(n, sum_dd):
    return (math.isqrt(4 * sum_dd // n) + 1) // 2


def kmer_table(k, levels, slots, uses_u):
    import itertools
    rows = []
    for s, t in enumerate(itertools.product("ACGU" if uses_u else "ACGT", repeat=k)):
        n, ne, sd, sdd = slots.get(s, (0, 0, 0, 0))
        rows.append("\t".join(["".join(t), str(n), str(ne), units_text(levels[s]) if levels[s] is not None else "",
                               units_text(mean_resid(n, sd)) if n else "", units_text(rms_resid(n, sdd)) if n else ""]) + "\n")
    return "".join(rows)
