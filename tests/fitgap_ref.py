"""The rule of `poregen fit` on the signal-to-reference alignment (a gapped batch: ops with I and D among them, seq the read's reference
slice), restated in Python integers independently of csrc/pg_fit.h. Sums, solve, residuals and the table text are fit_ref's, unchanged;
the pairing of events with k-mers is restated here. Nothing here calls the product.

Op types: 0 match, 1 I, 2 D. A match of n and an I of n advance the sample position by n, a D by 0. A match advances the reference column
by 1, a D of n by n, an I by 0; c_j is the column in front of op j, C the read's total, S the slice's length. Event j counts iff it is a
match, ops j - m .. j - m + k - 1 all exist and are all matches, min_dur <= n_j <= max_dur, and its k-mer -- seq[c_j - m, c_j - m + k),
with rna seq[S - (c_j - m) - k, S - (c_j - m)) -- lies inside the slice, has ACGT letters and a level. Statuses before the sums:
out_of_signal (q < 0 or the samples of the ops run past the read's), then ref_length (S != C)."""
import fit_ref as R

MATCH, INS, DEL = 0, 1, 2
REF_LENGTH = 6
STATUS = dict(R.STATUS)
STATUS[REF_LENGTH] = "ref_length"


def layout(ops, types, q):
    """(starts, cols): the first sample of every op and the column in front of it, one entry more than ops (the totals)."""
    starts, cols = [q], [0]
    for n, t in zip(ops, types):
        assert t in (MATCH, INS, DEL)
        starts.append(starts[-1] + (0 if t == DEL else n))
        cols.append(cols[-1] + (1 if t == MATCH else n if t == DEL else 0))
    return starts, cols


def pairing(seq, ops, types, q, k, m, rna=False):
    """[(op, k-mer, first sample, one past the last)] of every event that carries a k-mer, whatever its length or letters."""
    starts, cols = layout(ops, types, q)
    S, lb, out = len(seq), len(ops), []
    for j in range(lb):
        w = j - m
        if types[j] != MATCH or w < 0 or w + k > lb or any(types[w + i] != MATCH for i in range(k)):
            continue
        f = cols[j] - m
        if f < 0 or f + k > S:
            continue
        out.append((j, seq[S - f - k:S - f] if rna else seq[f:f + k], starts[j], starts[j + 1]))
    return out


def status_before(seq, ops, types, q, n_sig):
    starts, cols = layout(ops, types, q)
    if q < 0 or starts[-1] > n_sig:
        return R.OUT_OF_SIGNAL
    return REF_LENGTH if cols[-1] != len(seq) else R.OK


def walk(seq, ops, types, q, n_sig, levels, k, m, rna, min_dur, max_dur):
    """The counted events [(first sample, samples, slot)], or the status that keeps the read out (an int)."""
    st = status_before(seq, ops, types, q, n_sig)
    if st != R.OK:
        return st
    out = []
    for _, kmer, lo, hi in pairing(seq, ops, types, q, k, m, rna):
        if not min_dur <= hi - lo <= max_dur or any(c not in "ACGT" for c in kmer):
            continue
        s = R.slot_of(kmer)
        if levels[s] is not None:
            out.append((lo, hi - lo, s))
    return out


def fit(seq, ops, types, q, sig, levels, k, m, rna, min_dur, max_dur, min_events):
    """(status, sums7, a, b, events)"""
    ev = walk(seq, ops, types, q, len(sig), levels, k, m, rna, min_dur, max_dur)
    if isinstance(ev, int):
        return ev, (0,) * 7, None, None, []
    su = R.sums(sig, ev, levels)
    st, a, b = R.solve(su, min_events)
    return st, su, a, b, ev


# ---- on a read of only matches with S = Lb the gapped rule IS fit_ref's: its worked case -------------------------------------------------
assert [x[1:] for x in pairing("ACGTA", [3, 4, 5, 6, 7], [0] * 5, 10, 2, 1)] == R.WORKED_DNA
assert [x[1:] for x in pairing("ACGTA", [3, 4, 5, 6, 7], [0] * 5, 10, 2, 1, rna=True)] == R.WORKED_RNA

# ---- the worked gapped case: six matches with one I and one D among them, k = 3, m = 1 ---------------------------------------------------
# ops M3 I4 M5 M6 M7 M8 D2 M9 from q = 10 over the slice ACGTTGCA (S = 8).
#   first samples 10, 13, 17, 22, 28, 35, 43, 43 (the D takes none), end 52; columns 0, 1, 1, 2, 3, 4, 5, 7 (the I takes none, the D two): C = 8.
#   Event j needs ops j - 1, j, j + 1 to be matches: only j = 3 (ops 2, 3, 4) and j = 4 (ops 3, 4, 5). Op 2 has the I in front of it, op 5
#   the D behind it, ops 0 and 7 lack a neighbour.
#   j = 3: c = 2, first base 1: CGT on [22, 28); rna: seq[8 - 1 - 3, 7) = TGC.   j = 4: c = 3, first base 2: GTT on [28, 35); rna: seq[3, 6) = TTG.
WORKED = dict(seq="ACGTTGCA", ops=[3, 4, 5, 6, 7, 8, 2, 9], types=[0, 1, 0, 0, 0, 0, 2, 0], q=10, k=3, m=1)
WORKED_DNA = [(3, "CGT", 22, 28), (4, "GTT", 28, 35)]
WORKED_RNA = [(3, "TGC", 22, 28), (4, "TTG", 28, 35)]
assert layout(WORKED["ops"], WORKED["types"], 10) == ([10, 13, 17, 22, 28, 35, 43, 43, 52], [0, 1, 1, 2, 3, 4, 5, 7, 8])
assert pairing(**WORKED) == WORKED_DNA and pairing(rna=True, **WORKED) == WORKED_RNA
