"""The rule of `poregen realign` restated in Python integers, independently of csrc/pg_realign.h: the recurrence over all pairs of
candidates as it is stated, O(E (2W + 1)^2) per run, no prefix-minimum. Calibration and the residual d come from fit_ref. Nothing here
calls the product.

Boundaries B_0 = q, B_e = B_{e-1} + ops[e-1]. Event e is refinable iff fit counts it (level l_e). Boundary e, 0 < e < Lb, is free iff
events e - 1 and e are refinable and e % 256 != 0; all others are pinned. Per maximal run of free boundaries e0 < e < e1 (P0 = B_e0,
P1 = B_e1): candidates p = B_e + j, |j| <= W, admissible iff P0 + (e - e0) min_len <= p <= P1 - (e1 - e) min_len; D[e0][P0] = 0;
D[e][p] = min over reachable admissible p' with p' + min_len <= p of D[e-1][p'] + cost of event e - 1 on [p', p), ties to the smallest p';
at e1 the only candidate is P1; trace back."""
import fit_ref as R

PERIOD = 256
MAX_BAND = 31
MAX_DUR = 4096


def params_ok(band, min_len, min_dur, max_dur):
    return 0 <= band <= MAX_BAND and 1 <= min_len <= min_dur <= max_dur <= MAX_DUR


def event_levels(seq, ops, levels, k, m, rna, min_dur, max_dur):
    """Per event its level, or None when the event is not refinable."""
    lb, out = len(ops), []
    for e in range(lb):
        i = e - m
        if i < 0 or i > lb - k or not min_dur <= ops[e] <= max_dur:
            out.append(None); continue
        kmer = seq[lb - i - k:lb - i] if rna else seq[i:i + k]
        out.append(levels[R.slot_of(kmer)] if all(c in "ACGT" for c in kmer) else None)
    return out


def boundaries(ops, q):
    B = [q]
    for n in ops:
        B.append(B[-1] + n)
    return B


def free_boundaries(lv):
    lb = len(lv)
    return [0 < e < lb and lv[e - 1] is not None and lv[e] is not None and e % PERIOD != 0 for e in range(lb + 1)]


def realign(seq, ops, q, sig, levels, k, m, rna, min_dur, max_dur, band, min_len, a, b):
    """(new ops, n_free, n_moved, sum_abs_shift, cost_before, cost_after); sig a list of ints, a and b the read's fit."""
    assert params_ok(band, min_len, min_dur, max_dur)
    inv_b, lb, W = 1.0 / b, len(ops), band
    lv = event_levels(seq, ops, levels, k, m, rna, min_dur, max_dur)
    B = boundaries(ops, q)
    free = free_boundaries(lv)
    sq = {}

    def dd(t, l):
        key = (t, l)
        if key not in sq:
            d = R.residual(sig[t], a, inv_b, l)[0]
            sq[key] = d * d
        return sq[key]

    def cost(e, lo, hi):
        return sum(dd(t, lv[e]) for t in range(lo, hi))

    new = list(B)
    e0 = 0
    while e0 < lb:
        if not free[e0 + 1]:
            e0 += 1; continue
        e1 = e0 + 1
        while free[e1]:
            e1 += 1
        P0, P1 = B[e0], B[e1]

        def candidates(e):
            if e == e0:
                return [P0]
            if e == e1:
                return [P1]
            return [B[e] + j for j in range(-W, W + 1) if P0 + (e - e0) * min_len <= B[e] + j <= P1 - (e1 - e) * min_len]
        D = {P0: (0, None)}
        rows = [D]
        for e in range(e0 + 1, e1 + 1):
            prev, D = D, {}
            # cost of event e - 1 on [p', p) = S[p] - S[p']: running sums of d^2 under l_{e-1} over all a pair of candidates can span
            base, S = max(P0, B[e - 1] - W), [0]
            for t in range(base, min(P1, B[e] + W)):
                S.append(S[-1] + dd(t, lv[e - 1]))
            for p in candidates(e):
                best = None
                for pp in sorted(prev):                               # ascending p': the first minimum is the smallest p'
                    if pp + min_len > p:
                        continue
                    v = prev[pp][0] + S[p - base] - S[pp - base]
                    if best is None or v < best[0]:
                        best = (v, pp)
                if best is not None:
                    D[p] = best
            rows.append(D)
        p = P1
        for e in range(e1, e0, -1):
            p = rows[e - e0][p][1]
            if e - 1 > e0:
                new[e - 1] = p
        e0 = e1
    n_free = sum(free)
    moved = [abs(new[e] - B[e]) for e in range(lb + 1) if free[e] and new[e] != B[e]]
    before = sum(cost(e, B[e], B[e + 1]) for e in range(lb) if lv[e] is not None)
    after = sum(cost(e, new[e], new[e + 1]) for e in range(lb) if lv[e] is not None)
    return [new[e + 1] - new[e] for e in range(lb)], n_free, len(moved), sum(moved), before, after


# ---- the worked case, as literals -----------------------------------------------------------------------------------------------------------
# k = 1, m = 0, levels A 10, C 20, G 30, T 40 pA; a = 0, b = 0.001, so a raw sample reads as its level in pA; min_dur 2, min_len 1, W = 2.
# seq ACGTAC. The samples were made with the boundaries 0, 5, 8, 11, 16, 21, 24; the ops handed in are 4,4,4,4,4,4 from q = 0, which puts
# the five free boundaries at 4, 8, 12, 16, 20: off by -1, 0, +1, 0, -1.
WORKED = dict(seq="ACGTAC", ops=[4, 4, 4, 4, 4, 4], q=0, levels=[10000, 20000, 30000, 40000], k=1, m=0, rna=False, min_dur=2, max_dur=70, band=2, min_len=1, a=0.0, b=0.001,
              sig=[10] * 5 + [20] * 3 + [30] * 3 + [40] * 5 + [10] * 5 + [20] * 3)
# Before: sample 4 is an A (10) under C (20), sample 11 a T (40) under G (30), sample 20 an A (10) under C (20): three samples with
# |d| = 10000, 10^8 each. After: every boundary where the samples change, cost 0; three boundaries moved, by one sample each.
WORKED_RESULT = ([5, 3, 3, 5, 5, 3], 5, 3, 3, 3 * 10 ** 8, 0)
assert realign(**WORKED) == WORKED_RESULT


def rms_text(n, cost):
    return R.units_text(R.rms_resid(n, cost)) if n else ""
