"""The rule of `poregen realign` on the signal-to-reference alignment (a gapped batch), restated in Python integers independently of
csrc/pg_realign.h: the recurrence over all pairs of candidates as it is stated. Which events are refinable comes from fitgap_ref's pairing;
boundaries, free boundaries and the dynamic program are restated here. Nothing here calls the product.

Boundaries B_0 = q, B_{e+1} = B_e + n_e for a match or an I, B_{e+1} = B_e for a D (zero samples between its two boundaries). Event e is
refinable iff the gapped fit counts it; an I or a D never is, so both boundaries beside it are pinned. Boundary e, 0 < e < Lb, is free iff
events e - 1 and e are refinable and e % 256 != phase (the period counts OPS). The dynamic program per maximal run of free boundaries is
realign_ref's. The refined ops keep op_t, and the op_n of every I and D."""
import fit_ref as R
import fitgap_ref as G
import realign_ref as RR
import realign_phase_ref as RP

PERIOD = 256


def event_levels(seq, ops, types, levels, k, m, rna, min_dur, max_dur):
    """Per op its level, or None when it is not a refinable event."""
    out = [None] * len(ops)
    for j, kmer, lo, hi in G.pairing(seq, ops, types, 0, k, m, rna):
        if min_dur <= ops[j] <= max_dur and all(c in "ACGT" for c in kmer):
            out[j] = levels[R.slot_of(kmer)]
    return out


def free_boundaries(lv, phase=0):
    lb = len(lv)
    return [0 < e < lb and lv[e - 1] is not None and lv[e] is not None and e % PERIOD != phase for e in range(lb + 1)]


def realign(seq, ops, types, q, sig, levels, k, m, rna, min_dur, max_dur, band, min_len, a, b, phase=0):
    """(new ops, n_free, n_moved, sum_abs_shift, cost_before, cost_after) of a read that has a fit (status ok)."""
    assert 0 <= band <= 31 and 1 <= min_len <= min_dur <= max_dur <= 4096 and 0 <= phase < PERIOD
    assert G.status_before(seq, ops, types, q, len(sig)) == R.OK
    inv_b, lb, W = 1.0 / b, len(ops), band
    lv = event_levels(seq, ops, types, levels, k, m, rna, min_dur, max_dur)
    B = G.layout(ops, types, q)[0]
    free = free_boundaries(lv, phase)
    memo = {}

    def dd(t, l):
        if (t, l) not in memo:
            d = R.residual(sig[t], a, inv_b, l)[0]
            memo[(t, l)] = d * d
        return memo[(t, l)]

    def cost(e, lo, hi):
        return sum(dd(t, lv[e]) for t in range(lo, hi))

    new = list(B)
    e0 = 0
    while e0 < lb:
        if not free[e0 + 1]:
            e0 += 1
            continue
        e1 = e0 + 1
        while free[e1]:
            e1 += 1
        P0, P1 = B[e0], B[e1]
        rows = [{P0: (0, None)}]
        for e in range(e0 + 1, e1 + 1):
            prev = rows[-1]
            cand = [P1] if e == e1 else [B[e] + j for j in range(-W, W + 1) if P0 + (e - e0) * min_len <= B[e] + j <= P1 - (e1 - e) * min_len]
            # the cost of event e - 1 on [p', p) is S[p - base] - S[p' - base]: running sums of d^2 under l_{e-1} from the lowest p' on
            row, base, S = {}, min(prev), [0]
            for t in range(base, max(cand, default=base)):
                S.append(S[-1] + dd(t, lv[e - 1]))
            for p in cand:
                best = None
                for pp in sorted(prev):                                   # ascending p': the first minimum is the smallest p'
                    if pp + min_len > p:
                        break
                    v = prev[pp][0] + S[p - base] - S[pp - base]
                    if best is None or v < best[0]:
                        best = (v, pp)
                if best is not None:
                    row[p] = best
            rows.append(row)
        p = P1
        for e in range(e1, e0, -1):
            p = rows[e - e0][p][1]
            if e - 1 > e0:
                new[e - 1] = p
        e0 = e1
    shifts = [abs(new[e] - B[e]) for e in range(lb + 1) if free[e] and new[e] != B[e]]
    before = sum(cost(e, B[e], B[e + 1]) for e in range(lb) if lv[e] is not None)
    after = sum(cost(e, new[e], new[e + 1]) for e in range(lb) if lv[e] is not None)
    out = [ops[e] if types[e] != G.MATCH else new[e + 1] - new[e] for e in range(lb)]
    return out, sum(free), len(shifts), sum(shifts), before, after


def rounds(seq, ops, types, q, sig, levels, k, m, rna, min_dur, max_dur, min_events, band, min_len, n_rounds, phases=(0, 128)):
    """[(status, a, b, N, (ops_t, n_free, n_moved, sum_abs_shift, cost_before, cost_after))] for t = 1 .. n_rounds, as realign_phase_ref.rounds"""
    out, cur = [], list(ops)
    for t in range(1, n_rounds + 1):
        st, su, a, b, _ = G.fit(seq, cur, types, q, sig, levels, k, m, rna, min_dur, max_dur, min_events)
        res = (list(cur), 0, 0, 0, 0, 0)
        if st == R.OK:
            res = realign(seq, cur, types, q, sig, levels, k, m, rna, min_dur, max_dur, band, min_len, a, b, phases[(t - 1) % len(phases)])
        out.append((st, a, b, su[0] if st == R.OK else 0, res))
        cur = res[0]
    return out


# ---- on a read of only matches with S = Lb the gapped rule IS the old rule: the worked cases of realign_ref and realign_phase_ref -----------
_W = dict(RR.WORKED)
_W["types"] = [0] * len(_W["ops"])
assert realign(**_W) == RR.WORKED_RESULT and realign(phase=RP.WORKED_PHASE, **_W) == RP.WORKED_PHASE_RESULT

# ---- the worked gapped case: fitgap_ref's six matches with one I and one D, k = 3, m = 1 ---------------------------------------------------
# ops M3 I4 M5 M6 M7 M8 D2 M9 from q = 0 over ACGTTGCA: the refinable events are op 3 (CGT on [12, 18)) and op 4 (GTT on [18, 25)), so
# boundary 4, at 18, is the one free boundary; the boundaries beside the I and the D are pinned. Levels CGT 50 pA, GTT 70 pA (rna: TGC and
# TTG); a = 0, b = 0.001, so a raw sample reads as its value in pA. The samples were made with the boundary at 19: sample 18 is a 50 under
# the 70 of op 4, |d| = 20000, 4 * 10^8 before; after, the boundary sits at 19 and the cost is 0. Every other sample is a 90 and counts nowhere.
WORKED_LEVELS = {"CGT": 50000, "GTT": 70000, "TGC": 50000, "TTG": 70000}
WORKED = dict(seq="ACGTTGCA", ops=[3, 4, 5, 6, 7, 8, 2, 9], types=[0, 1, 0, 0, 0, 0, 2, 0], q=0, k=3, m=1, min_dur=2, max_dur=70, band=2, min_len=1, a=0.0, b=0.001,
              levels=[WORKED_LEVELS.get(a + b + c) for a in "ACGT" for b in "ACGT" for c in "ACGT"], sig=[90] * 12 + [50] * 7 + [70] * 6 + [90] * 17)
WORKED_RESULT = ([3, 4, 5, 7, 6, 8, 2, 9], 1, 1, 1, 4 * 10 ** 8, 0)
assert realign(rna=False, **WORKED) == WORKED_RESULT and realign(rna=True, **WORKED) == WORKED_RESULT
