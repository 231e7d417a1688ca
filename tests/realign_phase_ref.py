"""The rule of `poregen realign` with a phase for the pinned period, and rounds of fit and realign, restated in Python integers. Event
levels, boundaries and the calibration come from realign_ref and fit_ref; which boundaries are free and the dynamic program are restated
here. Nothing here calls the product.

Boundary e, 0 < e < Lb, is free iff events e - 1 and e are refinable and e % 256 != phase; all others are pinned. Everything else is
realign_ref's rule: per maximal run of free boundaries e0 < e < e1 (P0 = B_e0, P1 = B_e1) the candidates p = B_e + j, |j| <= W, admissible
iff P0 + (e - e0) min_len <= p <= P1 - (e1 - e) min_len; D[e0][P0] = 0; D[e][p] = min over reachable p' with p' + min_len <= p of
D[e-1][p'] + cost of event e - 1 on [p', p), ties to the smallest p'; at e1 only P1; trace back.

Rounds: ops_0 are the ops handed in; for t = 1 .. R, (status_t, a_t, b_t) is fit_ref's calibration over ops_{t-1} and ops_t the rule over
ops_{t-1} with that fit at phase 0 for odd t and 128 for even t; a read whose status_t is not ok keeps ops_{t-1} in round t."""
import fit_ref as R
import realign_ref as RR
from realign_ref import boundaries, event_levels

PERIOD = RR.PERIOD
ROUND_PHASES = (0, 128)


def phase_ok(phase):
    return 0 <= phase < PERIOD


def free_boundaries(lv, phase=0):
    lb = len(lv)
    return [0 < e < lb and lv[e - 1] is not None and lv[e] is not None and e % PERIOD != phase for e in range(lb + 1)]


def pieces(lb, phase):
    """[(first op, ops)]: what lies between two pinned boundaries of the period, the unit the device works in."""
    cuts = sorted({0, lb} | {e for e in range(1, lb) if e % PERIOD == phase})
    return [(x, y - x) for x, y in zip(cuts, cuts[1:])]


def realign(seq, ops, q, sig, levels, k, m, rna, min_dur, max_dur, band, min_len, a, b, phase=0):
    """(new ops, n_free, n_moved, sum_abs_shift, cost_before, cost_after)"""
    assert RR.params_ok(band, min_len, min_dur, max_dur) and phase_ok(phase)
    inv_b, lb, W = 1.0 / b, len(ops), band
    lv = event_levels(seq, ops, levels, k, m, rna, min_dur, max_dur)
    B = boundaries(ops, q)
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
            if e == e1:
                cand = [P1]
            else:
                cand = [B[e] + j for j in range(-W, W + 1) if P0 + (e - e0) * min_len <= B[e] + j <= P1 - (e1 - e) * min_len]
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
    return [new[e + 1] - new[e] for e in range(lb)], sum(free), len(shifts), sum(shifts), before, after


# ---- phase 0 is realign_ref's rule: its worked case ------------------------------------------------------------------------------------
assert realign(**RR.WORKED) == RR.WORKED_RESULT and realign(phase=0, **RR.WORKED) == RR.WORKED_RESULT

# ---- the same six events at phase 3 -----------------------------------------------------------------------------------------------------
# seq ACGTAC, levels 10 / 20 / 30 / 40 pA, samples made with the boundaries 0, 5, 8, 11, 16, 21, 24, handed in as 0, 4, 8, 12, 16, 20, 24.
# Boundary 3 (at 12, true 11) is free under phase 0 and pinned under phase 3: 3 % 256 == 3. That leaves two runs. Boundaries 1 and 2
# between 0 and 12: A on [0, 5), C on [5, 8), G on [8, 12) -- boundary 1 moves from 4 to 5, boundary 2 stays at 8, and sample 11, a T (40)
# under G (30), is the one sample that keeps its 10 pA: |d| = 10000, 10^8. Boundaries 4 and 5 between 12 and 24: T on [12, 16), A on
# [16, 21), C on [21, 24) -- boundary 4 stays, boundary 5 moves from 20 to 21, cost 0. Four free boundaries, two moved by one sample each.
# Before, as under phase 0: samples 4, 11 and 20 lie under the wrong level, 3 * 10^8.
WORKED_PHASE = 3
WORKED_PHASE_RESULT = ([5, 3, 4, 4, 5, 3], 4, 2, 2, 3 * 10 ** 8, 10 ** 8)
assert realign(phase=WORKED_PHASE, **RR.WORKED) == WORKED_PHASE_RESULT
assert free_boundaries([1] * 6, 3) == [False, True, True, False, True, True, False]
assert pieces(6, 3) == [(0, 3), (3, 3)] and pieces(6, 0) == [(0, 6)] and pieces(600, 128) == [(0, 128), (128, 256), (384, 216)] and pieces(3, 3) == [(0, 3)]


def fit(seq, ops, q, sig, levels, k, m, rna, min_dur, max_dur, min_events):
    """(status, a, b, N) of fit_ref's pass 1 over the ops; N the counted samples (0 unless ok)"""
    ev = R.walk(seq, ops, q, len(sig), levels, k, m, rna, min_dur, max_dur)
    if ev is None:
        return R.OUT_OF_SIGNAL, None, None, 0
    su = R.sums(sig, ev, levels)
    st, a, b = R.solve(su, min_events)
    return st, a, b, (su[0] if st == R.OK else 0)


def rounds(seq, ops, q, sig, levels, k, m, rna, min_dur, max_dur, min_events, band, min_len, n_rounds, phases=ROUND_PHASES):
    """[(status, a, b, N, (ops_t, n_free, n_moved, sum_abs_shift, cost_before, cost_after))] for t = 1 .. n_rounds; round t runs at
    phases[(t - 1) % len(phases)]. ops_R is the last entry's [4][0]."""
    assert 1 <= n_rounds <= 8
    out, cur = [], list(ops)
    for t in range(1, n_rounds + 1):
        st, a, b, n = fit(seq, cur, q, sig, levels, k, m, rna, min_dur, max_dur, min_events)
        res = (list(cur), 0, 0, 0, 0, 0)
        if st == R.OK:
            res = realign(seq, cur, q, sig, levels, k, m, rna, min_dur, max_dur, band, min_len, a, b, phases[(t - 1) % len(phases)])
        out.append((st, a, b, n, res))
        cur = res[0]
    return out
