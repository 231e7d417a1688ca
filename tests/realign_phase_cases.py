"""Shared by the tests of realign's phase and rounds: reads that sit on the edges of the pinned period under a phase, and the expected
results from realign_phase_ref (every read's fit from fit_ref, or handed in where a read is too short for one). Nothing here calls the
product."""
import types

import numpy as np

import fit_cases as FC
import fit_ref as R
import realign_cases as RC
import realign_phase_ref as PR

PHASES = (0, 1, 127, 128, 255)
HANDED_IN = (R.OK, 450.0, 0.006)          # a calibration as fit_cases.make_read draws them, for reads fit_ref does not fit


def params(band=2, min_len=2, k=2, m=0, rna=False):
    return RC.Params(k, m, rna, min_dur=4, max_dur=40, min_events=20, band=band, min_len=min_len)


def _read(rng, levels, p, n, name, long_at=()):
    ops = rng.integers(p.min_dur + 4, p.min_dur + 9, n)
    for x in long_at:                                                      # an event of more than max_dur samples is not refinable
        ops[x] = p.max_dur + 10
    r = RC.moved_read(rng, levels, p, ops, jitter=min(p.band, 2), noise=8, q=int(rng.integers(0, 6)), tail=int(rng.integers(0, 4)), name=name)
    if RC.fit_of(r, levels, "phase", p)[0] != R.OK:
        r.fit = HANDED_IN
    return r


def phase_reads(levels, p, phase, seed=41):
    """Reads of phase - 1, phase, phase + 1, phase + 255, phase + 256, phase + 257 ops and of 1 op, and reads of phase + 300 ops with an
    event that is not refinable on either side of boundary `phase` and of boundary `phase + 256`."""
    rng = np.random.default_rng(seed + phase)
    out = [_read(rng, levels, p, n, f"ops{n}") for n in sorted({1} | {n for n in (phase - 1, phase, phase + 1, phase + 255, phase + 256, phase + 257) if n > 0})]
    for x in (phase - 1, phase, phase + 255, phase + 256):
        if x >= 0:
            out.append(_read(rng, levels, p, phase + 300, f"long_event{x}", long_at=(x,)))
    return out


def piece_count_reads(levels, p, phase, counts=(63, 64, 65), seed=43):
    """Reads cut into exactly `counts` pieces under the phase: the loops of the per-read kernels past one wave's width."""
    rng = np.random.default_rng(seed)
    out = []
    for c in counts:
        lb = 100 + 256 * (c - 1) - ((256 - phase) if phase else 0)
        assert len(PR.pieces(lb, phase)) == c
        out.append(_read(rng, levels, p, lb, f"pieces{c}"))
    return out


def planted_256():
    """A noise-free read of 300 events over true boundaries; handed in with boundary 256 off by +3, every other boundary true."""
    p = RC.Params(2, 0, False, band=5, min_len=3)
    levels = [int(x) for x in np.random.default_rng(82).permutation(16) * 4500 + 60000]
    rng = np.random.default_rng(7)
    seq = "".join("ACGT"[(i * 7 + i // 3) % 4] for i in range(300))        # neighbouring 2-mers differ
    r = FC.make_read(rng, levels, p, rng.integers(12, 20, 300), q=4, tail=3, seq=seq, noise=0, name="planted256")
    r.true_ops = list(r.ops)
    lv = PR.event_levels(seq, r.ops, levels, 2, 0, False, p.min_dur, p.max_dur)
    assert all(lv[e] is not None and lv[e] != lv[e + 1] for e in range(250, 262))
    r.ops[255] += 3; r.ops[256] -= 3
    return levels, p, r


def expected(r, levels, lid, p, phase):
    """(status, a, b, (new ops, n_free, n_moved, sum_abs_shift, cost_before, cost_after)); a read that is not fitted keeps its ops."""
    key = ("realign_phase", lid, phase) + p.key()
    if key not in r._cache:
        st, a, b = RC.fit_of(r, levels, lid, p)
        if st != R.OK:
            r._cache[key] = (st, 0.0, 0.0, (list(r.ops), 0, 0, 0, 0, 0))
        else:
            r._cache[key] = (st, a, b, PR.realign(r.seq, r.ops, r.q, r.sig_list(), levels, p.k, p.m, p.rna, p.min_dur, p.max_dur, p.band, p.min_len, a, b, phase))
    return r._cache[key]


def fit_namespace(want):
    return types.SimpleNamespace(status=np.array([w[0] for w in want], np.uint32), a=np.array([w[1] or 0.0 for w in want]), b=np.array([w[2] or 0.0 for w in want]))


def rounds_of(r, levels, p, n_rounds, phases=PR.ROUND_PHASES):
    return PR.rounds(r.seq, r.ops, r.q, r.sig_list(), levels, p.k, p.m, p.rna, p.min_dur, p.max_dur, p.min_events, p.band, p.min_len, n_rounds, phases)
