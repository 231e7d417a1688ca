"""Shared by the tests of `poregen realign` (pg_realign_*): reads that sit on the edges of the rule and of the kernel's shapes, and the
expected results from realign_ref (the fit of every read from fit_ref). Nothing here calls the product."""
import numpy as np

import fit_cases as FC
import fit_ref as R
import realign_ref as RR


class Params(FC.Params):
    def __init__(self, k, m=0, rna=False, min_dur=5, max_dur=70, min_events=20, band=4, min_len=3):
        super().__init__(k, m, rna, min_dur, max_dur, min_events)
        self.band, self.min_len = band, min_len

    def fit_key(self):
        return super().key()

    def key(self):
        return super().key() + (self.band, self.min_len)


def fit_of(r, levels, lid, p):
    """(status, a, b) of the read: fit_ref's, or what the case hands in instead (r.fit)."""
    if getattr(r, "fit", None) is not None:
        return r.fit
    key = ("fit", lid) + p.fit_key()
    if key not in r._cache:
        if r.skip:
            r._cache[key] = (R.SKIPPED + r.skip, None, None)
        else:
            ev = R.walk(r.seq, r.ops, r.q, len(r.sig), levels, p.k, p.m, p.rna, p.min_dur, p.max_dur)
            if ev is None:
                r._cache[key] = (R.OUT_OF_SIGNAL, None, None)
            else:
                r._cache[key] = R.solve(R.sums(r.sig_list(), ev, levels), p.min_events)
    return r._cache[key]


def expected(r, levels, lid, p):
    """(status, a, b, (new ops, n_free, n_moved, sum_abs_shift, cost_before, cost_after)); a read that is not fitted keeps its ops."""
    key = ("realign", lid) + p.key()
    if key not in r._cache:
        st, a, b = fit_of(r, levels, lid, p)
        if st != R.OK:
            r._cache[key] = (st, 0.0, 0.0, (list(r.ops), 0, 0, 0, 0, 0))
        else:
            r._cache[key] = (st, a, b, RR.realign(r.seq, r.ops, r.q, r.sig_list(), levels, p.k, p.m, p.rna, p.min_dur, p.max_dur, p.band, p.min_len, a, b))
    return r._cache[key]


def jitter_ops(rng, ops, jitter, floor):
    """The ops with every inner boundary moved by up to `jitter`, no op below `floor`; the sum stays."""
    B = np.concatenate([[0], np.cumsum(ops)]).astype(np.int64)
    H = B.copy()
    for e in range(1, len(ops)):
        lo, hi = max(B[e] - jitter, H[e - 1] + floor), min(B[e] + jitter, B[e + 1] - jitter - floor if e + 1 < len(ops) else B[-1] - floor)
        H[e] = int(rng.integers(lo, hi + 1)) if hi >= lo else B[e]
    return [int(x) for x in np.diff(H)]


def moved_read(rng, levels, p, true_ops, jitter=None, noise=6, name="", **kw):
    """A read whose samples follow the model over true_ops, handed in with boundaries jittered by up to `jitter` (default: the band)."""
    r = FC.make_read(rng, levels, p, true_ops, noise=noise, name=name, **kw)
    j = p.band if jitter is None else jitter
    r.true_ops = list(r.ops)
    if j and len(r.ops) > 1:
        r.ops = jitter_ops(rng, r.ops, j, p.min_dur)
    return r


def ops_for(rng, p, n, lo=None, hi=30):
    """n true durations that leave room for a jitter of the band on either side and still count"""
    lo = p.min_dur + 2 * p.band if lo is None else lo
    return rng.integers(lo, max(hi, lo + 8) + 1, n)


def edge_reads(levels, p, seed=3, big=True):
    """[Read]: the shapes at which the rule or the kernel takes another path (names say what each is for). big: also the reads of more
    than 300 ops (for bands up to 4: the reference is quadratic in the band)."""
    rng = np.random.default_rng(seed)
    k, W, out = p.k, p.band, []
    for lb in sorted({1, 2, k - 1, k, k + 1} - {0}):
        out.append(moved_read(rng, levels, p, ops_for(rng, p, lb), name=f"lb{lb}"))
    sizes = [63, 64, 65, 255, 256, 257] + ([511, 512, 513, 1023, 1024, 1025] if big else [])
    for ne in sizes:
        out.append(moved_read(rng, levels, p, ops_for(rng, p, ne, hi=20), q=int(rng.integers(0, 40)), tail=int(rng.integers(0, 9)), name=f"ops{ne}"))
    # durations at the limits and around the width of a window: the windows of neighbouring boundaries overlap below 2 W, and the shift
    # c' + n - min_len is clipped from 2 W + min_len on
    durs = sorted({p.min_dur, max(2 * W - 1, p.min_dur), max(2 * W, p.min_dur), 2 * W + 1, 2 * W + p.min_len, p.max_dur, p.max_dur + 1, max(p.min_dur - 1, 1)})
    for d in durs:
        ops = ops_for(rng, p, 40); ops[11:14] = d; ops[25] = d
        out.append(moved_read(rng, levels, p, ops, jitter=0 if d >= p.max_dur - 4 else min(W, 2), noise=20, q=3, name=f"dur{d}"))
    ops = rng.integers(p.min_dur, p.min_dur + 3, 90)                     # every event short: all windows overlap, admissibility binds
    out.append(moved_read(rng, levels, p, ops, jitter=0, noise=40, q=2, name="all_short"))
    # the first event at sample 0 and the last ending on the read's last sample, loud neighbours on either side in the buffer
    out.append(FC.Read("ACGTACGTAC"[:max(k, 4)], [40] * max(k, 4), 0, np.full(40 * max(k, 4), 32000), skip=0, name="loud_before"))
    out[-1].fit = (R.FEW_EVENTS, None, None)
    out.append(moved_read(rng, levels, p, ops_for(rng, p, 70), q=0, tail=0, noise=30, name="edge_to_edge"))
    out.append(FC.Read("ACGTACGTAC"[:max(k, 4)], [40] * max(k, 4), 0, np.full(40 * max(k, 4), -32000), skip=0, name="loud_behind"))
    out[-1].fit = (R.FEW_EVENTS, None, None)
    # events that are not refinable: an N, a k-mer without a level (slot 1 is missing in the tests' models), too short, too long -- in the
    # middle, at e = m, and on either side of boundary 256
    for where, name in ((40, "middle"), (p.m, "at_m"), (255, "before_256"), (256, "after_256")):
        n = 300
        seq = list("ACGT"[i] for i in rng.integers(0, 4, n))
        ops = ops_for(rng, p, n, hi=16)
        at = where + (k if p.rna else 0)
        seq[min(at, n - 1)] = "N"
        ops[min(where + 9, n - 1)] = max(p.min_dur - 1, 1); ops[min(where + 17, n - 1)] = p.max_dur + 1
        out.append(moved_read(rng, levels, p, ops, seq="".join(seq), jitter=min(W, 2), name=f"unrefinable_{name}"))
    # neighbouring events of one level (a homopolymer stretch) and a constant signal: ties everywhere; the fit is handed in, the
    # calibration of a constant signal being flat
    seq = "".join("ACGT"[i] for i in rng.integers(0, 4, 30)) + "A" * 30 + "".join("ACGT"[i] for i in rng.integers(0, 4, 30))
    out.append(moved_read(rng, levels, p, ops_for(rng, p, 90, hi=14), seq=seq, jitter=min(W, 2), noise=0, name="one_level_neighbours"))
    ops = ops_for(rng, p, 80, hi=12)
    r = FC.Read("".join("ACGT"[i] for i in rng.integers(0, 4, 80)), ops, 4, np.full(4 + int(sum(ops)) + 2, 500), name="constant_signal")
    r.fit = (R.OK, 100.0, 0.005)
    out.append(r)
    r = moved_read(rng, levels, p, ops_for(rng, p, 120, hi=14), name="outliers_clamp")
    B = RR.boundaries(r.ops, r.q)
    r.sig[B[30] + 1] = 32767; r.sig[B[60] - 1] = -32767; r.sig[B[61]] = 32767
    out.append(r)
    # every status that is not ok, among good reads: ops unchanged, zeros
    out.append(moved_read(rng, levels, p, ops_for(rng, p, 80), q=5, tail=-1, jitter=0, name="out_of_signal"))
    out.append(moved_read(rng, levels, p, ops_for(rng, p, 10), name="few_events"))
    out.append(moved_read(rng, levels, p, ops_for(rng, p, 60), seq="A" * 60, name="flat"))
    out.append(moved_read(rng, levels, p, ops_for(rng, p, 100), falling=True, name="negative_scale"))
    r = moved_read(rng, levels, p, ops_for(rng, p, 50), name="too_long"); r.fit = (R.TOO_LONG, None, None); out.append(r)
    r = moved_read(rng, levels, p, ops_for(rng, p, 50), name="skipped"); r.fit = (R.SKIPPED + 3, None, None); out.append(r)
    out.append(moved_read(rng, levels, p, ops_for(rng, p, 70), name="after_the_bad_ones"))
    return out


def planted_reads(levels, p, n, seed=21, n_events=60):
    """Reads with noise-free samples over true boundaries, handed in jittered by up to the band: only those are kept where THE REFERENCE
    puts every free boundary between two different levels back where it was."""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(4 * n):
        r = moved_read(rng, levels, p, ops_for(rng, p, n_events, hi=40), noise=0, q=int(rng.integers(0, 9)), tail=3, name=f"planted{i}")
        st, a, b, (new, *_rest) = expected(r, levels, "planted", p)
        if st != R.OK:
            continue
        lv = RR.event_levels(r.seq, r.ops, levels, p.k, p.m, p.rna, p.min_dur, p.max_dur)
        free = RR.free_boundaries(lv)
        T, N = RR.boundaries(r.true_ops, r.q), RR.boundaries(new, r.q)
        r.checked = [e for e in range(len(r.ops)) if free[e] and lv[e - 1] != lv[e]]
        if r.checked and all(T[e] == N[e] for e in r.checked) and r.ops != r.true_ops:
            out.append(r)
        if len(out) == n:
            break
    return out


def random_small_reads(levels, p, n, seed=31):
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        ne = int(rng.integers(p.k + 21, p.k + 40))
        out.append(moved_read(rng, levels, p, rng.integers(p.min_dur, 26, ne), jitter=min(p.band, 3), noise=int(rng.integers(0, 40)), q=int(rng.integers(0, 5)),
                              tail=int(rng.integers(0, 3)), name=f"small{i}"))
    return out
