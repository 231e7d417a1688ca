"""Shared by the tests of fit and realign on gapped batches (PG_BATCH_GAPPED): reads on the signal-to-reference alignment -- ops with I
and D among them over a reference slice -- placed on the edges of the rule and of the kernels' shapes, batches of them laid out as a
pg_batch, and the expected results from fitgap_ref and realigngap_ref. Nothing here calls the product."""
import numpy as np

import fit_cases as FC
import fit_ref as R
import fitgap_ref as G
import realign_cases as RC
import realigngap_ref as RG

M, I, D = G.MATCH, G.INS, G.DEL
Params = RC.Params


class GRead:
    def __init__(self, seq, ops, types, q, sig, skip=0, name=""):
        self.seq, self.ops, self.types, self.q, self.skip, self.name = seq, [int(x) for x in ops], [int(t) for t in types], int(q), int(skip), name
        self.sig = np.asarray(sig, np.int16)
        self._sig_list, self._cache, self.fit = None, {}, None

    def sig_list(self):
        if self._sig_list is None:
            self._sig_list = [int(x) for x in self.sig]
        return self._sig_list

    def fit_expected(self, levels, lid, p):
        """(status, sums7, a, b, events) by fitgap_ref"""
        key = ("fit", lid) + p.fit_key()
        if key not in self._cache:
            if self.skip:
                self._cache[key] = (R.SKIPPED + self.skip, (0,) * 7, None, None, [])
            else:
                self._cache[key] = G.fit(self.seq, self.ops, self.types, self.q, self.sig_list(), levels, p.k, p.m, p.rna, p.min_dur, p.max_dur, p.min_events)
        return self._cache[key]

    def realign_expected(self, levels, lid, p, phase=0):
        """(status, a, b, (new ops, n_free, n_moved, sum_abs_shift, cost_before, cost_after)); a read that is not fitted keeps its ops"""
        key = ("realign", lid, phase) + p.key()
        if key not in self._cache:
            st, _, a, b, _ = self.fit_expected(levels, lid, p) if self.fit is None else (self.fit[0], None, self.fit[1], self.fit[2], None)
            if st != R.OK:
                self._cache[key] = (st, 0.0, 0.0, (list(self.ops), 0, 0, 0, 0, 0))
            else:
                self._cache[key] = (st, a, b, RG.realign(self.seq, self.ops, self.types, self.q, self.sig_list(), levels, p.k, p.m, p.rna, p.min_dur, p.max_dur, p.band,
                                                         p.min_len, a, b, phase))
        return self._cache[key]


def rand_seq(rng, n):
    return "".join("ACGT"[i] for i in rng.integers(0, 4, n))


def types_with(n, gaps):
    """n ops, all matches but gaps: {op: I or D}"""
    t = [M] * n
    for at, what in gaps.items():
        if 0 <= at < n:
            t[at] = what
    return t


def rand_types(rng, n, rate=0.05):
    x = rng.random(n)
    return [I if v < rate / 2 else D if v < rate else M for v in x]


def make_read(rng, levels, p, types, q=0, tail=0, seq=None, seq_delta=0, noise=6, jitter=None, falling=False, d_cols=None, i_samples=None, dur_hi=22, name=""):
    """A read whose samples follow the model over true boundaries -- raw = a + b * level + noise over every event the gapped rule pairs with
    a k-mer that has a level, noise elsewhere -- handed in with the boundaries between two matches moved by up to `jitter` (default: the
    band; the ops keep their sum, an I and a D keep their op_n). A match lasts min_dur + 2 band samples or more, an I 3 to 40 samples
    (i_samples: that many), a D 1 to 3 columns (d_cols: that many). seq_delta: the slice is that much longer (or shorter) than the columns."""
    types = [int(t) for t in types]
    lb = len(types)
    lo = p.min_dur + 2 * p.band
    ops = [int(rng.integers(lo, max(dur_hi, lo + 8) + 1)) if t == M else
           (int(rng.integers(3, 41)) if i_samples is None else i_samples) if t == I else (int(rng.integers(1, 4)) if d_cols is None else d_cols) for t in types]
    starts, cols = G.layout(ops, types, q)
    if seq is None:
        seq = rand_seq(rng, max(cols[-1] + seq_delta, 0))
    total = starts[-1] + tail
    a, b = float(rng.uniform(300, 600)), float(rng.uniform(0.004, 0.008)) * (-1 if falling else 1)
    sig = rng.integers(200, 900, max(total, 0)).astype(np.int64)
    if len(seq) == cols[-1]:
        for _, kmer, s0, s1 in G.pairing(seq, ops, types, q, p.k, p.m, p.rna):
            if any(c not in "ACGT" for c in kmer) or levels[R.slot_of(kmer)] is None:
                continue
            s1 = min(s1, len(sig))
            if s1 > s0:
                sig[s0:s1] = np.rint(a + b * levels[R.slot_of(kmer)]).astype(np.int64) + rng.integers(-noise, noise + 1, s1 - s0)
    j = p.band if jitter is None else jitter
    true_ops = list(ops)
    if j and lb > 1:
        H = list(starts)
        for e in range(1, lb):
            if types[e - 1] == M and types[e] == M:
                lo_, hi_ = max(starts[e] - j, H[e - 1] + p.min_dur), min(starts[e] + j, starts[e + 1] - j - p.min_dur)
                H[e] = int(rng.integers(lo_, hi_ + 1)) if hi_ >= lo_ else starts[e]
        ops = [ops[e] if types[e] == D else H[e + 1] - H[e] for e in range(lb)]
    r = GRead(seq, ops, types, q, np.clip(sig, -32768, 32767).astype(np.int16), name=name)
    r.true_ops = true_ops
    return r


def to_batch(reads, gapped=True):
    """engine.Batch (host arrays) of the reads"""
    from poregen_amd.engine import Batch
    n = len(reads)
    cat = lambda parts, dt: np.concatenate([np.asarray(x, dt) for x in parts]) if parts else np.zeros(0, dt)
    off = lambda lens: np.cumsum([0] + list(lens)).astype(np.uint64)
    return Batch(n_reads=n, sig=cat([r.sig for r in reads], np.int16), sig_off=off(len(r.sig) for r in reads),
                 digitisation=np.full(n, 8192.0), offset=3.0 + np.arange(n), range=1400.0 + 0.5 * np.arange(n),
                 query_start=np.array([r.q for r in reads], np.int32), target_start=np.zeros(n, np.int32), target_end=np.array([len(r.seq) for r in reads], np.int32),
                 seq=np.frombuffer("".join(r.seq for r in reads).encode(), np.uint8).copy(), seq_off=off(len(r.seq) for r in reads),
                 op_n=cat([r.ops for r in reads], np.uint32), op_t=cat([r.types for r in reads], np.uint8), op_off=off(len(r.ops) for r in reads),
                 gapped=gapped, all_matches=not gapped)


def fit_expected(reads, levels, lid, p):
    """Per read (status, sums, a, b) and, over the fitted reads, the slots' sums and the clamped samples."""
    per_read, slots, clamped = [], {}, 0
    for r in reads:
        st, su, a, b, ev = r.fit_expected(levels, lid, p)
        per_read.append((st, su, a, b))
        if st == R.OK:
            key = ("resid", lid) + p.fit_key()
            if key not in r._cache:
                own = {}
                r._cache[key] = (own, R.residuals(r.sig_list(), ev, levels, a, b, own))
            own, c = r._cache[key]
            clamped += c
            for s, v in own.items():
                acc = slots.setdefault(s, [0, 0, 0, 0])
                for x in range(4):
                    acc[x] += v[x]
    return per_read, slots, clamped


# ---- the shapes ------------------------------------------------------------------------------------------------------------------------------
STEP_EDGES = (62, 63, 64, 65)
PIECE_EDGES = (254, 255, 256, 257)
GROUP_EDGES = (1023, 1024, 1025)


def edge_gap_reads(levels, p, seed=5, edges=STEP_EDGES + PIECE_EDGES + GROUP_EDGES):
    """One read per (edge op, I or D) with the gap AT that op, and one whose gap lies k ops in front of the edge, so that the clean windows
    of the events around the edge straddle it while the gap's own window ends on it."""
    rng = np.random.default_rng(seed)
    out = []
    for at in edges:
        n = at + 40
        for what, nm in ((I, "I"), (D, "D")):
            out.append(make_read(rng, levels, p, types_with(n, {at: what}), q=int(rng.integers(0, 9)), tail=int(rng.integers(0, 4)), name=f"{nm}_at_{at}"))
        out.append(make_read(rng, levels, p, types_with(n, {at - p.k: D, at + p.k + 1: I}), q=2, name=f"window_straddles_{at}"))
    return out


def piece_shape_reads(levels, p, seed=6):
    """A D as the first and as the last op of a piece and of the read (its columns are carried into the next piece); a piece of only I and
    D; gaps k - 1 and k ops apart; an I of 0 samples; a D of 1 column beside one of 1000."""
    rng = np.random.default_rng(seed)
    out = [make_read(rng, levels, p, types_with(600, {0: D, 255: D, 256: D, 511: D, 512: I, 599: D}), d_cols=3, name="D_first_and_last_of_pieces"),
           make_read(rng, levels, p, [M] * 256 + [I, D] * 128 + [M] * 100, name="piece_of_only_I_and_D"),
           make_read(rng, levels, p, types_with(120, {30: I, 30 + p.k: D, 70: D, 70 + p.k + 1: I}), name="gaps_k_minus_1_and_k_apart"),
           make_read(rng, levels, p, types_with(90, {20: I, 50: I}), i_samples=0, name="I_of_0_samples"),
           make_read(rng, levels, p, types_with(90, {20: D}), d_cols=1, name="D_of_1"),
           make_read(rng, levels, p, types_with(90, {20: D, 60: D}), d_cols=1000, name="D_of_1000")]
    return out


def status_reads(levels, p, seed=7):
    """Every status among good neighbours."""
    rng = np.random.default_rng(seed)
    g = lambda n: types_with(n, {n // 3: I, 2 * n // 3: D})
    out = [make_read(rng, levels, p, g(80), name="good0"),
           make_read(rng, levels, p, g(80), q=5, tail=-1, jitter=0, name="out_of_signal"),
           make_read(rng, levels, p, g(80), seq_delta=-1, name="ref_length_short"),
           make_read(rng, levels, p, g(80), seq_delta=1, name="ref_length_long"),
           make_read(rng, levels, p, g(80), seq="", name="ref_length_empty"),
           make_read(rng, levels, p, g(80), q=5, tail=-1, seq_delta=3, jitter=0, name="out_of_signal_before_ref_length"),
           make_read(rng, levels, p, g(12), name="few_events"),
           make_read(rng, levels, p, g(60), seq="A" * 60, d_cols=2, name="flat"),          # 58 matches and a D of 2: 60 columns
           make_read(rng, levels, p, g(100), falling=True, name="negative_scale"),
           GRead("ACGT", [], [], 0, rng.integers(200, 900, 30), skip=3, name="skipped"),
           make_read(rng, levels, p, g(80), name="good1")]
    return out


def many_piece_reads(levels, p, n_pieces, seed=8):
    """A read of exactly n_pieces pieces with one gap in it (the per-read kernels take 64 pieces a step)."""
    rng = np.random.default_rng(seed + n_pieces)
    n = 256 * n_pieces - 17
    return make_read(rng, levels, p, types_with(n, {n // 2: D if n_pieces % 2 else I}), dur_hi=p.min_dur + 2 * p.band, name=f"pieces{n_pieces}")


def random_small_reads(levels, p, n, seed=9, rate=0.12):
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        ne = int(rng.integers(p.k + 21, p.k + 40))
        out.append(make_read(rng, levels, p, rand_types(rng, ne, rate), jitter=min(p.band, 3), noise=int(rng.integers(0, 40)), q=int(rng.integers(0, 5)),
                             tail=int(rng.integers(0, 3)), name=f"small{i}"))
    return out


def planted_reads(levels, p, n, seed=21, n_ops=70):
    """Gapped reads with noise-free samples over true boundaries, handed in jittered by up to the band: only those are kept where THE
    REFERENCE puts every free boundary between two different levels back where it was."""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(6 * n):
        r = make_read(rng, levels, p, rand_types(rng, n_ops, 0.06), noise=0, q=int(rng.integers(0, 9)), tail=3, dur_hi=40, name=f"planted{i}")
        st, a, b, (new, *_rest) = r.realign_expected(levels, "planted", p)
        if st != R.OK or not any(r.types):
            continue
        lv = RG.event_levels(r.seq, r.ops, r.types, levels, p.k, p.m, p.rna, p.min_dur, p.max_dur)
        free = RG.free_boundaries(lv)
        T, N = G.layout(r.true_ops, r.types, r.q)[0], G.layout(new, r.types, r.q)[0]
        r.checked = [e for e in range(len(r.ops)) if free[e] and lv[e - 1] != lv[e]]
        if r.checked and all(T[e] == N[e] for e in r.checked) and r.ops != r.true_ops:
            out.append(r)
        if len(out) == n:
            break
    return out
