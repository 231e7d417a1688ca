"""Shared by the tests of `poregen fit` (pg_fit_*): synthetic models, reads that sit on the edges of the rule and of the kernels' shapes,
batches of them laid out as a pg_batch, files of them written with the writers the --reform tests use, and the expected results from
fit_ref. Nothing here calls the product."""
import numpy as np

import fit_ref as R


class Params:
    def __init__(self, k, m=0, rna=False, min_dur=5, max_dur=70, min_events=20):
        self.k, self.m, self.rna, self.min_dur, self.max_dur, self.min_events = k, m, rna, min_dur, max_dur, min_events

    def key(self):
        return (self.k, self.m, self.rna, self.min_dur, self.max_dur, self.min_events)


def model_levels(k, seed=1, missing=()):
    """Levels in 1e-3 pA, 60 to 130 pA, None for the slots in `missing`."""
    rng = np.random.default_rng(seed)
    lv = [int(x) for x in rng.integers(60000, 130000, 4 ** k)]
    for s in missing:
        lv[s] = None
    return lv


def levels_array(levels):
    return np.array([0 if l is None else l for l in levels], np.uint32)


class Read:
    def __init__(self, seq, ops, q, sig, skip=0, name=""):
        self.seq, self.ops, self.q, self.skip, self.name = seq, [int(x) for x in ops], int(q), int(skip), name
        self.sig = np.asarray(sig, np.int16)
        self._sig_list = None
        self._cache = {}

    def sig_list(self):
        if self._sig_list is None:
            self._sig_list = [int(x) for x in self.sig]
        return self._sig_list

    def expected(self, levels, lid, p):
        """(status, sums7, a, b, events): the reference's word on this read; cached per (model, parameters)."""
        key = (lid,) + p.key()
        if key not in self._cache:
            if self.skip:
                out = (R.SKIPPED + self.skip, (0,) * 7, None, None, [])
            else:
                ev = R.walk(self.seq, self.ops, self.q, len(self.sig), levels, p.k, p.m, p.rna, p.min_dur, p.max_dur)
                if ev is None:
                    out = (R.OUT_OF_SIGNAL, (0,) * 7, None, None, [])
                else:
                    su = R.sums(self.sig_list(), ev, levels)
                    st, a, b = R.solve(su, p.min_events)
                    out = (st, su, a, b, ev)
            self._cache[key] = out
        return self._cache[key]


def make_read(rng, levels, p, ops, q=0, tail=0, seq=None, falling=False, noise=12, name=""):
    """A read whose samples follow the model: raw = a + b * level + noise over every event that carries a k-mer with a level, noise
    elsewhere. tail: samples behind the last op (-1: the ops run one sample past the signal)."""
    ops = [int(x) for x in ops]
    lb = len(ops)
    if seq is None:
        seq = "".join("ACGT"[i] for i in rng.integers(0, 4, lb))
    total = q + sum(ops) + tail
    a, b = float(rng.uniform(300, 600)), float(rng.uniform(0.004, 0.008)) * (-1 if falling else 1)
    sig = rng.integers(200, 900, max(total, 0)).astype(np.int64)
    for kmer, lo, hi in R.pairing(seq, ops, q, p.k, p.m, p.rna):
        if any(c not in "ACGT" for c in kmer) or levels[R.slot_of(kmer)] is None:
            continue
        hi = min(hi, len(sig))
        if hi > lo:
            sig[lo:hi] = np.rint(a + b * levels[R.slot_of(kmer)]).astype(np.int64) + rng.integers(-noise, noise + 1, hi - lo)
    return Read(seq, ops, q, np.clip(sig, -32768, 32767).astype(np.int16), name=name)


def rand_ops(rng, n, lo=5, hi=30):
    return rng.integers(lo, hi + 1, n)


def edge_reads(levels, p, seed=3, min_events=20):
    """[Read]: the shapes at which the rule takes another path, for the model and parameters given (names say what each is for)."""
    rng = np.random.default_rng(seed)
    k, out = p.k, []
    for lb in (k - 1, k, k + 1):
        if lb >= 1:
            out.append(make_read(rng, levels, p, rand_ops(rng, lb), name=f"lb{lb}"))
    for ne in (63, 64, 65, 128, 129, 255, 256, 257, 1023, 1024, 1025):
        out.append(make_read(rng, levels, p, rand_ops(rng, ne), q=int(rng.integers(0, 40)), tail=int(rng.integers(0, 9)), name=f"events{ne}"))
    ops = rand_ops(rng, 90); ops[10:18] = [max(p.min_dur - 1, 0), p.min_dur, p.min_dur + 1, p.max_dur - 1, p.max_dur, p.max_dur + 1, 3 * p.max_dur, max(p.min_dur - 2, 0)]
    out.append(make_read(rng, levels, p, ops, name="duration_limits"))
    out.append(make_read(rng, levels, p, rand_ops(rng, 80), q=137, name="q_positive"))
    out.append(make_read(rng, levels, p, rand_ops(rng, 80), q=5, tail=0, name="ends_at_last_sample"))
    out.append(make_read(rng, levels, p, rand_ops(rng, 80), q=5, tail=-1, name="one_past_last_sample"))
    r = make_read(rng, levels, p, rand_ops(rng, 80), name="negative_q"); r.q = -1; out.append(r)
    seq = "".join("ACGT"[i] for i in rng.integers(0, 4, 100)); seq = seq[:40] + "N" + seq[41:70] + "NN" + seq[72:]
    out.append(make_read(rng, levels, p, rand_ops(rng, 100), seq=seq, name="n_inside_kmers"))
    out.append(make_read(rng, levels, p, rand_ops(rng, 60), seq="A" * 60, name="flat_one_kmer"))
    out.append(make_read(rng, levels, p, rand_ops(rng, 120), falling=True, name="falling_level"))
    # E = min_events - 1 and E = min_events: every op inside the limits, no N; a missing k-mer may still drop events, so the count is
    # taken from the reference and the reads are trimmed to it
    for want in (min_events - 1, min_events):
        lb = want + k + p.m + 4
        while True:
            seq = "".join("ACGT"[i] for i in rng.integers(0, 4, lb))
            r = make_read(rng, levels, p, rand_ops(rng, lb, max(p.min_dur, 1), min(p.max_dur, 30)), seq=seq, name=f"counted{want}")
            e = len(R.walk(r.seq, r.ops, r.q, len(r.sig), levels, p.k, p.m, p.rna, p.min_dur, p.max_dur))
            if e == want:
                break
            lb += 1 if e < want else -1
        out.append(r)
    r = make_read(rng, levels, p, rand_ops(rng, 200), name="one_outlier_clamps")
    ev = R.walk(r.seq, r.ops, r.q, len(r.sig), levels, p.k, p.m, p.rna, p.min_dur, p.max_dur)
    r.sig[ev[len(ev) // 2][0] + 1] = 32767
    out.append(r)
    out.append(Read("ACGTACGTAC", [], 0, rng.integers(200, 900, 50), skip=3, name="refused_by_reform"))   # the expander leaves such a read without ops
    out.append(make_read(rng, levels, p, rand_ops(rng, 70), name="after_the_refused_one"))
    return out


ROUND_TOTALS = (63, 64, 65, 255, 256, 257, 511, 512, 513)


def round_edge_read(levels, p, seed=15):
    """One read whose steps of 64 ops hold exactly ROUND_TOTALS counted samples, step after step: one below, at and one above a quarter,
    one, two rounds of the 256 samples the lanes of a wave take per round. Ops of 2 samples lie below min_dur 5 and do not count; the
    model must have every level and p.m must be 0."""
    rng = np.random.default_rng(seed)
    fill = lambda counted: list(counted) + [2] * (64 - len(counted))
    steps = [fill([7] * 9), fill([8] * 8), fill([5] * 13), fill([5] * 51), fill([8] * 32), fill([5] * 50 + [7]), [8] * 63 + [7], [8] * 64, [8] * 63 + [9]]
    ops = []
    for s in steps:
        s = list(s)
        rng.shuffle(s)
        ops += s
    return make_read(rng, levels, p, ops + [6] * (p.k + 10), q=3, tail=2, name="round_edges")


def step_totals(r, levels, p):
    """The counted samples of every step of 64 ops of the read, by the reference."""
    out = [0] * ((len(r.ops) + 63) // 64)
    starts = [r.q]
    for n in r.ops:
        starts.append(starts[-1] + n)
    counted = {(lo, n) for lo, n, _ in R.walk(r.seq, r.ops, r.q, len(r.sig), levels, p.k, p.m, p.rna, p.min_dur, p.max_dur)}
    for e, n in enumerate(r.ops):
        if n and (starts[e], n) in counted:
            out[e // 64] += n
    return out


def long_event_reads(levels, p, seed=4):
    """Events of 1, 63, 64, 65 and 129 samples between ordinary ones (for min_dur 1 and a max_dur of 129 or more)."""
    rng = np.random.default_rng(seed)
    out = []
    for special in (1, 63, 64, 65, 129):
        ops = rand_ops(rng, 70, 1, 20); ops[5] = special; ops[33] = special; ops[69] = special
        out.append(make_read(rng, levels, p, ops, name=f"event_of_{special}"))
    return out


def long_read(levels, p, n_samples=1 << 18, seed=5):
    """One read of exactly n_samples samples."""
    rng = np.random.default_rng(seed)
    ops = list(rand_ops(rng, n_samples // 12, 5, 16))
    while sum(ops) > n_samples - 10:
        ops.pop()
    return make_read(rng, levels, p, ops, q=7, tail=n_samples - 7 - sum(ops), name="long")


def many_small_reads(levels, p, n, seed=6):
    rng = np.random.default_rng(seed)
    return [make_read(rng, levels, p, rand_ops(rng, int(rng.integers(p.k + 20, p.k + 30)), 5, 8), name=f"s{i}") for i in range(n)]


def file_reads(levels, p, n, seed=14, n_at=None):
    """Reads a basecaller could have written: dwells that are multiples of the stride 5, query_start 0, the ops ending on the last sample.
    n_at: that read carries an N which was a T when its signal was made (for --n_to_t)."""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        lb = int(rng.integers(60, 200))
        r = make_read(rng, levels, p, 5 * rng.integers(1, 9, lb), name=f"r{i}")
        if i == n_at:
            at = r.seq.index("T", 20)
            r.seq = r.seq[:at] + "N" + r.seq[at + 1:]
        out.append(r)
    return out


def to_batch(reads):
    """engine.Batch (host arrays) of the reads, every op a match."""
    from poregen_amd.engine import Batch
    n = len(reads)
    cat = lambda parts, dt: np.concatenate([np.asarray(x, dt) for x in parts]) if parts else np.zeros(0, dt)
    off = lambda lens: np.cumsum([0] + list(lens)).astype(np.uint64)
    op_n = cat([r.ops for r in reads], np.uint32)
    return Batch(n_reads=n, sig=cat([r.sig for r in reads], np.int16), sig_off=off(len(r.sig) for r in reads),
                 digitisation=np.full(n, 8192.0), offset=3.0 + np.arange(n), range=1400.0 + 0.5 * np.arange(n),
                 query_start=np.array([r.q for r in reads], np.int32), target_start=np.zeros(n, np.int32), target_end=np.array([len(r.seq) for r in reads], np.int32),
                 seq=np.frombuffer("".join(r.seq for r in reads).encode(), np.uint8).copy(), seq_off=off(len(r.seq) for r in reads),
                 op_n=op_n, op_t=np.zeros(op_n.size, np.uint8), op_off=off(len(r.ops) for r in reads), all_matches=True)


def expected(reads, levels, lid, p):
    """Per read (status, sums, a, b) and, over the fitted reads, the slots' sums and the clamped samples."""
    per_read, slots, clamped = [], {}, 0
    for r in reads:
        st, su, a, b, ev = r.expected(levels, lid, p)
        per_read.append((st, su, a, b))
        if st == R.OK:
            key = ("resid", lid) + p.key()
            if key not in r._cache:
                own = {}
                r._cache[key] = (own, R.residuals(r.sig_list(), ev, levels, a, b, own))
            own, c = r._cache[key]
            clamped += c
            for s, v in own.items():
                acc = slots.setdefault(s, [0, 0, 0, 0])
                for j in range(4):
                    acc[j] += v[j]
    return per_read, slots, clamped


def assert_well_conditioned(reads, levels, lid, p):
    """The fitted reads keep 1 - R^2 >= 1e-3: the subtraction in RSS then loses nothing that matters."""
    from fractions import Fraction
    for r in reads:
        st, su, _, _, _ = r.expected(levels, lid, p)
        if st == R.OK:
            assert R.one_minus_r2(su) >= Fraction(1, 1000), r.name
