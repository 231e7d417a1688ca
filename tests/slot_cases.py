"""K-mer lists at the slot counts where the collector's ranking switches path or digit width, and what the oracle makes of them.

pg_create picks the ranking from n_slots alone (key_bits = the smallest b with 2^b >= n_slots): up to 1024 slots the slot itself is the
digit, up to 2^20 two digits (hi = (key_bits + 1) / 2, lo = key_bits - hi), beyond that -- or forced by PGMOVE_LSD_SORT=1 -- an LSD
radix sort of ceil(key_bits / 10) balanced passes. One shared batch; per size a list that is a seeded permutation of generate_kmers(k),
with the batch's most frequent k-mers swapped into the slots at the digit borders, and two oracle runs over it (sample_limit 2 and
2^31 - 1). Everything here runs on the CPU; nothing of the product is used but generate_kmers and synth."""
import collections
import functools

import numpy as np

from helpers import oracle_for
from poregen_amd import synth
from poregen_amd.engine import generate_kmers

LIMIT = 2
NO_LIMIT = 2 ** 31 - 1
DIRECT_MAX_SLOTS = 1024
PART_MAX_KEY_BITS = 20
RANK_MAX_BITS = 10

# n_slots -> (k, key_bits, (hi, lo) or None, path): the table of the sizes, as written down before any code ran
SIZES = {
    1000: (5, 10, None, "direct"),
    1024: (5, 10, None, "direct"),
    1025: (6, 11, (6, 5), "partitioned"),
    2048: (6, 11, (6, 5), "partitioned"),
    2049: (6, 12, (6, 6), "partitioned"),
    4097: (7, 13, (7, 6), "partitioned"),
    8192: (7, 13, (7, 6), "partitioned"),
    16385: (8, 15, (8, 7), "partitioned"),
    65537: (9, 17, (9, 8), "partitioned"),
    262145: (10, 19, (10, 9), "partitioned"),
    524289: (10, 20, (10, 10), "partitioned"),
    1048576: (10, 20, (10, 10), "partitioned"),
    1048577: (11, 21, None, "lsd"),
}
FORCED_LSD = (1025, 4097, 16385)        # PGMOVE_LSD_SORT=1: two passes, the last one narrower
UNFUSED_AND_BASE = (1025, 262145, 1048576)


def key_bits_of(n_slots):
    b = 1
    while (1 << b) < n_slots:
        b += 1
    return b


def path_of(n_slots, forced_lsd=False):
    if n_slots <= DIRECT_MAX_SLOTS:
        return "direct"
    return "partitioned" if key_bits_of(n_slots) <= PART_MAX_KEY_BITS and not forced_lsd else "lsd"


def part_digits(n_slots):
    kb = key_bits_of(n_slots)
    hi = (kb + 1) // 2
    return hi, kb - hi


def lsd_widths(n_slots):
    """bits of every pass of the LSD sort, first pass first"""
    kb = key_bits_of(n_slots)
    passes = (kb + RANK_MAX_BITS - 1) // RANK_MAX_BITS
    per = (kb + passes - 1) // passes
    return [min(per, kb - p * per) for p in range(passes)]


def smallest_k(n_slots):
    k = 1
    while 4 ** k < n_slots:
        k += 1
    return k


def named_slots(n_slots):
    """the slots that get the batch's most frequent k-mers: the list's ends and both sides of the digit borders"""
    path = path_of(n_slots)
    if path == "direct":
        named = [0, n_slots - 1, 511, 512]
    elif path == "partitioned":
        hi, lo = part_digits(n_slots)
        r = (n_slots - 1) >> lo
        named = [0, n_slots - 1, (1 << lo) - 1, 1 << lo, (r << lo) - 1, r << lo]
        if hi == 10:  # a high digit that only the second half of k_part_scatter's prefix registers holds
            named.append(min((768 << lo) + 5, n_slots - 1))
        if n_slots in FORCED_LSD:  # the border between the forced sort's two passes
            w = lsd_widths(n_slots)[0]
            named += [(1 << w) - 1, 1 << w]
    else:
        w = lsd_widths(n_slots)
        named = [0, n_slots - 1, (1 << w[0]) - 1, 1 << w[0], (1 << (w[0] + w[1])) - 1, 1 << (w[0] + w[1])]
    out = []
    for s in named:
        assert 0 <= s < n_slots, (n_slots, s)
        if s not in out:
            out.append(s)
    return out


@functools.lru_cache(maxsize=None)
def batch():
    """about 38 000 ops: ten tiles of 4096 op indices, three workgroups of pass A, the last one partial"""
    return synth.make_batch(120, kind="dna_r10", seed=20261019, homopolymer_frac=0.2)


@functools.lru_cache(maxsize=None)
def _read_seqs():
    b = batch()
    return [synth.seq_string(b, r) for r in range(b.n_reads)]


@functools.lru_cache(maxsize=None)
def _full(k):
    """generate_kmers(k) as an array of byte strings, for numpy indexing"""
    return np.array(generate_kmers(k), dtype=f"S{k}")


def code_of(kmer):
    """index of a k-mer in generate_kmers(len(kmer))"""
    c = 0
    for ch in kmer:
        c = c * 4 + "ACGT".index(ch)
    return c


@functools.lru_cache(maxsize=None)
def _read_codes(k):
    """per read, code_of of every k-mer in its sequence"""
    return [np.array([code_of(s[i:i + k]) for i in range(len(s) - k + 1)], np.int64) for s in _read_seqs()]


@functools.lru_cache(maxsize=None)
def _frequent(k):
    """the batch's k-mers, most frequent first (ties: alphabetical), counted from the reads' sequences"""
    cnt = collections.Counter()
    for s in _read_seqs():
        for i in range(len(s) - k + 1):
            cnt[s[i:i + k]] += 1
    return [km for km, _ in sorted(cnt.items(), key=lambda t: (-t[1], t[0]))]


def list_codes(k, n_slots, seed):
    """the list as indices into generate_kmers(k): a seeded permutation's first n_slots, then the frequent k-mers moved to the named slots"""
    codes = np.random.default_rng(seed).permutation(4 ** k)[:n_slots].astype(np.int64)
    named = named_slots(n_slots)
    for slot, km in zip(named, _frequent(k)):
        c = code_of(km)
        at = np.flatnonzero(codes == c)
        if at.size:       # already in the list: the two change places
            codes[int(at[0])] = codes[slot]
        codes[slot] = c   # else: the named slot's k-mer leaves the list
    return codes


def kmer_list(k, n_slots, seed):
    return _full(k)[list_codes(k, n_slots, seed)].astype(f"U{k}").tolist()


class Expected:
    """One oracle run, flattened k-mer-major as the product returns it. counts: per slot, the events the oracle wrote into the slot
    (min(accepted events, sample_limit)); ev_len, ev_read: the window length and the read of every one of them."""

    def __init__(self, counts, ev_len, ev_read, samples):
        self.counts = counts
        self.ev_off = np.concatenate([[0], np.cumsum(counts, dtype=np.uint64)]).astype(np.uint64)
        self.ev_len, self.ev_read, self.samples = ev_len, ev_read, samples
        self.samp_off = np.concatenate([[0], np.cumsum(ev_len, dtype=np.uint64)]).astype(np.uint64)
        assert int(self.ev_off[-1]) == ev_len.size == ev_read.size and int(self.samp_off[-1]) == samples.size

    def first_events(self, room):
        """the run cut to each slot's first room[slot] events: what a collector keeps that starts with sample_limit - room events in the slot"""
        room = np.asarray(room, np.uint64)
        keep_n = np.minimum(self.counts, room)
        slot_of_ev = np.repeat(np.arange(self.counts.size), self.counts.astype(np.int64))
        rank = np.arange(self.ev_len.size, dtype=np.uint64) - self.ev_off[:-1][slot_of_ev]
        keep = rank < room[slot_of_ev]
        return Expected(keep_n, self.ev_len[keep], self.ev_read[keep], self.samples[np.repeat(keep, self.ev_len.astype(np.int64))])


def run_oracle(kmers, codes, k, sample_limit):
    """The oracle over the shared batch, read by read. It does not say which read an event came from: the slots a read can reach are
    those of the k-mers in its sequence, and their counts before and after the read tell (checked against the final counts)."""
    b = batch()
    o = oracle_for(kmers, kmer_size=k, scaling=1, sample_limit=sample_limit)
    slot_of_code = np.full(4 ** k, -1, np.int64)
    slot_of_code[codes] = np.arange(codes.size)
    reads_of = collections.defaultdict(list)
    for r, rc in enumerate(_read_codes(k)):
        cand = [int(x) for x in np.unique(slot_of_code[rc]) if x >= 0]
        before = [o.count(x) for x in cand]
        rcs = o.run_batch(b.slice_reads(r, r + 1))
        assert rcs in ([0], [1], [2]), (r, rcs)
        for x, c0 in zip(cand, before):
            reads_of[x] += [r] * (o.count(x) - c0)
        if rcs == [2]:   # every k-mer of the list is complete: the reference stops reading, and no later read could add an event
            break
    counts = o.counts()
    told = np.zeros(counts.size, np.uint64)
    for x, rs in reads_of.items():
        told[x] = len(rs)
    assert np.array_equal(told, counts), "an event in a slot whose k-mer its read does not hold"
    nz = [int(x) for x in np.flatnonzero(counts)]
    ev_len = np.concatenate([o.event_lens(x) for x in nz]).astype(np.uint32) if nz else np.zeros(0, np.uint32)
    ev_read = np.concatenate([np.asarray(reads_of[x], np.uint32) for x in nz]) if nz else np.zeros(0, np.uint32)
    samples = np.concatenate([o.values(x) for x in nz]) if nz else np.zeros(0, np.float64)
    return Expected(counts, ev_len, ev_read, samples)


class Case:
    def __init__(self, n_slots):
        self.n_slots = n_slots
        self.k = smallest_k(n_slots)
        self.key_bits = key_bits_of(n_slots)
        self.path = path_of(n_slots)
        self.named = named_slots(n_slots)
        self.codes = list_codes(self.k, n_slots, seed=n_slots)
        self.kmers = _full(self.k)[self.codes].astype(f"U{self.k}").tolist()
        self.params = dict(kmer_size=self.k, scaling=1, sample_limit=LIMIT)
        self.cut = run_oracle(self.kmers, self.codes, self.k, LIMIT)          # what a job with sample_limit 2 keeps
        self.all = run_oracle(self.kmers, self.codes, self.k, NO_LIMIT)       # every accepted event
        self.check()

    def regions_hit(self):
        _, lo = part_digits(self.n_slots)
        return np.unique(np.flatnonzero(self.all.counts) >> lo)

    def check(self):
        """the conditions without which a comparison would pass vacuously, from the oracle alone"""
        acc = self.all.counts
        assert np.array_equal(self.cut.counts, np.minimum(acc, LIMIT)), self.n_slots
        assert all(acc[s] > 0 for s in self.named), (self.n_slots, [(s, int(acc[s])) for s in self.named])
        assert any(acc[s] > LIMIT for s in self.named), (self.n_slots, [(s, int(acc[s])) for s in self.named])
        if self.path == "partitioned":
            hi, lo = part_digits(self.n_slots)
            last = (self.n_slots - 1) >> lo           # the last region that has a slot
            hit = self.regions_hit()
            if self.n_slots == (1 << (self.key_bits - 1)) + 1:
                assert last + 1 < (1 << hi) and hit.max() == last, (self.n_slots, last, hit.max())   # regions beyond it: no slot, no event
            else:
                assert last + 1 == (1 << hi)
            assert hit.size == last + 1, (self.n_slots, hit.size, last + 1)                            # every region with slots has events

    def base_for_collect(self):
        """a base for pg_collect that is non-zero in the named slots: one event short of the limit, at it, beyond it, in turn"""
        base = np.zeros(self.n_slots, np.uint64)
        for i, s in enumerate(self.named):
            base[s] = 1 + i % 3
        return base

    def expected_after_base(self, base):
        room = np.where(base >= LIMIT, 0, LIMIT - base.astype(np.int64)).astype(np.uint64)
        return self.all.first_events(room)


@functools.lru_cache(maxsize=None)
def case(n_slots):
    return Case(n_slots)


def clear_caches():
    case.cache_clear(); _full.cache_clear()
