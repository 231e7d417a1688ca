"""Constructed batches for the dense gathers (pg_place.hip: k_gather_wave, k_gather_evpair, k_gather_chunks<G, P>) whose kept events
are known exactly, and a numpy restatement of the gather alone. No GPU and no engine here: only the Batch data holder is imported.

Base recipe: kmer_size 1, DNA, every base 'A', every op a match, kmer_pick_margin 0, min_dur 1, sample_limit 10^6. Every op is then an
accepted event of slot 0 and the kept order is the op order; an op outside [min_dur, max_dur] is dropped. The window of an op is
[query_start + prefix - margin, query_start + prefix + op_n + margin), cut at the read's length (gmove.cpp:928-941).

A family is a list of Case; its builder asserts from the geometry constants below and from its own lengths that it reaches the edge it
is named for (the `reaches` list says which). The constants restate macros and template arguments of the kernels;
test_gather_cases_host.py compares them with the sources, so that a retuned kernel fails there instead of silently moving the edges.
"""
import functools
from dataclasses import dataclass, field

import numpy as np

# ---- geometry of the dense gathers (name of the macro / template argument behind each) ---------------------------------------------
GROUP = 64          # WAVE: kept events a wave of k_gather_wave / k_gather_evpair owns at a time
SPAN = 4096         # PG_GW_SPAN: output samples per bit map of k_gather_wave
PAIR_SPAN = 2048    # SPAN2 = PG_GW_SPAN / 2: pair slots per bit map of k_gather_evpair
SUB = 1024          # PG_G2_SUB: kept events per sub-chunk (k_gather_chunks holds one in LDS)
SEG = 2048          # PG_GW_SEG: kept events per segment of a chunk (wave and event-pair forms)
FINE = 8192         # PG_CHUNK_FINE: fine chunk sums; more chunks than this double sub_per_chunk
LANE_FORMS = ((4, 4), (8, 3), (16, 2))   # k_gather_chunks<G, P>: windows above 2 * G * P samples take the loop of gather_finish
DENSE_MIN_DEFAULT = 64 * 4096            # pg_api.hip: dense_min(); the chunked gather needs a larger cap on kept events (or PGMOVE_DENSE_MIN)

# calibrations (digitisation, offset, range): they differ from read to read, so a mixed-up read shows in the bits
CALS = ((2048.0, -240.0, 281.0), (2048.0, -243.0, 281.345551), (8192.0, 12.0, 1437.976685), (8192.0, -101.5, 1437.976685),
        (2048.0, 12.0, 281.0), (8192.0, -240.0, 1437.976685))

BASE_P = dict(kmer_size=1, kmer_pick_margin=0, min_dur=1, sample_limit=10 ** 6, margin=0)
PA = (40.0, 180.0)


@dataclass
class Case:
    name: str
    batch: object
    p: dict                      # GmoveParams names, without scaling / pa_min / pa_max / kmers
    reaches: list = field(default_factory=list)   # the edges the builder asserted
    base_recipe: bool = True     # False: the kmers family (the oracle is the only reference)


def chunk_geometry(n_kept_cap):
    """pg_gather_chunks: (sub_per_chunk, chunks) for a cap on kept events."""
    m = 1
    while (n_kept_cap + m * SUB - 1) // (m * SUB) > FINE:
        m *= 2
    return m, (n_kept_cap + m * SUB - 1) // (m * SUB)


# ---- builder ---------------------------------------------------------------------------------------------------------------------
def build_batch(op_n, ops_per_read, lead, trail, seed, bases=None):
    """Reads of match ops only. op_n: every op's length; ops_per_read: ops of each read; lead: query_start of each read (unused samples
    in front of its first op); trail: unused samples behind its last op. bases: one per op (default 'A'). Vectorised: no loop per read."""
    from poregen_amd.engine import Batch
    op_n = np.asarray(op_n, np.int64); npr = np.asarray(ops_per_read, np.int64)
    lead = np.asarray(lead, np.int64); trail = np.asarray(trail, np.int64)
    n = npr.size
    assert n and npr.min() >= 1 and int(npr.sum()) == op_n.size and lead.size == n and trail.size == n and op_n.min() >= 1
    op_off = np.concatenate([[0], np.cumsum(npr)])
    cs = np.concatenate([[0], np.cumsum(op_n)])
    L = lead + (cs[op_off[1:]] - cs[op_off[:-1]]) + trail
    sig_off = np.concatenate([[0], np.cumsum(L)])
    rng = np.random.default_rng(seed)
    cal = np.asarray(CALS)[rng.integers(0, len(CALS), n)]
    cal[1:][np.all(cal[1:] == cal[:-1], axis=1)] = CALS[0]   # (two neighbours may still agree; most do not)
    dig, off, rg = (np.ascontiguousarray(cal[:, i]) for i in range(3))
    scale = rg / dig
    rid = np.repeat(np.arange(n), L)
    total = int(sig_off[-1])
    raw = np.rint(rng.standard_normal(total) * 60.0 + (95.0 / scale - off)[rid])          # ~N(centre, 60) raw codes around 95 pA
    hot = rng.random(total) < 0.02                                                        # ~2 % above pa_max: zero-filled per sample
    raw[hot] = np.rint((rng.uniform(200.0, 260.0, int(hot.sum())) / scale[rid[hot]]) - off[rid[hot]])
    sig = np.clip(raw, -32768, 32767).astype(np.int16)
    seq = np.full(op_n.size, ord("A"), np.uint8) if bases is None else np.frombuffer(b"ACGT", np.uint8)[np.asarray(bases)]
    return Batch(n_reads=n, sig=sig, sig_off=sig_off.astype(np.uint64), digitisation=dig, offset=off, range=rg,
                 query_start=lead.astype(np.int32), target_start=np.zeros(n, np.int32), target_end=npr.astype(np.int32),
                 seq=np.ascontiguousarray(seq), seq_off=op_off.astype(np.uint64), op_n=op_n.astype(np.uint32),
                 op_t=np.zeros(op_n.size, np.uint8), op_off=op_off.astype(np.uint64)).validate_host()


def _cut(n_ops, pattern, min_last=1):
    """ops per read: the pattern cycled until n_ops are used; a last read below min_last ops joins the one in front of it"""
    out = []; left = n_ops; k = 0
    while left:
        c = min(left, pattern[k % len(pattern)]); out.append(c); left -= c; k += 1
    if len(out) > 1 and out[-1] < min_last:
        out[-2] += out.pop()
    return out


def _pads(n):
    """default unused samples in front of and behind each read: enough for a median and a MAD that are not degenerate, and of both
    parities so that signal starts and window sources are odd and even"""
    r = np.arange(n)
    return 16 + r % 5, 17 + r % 3


def from_ops(ops, pattern, seed, lead=None, trail=None, bases=None, min_last=1):
    npr = _cut(len(ops), pattern, min_last)
    dl, dt = _pads(len(npr))
    return build_batch(ops, npr, dl if lead is None else lead, dt if trail is None else trail, seed, bases)


# ---- the kept events of a base-recipe batch, and the gather restated -------------------------------------------------------------------
def kept_events(b, p):
    """(read, global source index of the window's first sample, window length) of every kept event, in kept order"""
    assert p["kmer_size"] == 1 and p["kmer_pick_margin"] == 0 and not np.any(b.op_t) and np.all(b.seq == ord("A")), "base recipe only"
    opn = b.op_n.astype(np.int64); op_off = b.op_off.astype(np.int64); sig_off = b.sig_off.astype(np.int64)
    rd = np.repeat(np.arange(b.n_reads), np.diff(op_off))
    cs = np.cumsum(opn) - opn
    prefix = cs - cs[op_off[:-1]][rd]
    L = np.diff(sig_off)
    qs = b.query_start.astype(np.int64)
    m = int(p.get("margin", 0))
    start = qs[rd] + prefix - m
    end = np.minimum(qs[rd] + prefix + opn + m, L[rd])
    keep = (opn >= p["min_dur"]) & (opn <= p["max_dur"])
    assert np.all(start[keep] >= 0) and np.all(end[keep] > start[keep]), "outside the reference's defined behaviour (rc -5)"
    assert int(keep.sum()) <= p["sample_limit"]
    return rd[keep], (sig_off[:-1][rd] + start)[keep], (end - start)[keep]


def expected(b, p, medmad=None):
    """The gather alone in numpy, float64, in the reference's order of operations: pA = (raw + offset) * (range / digitisation), zero
    outside [pa_min, pa_max], then (x - med) / mad with scaling 1 (medmad: per read, from Oracle.run_batch(b, record_medmad=True))."""
    rd, src, ln = kept_events(b, p)
    samp_off = np.concatenate([[0], np.cumsum(ln)]).astype(np.uint64)
    total = int(samp_off[-1])
    idx = np.repeat(src - samp_off[:-1].astype(np.int64), ln) + np.arange(total)
    rs = np.repeat(rd, ln)
    pa = (b.sig[idx].astype(np.float64) + b.offset[rs]) * (b.range / b.digitisation)[rs]
    x = np.where((pa < p.get("pa_min", PA[0])) | (pa > p.get("pa_max", PA[1])), 0.0, pa)
    if p.get("scaling", 0) == 1:
        mm = np.asarray(medmad, np.float64).reshape(b.n_reads, 2)
        x = (x - mm[:, 0][rs]) / mm[:, 1][rs]
    counts = np.zeros(4, np.uint64); counts[0] = ln.size
    return dict(counts=counts, ev_len=ln.astype(np.uint32), ev_read=rd.astype(np.uint32), samp_off=samp_off, samples=x)


# ---- what a list of kept window lengths reaches -----------------------------------------------------------------------------------
def group_view(ln, unit=1):
    """per group of GROUP consecutive kept events: (offsets inside the group, lengths, lengths in samples), the first two in samples
    (unit 1) or pair slots (unit 2)"""
    smp = np.asarray(ln, np.int64)
    ln = smp if unit == 1 else (smp + 1) // 2
    for g in range(0, ln.size, GROUP):
        x = ln[g:g + GROUP]
        yield np.cumsum(x) - x, x, smp[g:g + GROUP]


def tile_facts(ln, unit=1):
    """what the tile loop of the wave form (unit 1, tiles of SPAN samples) or of the event-pair form (unit 2, tiles of PAIR_SPAN pair
    slots) meets in these kept events"""
    span = SPAN if unit == 1 else PAIR_SPAN
    f = dict(totals=[], second_tile=False, empty_tile=False, starts_in_front=False, start_on_last=False, start_on_first=False,
             one_before=set(), one_after=set(), one_before_samples=set(), one_after_samples=set())
    for off, x, smp in group_view(ln, unit):
        tot = int(x.sum()); f["totals"].append(tot)
        tiles = (tot + span - 1) // span
        f["second_tile"] |= tiles > 1
        have = set((off // span).tolist())
        f["empty_tile"] |= any(t not in have for t in range(tiles))
        if tiles > 1:
            end = off + x
            f["starts_in_front"] |= bool(np.any((off // span) < ((end - 1) // span)))
            f["start_on_last"] |= bool(np.any((off % span == span - 1) & (off // span < tiles - 1)))
            f["start_on_first"] |= bool(np.any((off % span == 0) & (off > 0)))
            cross = (off // span) < ((end - 1) // span)
            f["one_before"] |= set((x[cross & (off % span == span - 1)] % 2).tolist())   # one unit in front of the boundary: parities of the length
            f["one_after"] |= set((x[cross & (end % span == 1)] % 2).tolist())           # one unit behind it
            f["one_before_samples"] |= set((smp[cross & (off % span == span - 1)] % 2).tolist())   # the same windows: parities of the length in samples
            f["one_after_samples"] |= set((smp[cross & (end % span == 1)] % 2).tolist())
    return f


def _base_parities(ln):
    """parity of the first output index of every group"""
    ln = np.asarray(ln, np.int64)
    return (np.concatenate([[0], np.cumsum(ln)])[:-1][::GROUP] % 2).tolist()


# ---- group construction ---------------------------------------------------------------------------------------------------------------
def _group(total, must, forbid, rng, n=GROUP):
    """n window lengths that sum to `total`: starts at 0, at every offset of `must`, at none of `forbid`, the others drawn"""
    must = sorted(set([0]) | set(must))
    free = np.setdiff1d(np.arange(1, total), np.asarray(sorted(set(must) | set(forbid))))
    starts = np.sort(np.concatenate([must, rng.choice(free, n - len(must), replace=False)]))
    ln = np.diff(np.concatenate([starts, [total]]))
    assert ln.size == n and ln.min() >= 1 and int(ln.sum()) == total
    return ln.tolist()


def _boundary_variants(B, total):
    """(must, forbid) for windows around offset B inside a group of `total` units: a start on the last unit in front of B and one on B;
    windows with one unit in front of B and lengths 2 and 3; windows with one unit behind B and lengths 4 and 3"""
    v = []
    if total > B:
        v.append(({B}, set()))
        v.append(({B - 2, B + 1} if total > B + 1 else {B - 2}, {B - 1, B}))             # [B - 2, B + 1): length 3, one unit behind B
        v.append(({B - 3, B + 1} if total > B + 1 else {B - 3}, {B - 2, B - 1, B}))      # length 4
    if total > B + 2:
        v.append(({B - 1, B}, set()))                                                     # length 1 on the last unit, next one on B
        v.append(({B - 1, B + 1}, {B}))                                                   # length 2, one unit in front
        v.append(({B - 1, B + 2}, {B, B + 1}))                                            # length 3
    return v or [(set(), set())]


def _tile_groups(rng):
    """sample groups for the wave form, then pair-slot groups for the event-pair form"""
    groups = []
    for total in (SPAN - 1, SPAN, SPAN + 1, 2 * SPAN, 2 * SPAN + 1):
        for must, forbid in _boundary_variants(SPAN, total):
            groups.append(_group(total, must, forbid, rng))
    for slots in (PAIR_SPAN - 1, PAIR_SPAN, PAIR_SPAN + 1, 2 * PAIR_SPAN + 1):
        for must, forbid in _boundary_variants(PAIR_SPAN, slots):
            s = np.asarray(_group(slots, must, forbid, rng))
            for phase in (0, 1):   # odd and even window lengths in every group; both phases: every window at a boundary has an odd and an even length
                groups.append((2 * s - (np.arange(s.size) + phase) % 2).tolist())
    return groups


LONG_OPS = ([1, SPAN - 1, 1, SPAN, 1, SPAN + 1, 1, 2 * SPAN - 1, 1, 2 * SPAN + 1, 1, 9000, 1, 9000, SPAN + 1, 1] + [1] * 48   # group 0: single long windows, two back to back
            + [9000] + [1] * 63                                                                                            # group 1: one long window, then 63 ones
            + [x for e in (31, 32, 33, 47, 48, 49, 63, 64, 65, 129) for x in (e, 1)] + [2, 3] * 22)                         # group 2: the 2 * G * P edges
assert len(LONG_OPS) == 3 * GROUP


def _assert_long(ln, reaches):
    for unit, form in ((1, "k_gather_wave"), (2, "k_gather_evpair")):
        f = tile_facts(ln, unit)
        assert f["second_tile"] and f["empty_tile"] and f["starts_in_front"], (form, f)
        reaches.append(f"{form}: tb > 0, a tile without a window start, events that start in front of a tile")
    for G, P in LANE_FORMS:
        e = 2 * G * P
        assert {e - 1, e, e + 1} <= set(int(x) for x in ln) and max(ln) > 2 * e
        reaches.append(f"k_gather_chunks<{G},{P}>: windows of {e - 1}, {e}, {e + 1} samples and the gather_finish loop")


# ---- families ---------------------------------------------------------------------------------------------------------------------
CYCLE = (1, 2, 3, 2, 3, 1, 3, 1, 2, 1)   # lengths 1, 2, 3 in turn; the odd sum of a period puts each of them on both output parities
COUNTS_N = (1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049)


@functools.lru_cache(maxsize=None)
def counts():
    out = []
    for n in COUNTS_N:
        for variant, ops in (("ones", [1] * n), ("cycle", [CYCLE[i % len(CYCLE)] for i in range(n)])):
            b = from_ops(ops, (1, 2, 3, 4, 5), seed=1000 + n)
            p = dict(BASE_P, max_dur=3)
            rd, src, ln = kept_events(b, p)
            assert ln.size == n and ln.tolist() == ops
            reaches = [f"n_kept = {n}"]
            if n >= GROUP:
                assert np.unique(rd[:GROUP]).size >= 13; reaches.append("a group of 64 events spans at least 13 reads")
            if variant == "cycle" and n >= 2 * len(CYCLE):
                so = np.cumsum(ln) - ln
                assert {(int(a) % 2, int(l)) for a, l in zip(so, ln)} == {(a, l) for a in (0, 1) for l in (1, 2, 3)}
                reaches.append("windows of 1, 2, 3 samples at both output parities")
            if variant == "ones" and n >= 2:
                assert set((src % 2).tolist()) == {0, 1}; reaches.append("1-sample windows at odd and even source indices")
            out.append(Case(f"n{n}-{variant}", b, p, reaches))
    return out


@functools.lru_cache(maxsize=None)
def tile():
    rng = np.random.default_rng(4096)
    groups = _tile_groups(rng)
    shift = [1] * 63 + [2]                                    # an odd group in front: every later group's first output index changes parity
    out = []; par = []
    for name, gl in (("as-built", groups), ("shifted", [shift] + groups)):
        ops = [x for g in gl for x in g]
        b = from_ops(ops, (5, 9, 13, 7, 3), seed=77)
        p = dict(BASE_P, max_dur=max(ops))
        rd, src, ln = kept_events(b, p)
        assert ln.tolist() == ops
        reaches = []
        f1, f2 = tile_facts(ln, 1), tile_facts(ln, 2)
        assert {SPAN - 1, SPAN, SPAN + 1, 2 * SPAN, 2 * SPAN + 1} <= set(f1["totals"]); reaches.append("groups of 4095, 4096, 4097, 8192, 8193 samples")
        assert {PAIR_SPAN - 1, PAIR_SPAN, PAIR_SPAN + 1, 2 * PAIR_SPAN + 1} <= set(f2["totals"]); reaches.append("groups of 2047, 2048, 2049, 4097 pair slots")
        for f, what in ((f1, "samples"), (f2, "pair slots")):
            assert f["second_tile"] and f["starts_in_front"] and f["start_on_last"] and f["start_on_first"], f
            assert f["one_before"] == {0, 1} and f["one_after"] == {0, 1}, f
            assert f["one_before_samples"] == {0, 1} and f["one_after_samples"] == {0, 1}, f
            reaches.append(f"{what}: a start on a tile's last unit and on the next tile's first; windows with one unit on either side of a boundary, "
                           f"of an odd and an even number of {what} and of an odd and an even number of samples")
        assert np.unique(rd[:GROUP]).size >= 5; reaches.append("groups mix reads of different calibrations")
        par.append(_base_parities(ln)[len(gl) - len(groups):])
        out.append(Case(name, b, p, reaches))
    assert all(a != c for a, c in zip(*par)), "every group starts at an odd output index in one placement and at an even one in the other"
    return out


@functools.lru_cache(maxsize=None)
def long():
    b = from_ops(LONG_OPS, (1, 2, 3), seed=9000)
    p = dict(BASE_P, max_dur=9000)
    rd, src, ln = kept_events(b, p)
    assert ln.tolist() == LONG_OPS
    reaches = []
    _assert_long(ln, reaches)
    assert ln[GROUP] == 9000 and np.all(ln[GROUP + 1:2 * GROUP] == 1); reaches.append("a group that is one 9000-sample window and 63 ones")
    return [Case("long", b, p, reaches)]


@functools.lru_cache(maxsize=None)
def ends():
    out = []
    for last in (1, 2, 3, 9000):
        for parity in (0, 1):
            for unused in (0, 1):
                ops = [3, 1, 2] * 23 + [last]
                npr = _cut(len(ops), (4, 5, 3))
                lead, trail = (x.copy() for x in _pads(len(npr)))
                lead[0] = 0; trail[-1] = unused
                for _ in range(2):
                    b = build_batch(ops, npr, lead, trail, seed=500 + last)
                    p = dict(BASE_P, max_dur=max(3, last))
                    rd, src, ln = kept_events(b, p)
                    if int(src[-1]) % 2 == parity:
                        break
                    lead[-1] += 1
                total = int(b.sig_off[-1])
                assert src[0] == 0, "the first kept window starts at sample 0"
                assert int(src[-1] + ln[-1]) == total - unused and ln[-1] == last and int(src[-1]) % 2 == parity
                assert ln.size > GROUP
                reaches = [f"the last window ({last} samples, source index {'odd' if parity else 'even'}) ends {unused} samples in front of sig_off[-1]: "
                           "2 * d + 3 < total fails in gather_load / gather_finish, `tail` in k_gather_evpair"]
                out.append(Case(f"last{last}-{'odd' if parity else 'even'}-unused{unused}", b, p, reaches))
    return out


@functools.lru_cache(maxsize=None)
def margin():
    out = []
    for m in (1, 3, 150):
        sets = [(f"cycle{n}", [CYCLE[i % len(CYCLE)] for i in range(n)], (3, 4, 5, 6, 7), 3) for n in (65, 1025, 2049)] + [("long", LONG_OPS, (1, 2, 3), 9000)]
        for name, ops, pattern, max_dur in sets:
            npr = _cut(len(ops), pattern)
            b = build_batch(ops, npr, np.full(len(npr), m), np.zeros(len(npr), np.int64), seed=150 + m)
            p = dict(BASE_P, max_dur=max_dur, margin=m)
            assert (max_dur + 2 * m + 1) * 4096 < 2 ** 32 and len(ops) * (max_dur + 2 * m) * 8 < 2 ** 30
            rd, src, ln = kept_events(b, p)
            assert ln.size == len(ops) and np.all(b.query_start == m)
            first = np.concatenate([[True], rd[1:] != rd[:-1]]); last_ = np.concatenate([rd[1:] != rd[:-1], [True]])
            assert np.all(src[first] == b.sig_off[:-1].astype(np.int64)), "query_start == margin: every read's first window starts on its first sample"
            assert np.all(ln[last_] < np.asarray(ops)[last_] + 2 * m), "every read's last window is clipped at the read's end"
            assert np.all((src + ln)[last_] == b.sig_off[1:].astype(np.int64))
            reaches = [f"margin {m}: smallest legal start, clipped last windows, overlapping sources"]
            if m == 3 and name != "long":
                assert ln[0] == ops[0] + 6 and ln[-1] == ops[-1] + 3   # a first window of 7 samples, a last one of op + 3
            if m == 150:
                assert tile_facts(ln, 1)["second_tile"] and tile_facts(ln, 2)["second_tile"]; reaches.append("short ops, yet several tiles per group")
            out.append(Case(f"m{m}-{name}", b, p, reaches))
    return out


@functools.lru_cache(maxsize=None)
def rejected():
    ops = [(1, 2, 3, 4, 11, 12, 20)[i % 7] for i in range(3000)]
    b0 = from_ops(ops, (2, 3, 5), seed=31)
    p0 = dict(BASE_P, min_dur=5, max_dur=10)
    assert kept_events(b0, p0)[2].size == 0
    ops = [(1 + (i // 2) % 3) if i % 2 == 0 else 4 + (i // 2) % 6 for i in range(4100)]
    b1 = from_ops(ops, (2, 3, 5), seed=32)
    p1 = dict(BASE_P, max_dur=3)
    n = kept_events(b1, p1)[2].size
    m, chunks = chunk_geometry(len(ops))
    assert n == 2050 and m == 1 and chunks == 5 and (n + SUB - 1) // SUB == 3
    return [Case("none-kept", b0, p0, ["n_kept = 0 with 3000 ops: the blockIdx.x == 0 early exit"]),
            Case("every-second", b1, p1, ["5 chunks launched for the cap of 4100 ops, 2 of them behind n_kept = 2050, the third holds 2 events"])]


@functools.lru_cache(maxsize=None)
def chunks():
    n = 65 * SUB + 1
    ops = np.random.default_rng(65).integers(1, 4, n)
    b = from_ops(ops.tolist(), (11, 17, 23, 5), seed=65)
    p = dict(BASE_P, max_dur=3)
    assert kept_events(b, p)[2].size == n
    m, c = chunk_geometry(n)
    assert m == 1 and c == 66 and n - 65 * SUB == 1
    return [Case("65k+1", b, p, ["66 chunks: chunk_base adds a coarse sum for chunks 64 and 65, the last chunk holds one event"])]


@functools.lru_cache(maxsize=None)
def kmers():
    ops = LONG_OPS + [x for g in _tile_groups(np.random.default_rng(4096)) for x in g]
    out = []
    for k in (6, 3):
        b = from_ops(ops, (9, 12, 17), seed=60 + k, bases=np.random.default_rng(k).integers(0, 4, len(ops)), min_last=k)
        p = dict(BASE_P, kmer_size=k, max_dur=9000)
        assert len(ops) * 9000 * 8 < 2 ** 30 and max(ops) > 2 * SPAN
        out.append(Case(f"k{k}", b, p, [f"k = {k}: {4 ** k} slots, the long and tile lengths in slot-major order"], base_recipe=False))
    return out


SEGMENTS_N = 16_777_216 + 5_000


def segments():
    """One batch; built vectorised. Its only reference is expected(). Not cached: 16.8 M events; the caller holds it as long as it needs it."""
    rng = np.random.default_rng(16)
    ops = rng.integers(1, 3, SEGMENTS_N)
    npr = []; left = SEGMENTS_N; r = 0
    while left:
        c = min(left, 2048 + 37 * (r % 29)); npr.append(c); left -= c; r += 1
    lead, trail = _pads(len(npr))
    b = build_batch(ops, npr, lead, trail, seed=17)
    p = dict(BASE_P, max_dur=2, sample_limit=10 ** 8)
    m, c = chunk_geometry(SEGMENTS_N)
    assert SEGMENTS_N > 2 * FINE * SUB and m == 4 and m * SUB == 2 * SEG and SEGMENTS_N % (m * SUB) != 0
    assert SEGMENTS_N * (2 + 0) * 8 < 2 ** 30
    return Case("segments", b, p, [f"sub_per_chunk 4: {c} chunks of two segments (the seg != c0 barrier) / four sub-chunks, the last chunk partial"])


FAMILIES = dict(counts=counts, tile=tile, long=long, ends=ends, margin=margin, rejected=rejected, chunks=chunks, kmers=kmers)


# ---- references, computed once per process and shared by the tests -----------------------------------------------------------------------
def kmer_list(p):
    import itertools
    return ["".join(t) for t in itertools.product("ACGT", repeat=p["kmer_size"])]


@functools.lru_cache(maxsize=None)
def oracle_run(family, index, scaling, pa_min=PA[0], pa_max=PA[1]):
    """(oracle, return codes, per-read (median, MAD)) of one case"""
    from helpers import oracle_for
    c = FAMILIES[family]()[index]
    p = dict(c.p, scaling=scaling, pa_min=pa_min, pa_max=pa_max)
    o = oracle_for(kmer_list(p), **p)
    rcs = o.run_batch(c.batch, record_medmad=True)
    return o, rcs, list(o.medmad)


@functools.lru_cache(maxsize=None)
def reference(family, index, scaling, pa_min=PA[0], pa_max=PA[1]):
    """(expected(...), the oracle's sample stream, the oracle's event lengths) of a base-recipe case"""
    c = FAMILIES[family]()[index]
    o, rcs, mm = oracle_run(family, index, scaling, pa_min, pa_max)
    e = expected(c.batch, dict(c.p, scaling=scaling, pa_min=pa_min, pa_max=pa_max), mm)
    return e, o.all_values(), o.all_event_lens()


def clear_caches():
    """drop the families, oracles and references held for sharing (a test module calls this when it is through)"""
    for f in (*FAMILIES.values(), oracle_run, reference):
        f.cache_clear()
