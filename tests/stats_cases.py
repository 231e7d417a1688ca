"""Inputs for the read statistics kernels (k_read_plan, k_read_stats, the rare workers: poregen_amd/csrc/pg_kernels.hip) in which EVERY
sample decides -- the median and the MAD are robust, so on realistic signals a sample that is dropped, binned twice or taken from the
neighbouring read changes neither. tests/test_stats_cases_host.py proves what is claimed here, tests/test_gpu_stats_edges.py runs the
groups on the device.

Sentinel reads. Three values: two in-range codes A < B (pA > 0) and out-of-range samples, which the reference zero-fills (Z = 0.0 < A).
The sorted vector is Z.. A.. B.. and the upper median is element k = L // 2.
  "loss" read: nZ + nA == k, so the median is the FIRST B. A B that is not counted becomes a zero-filled sample (nZ = L - in-range):
               the median drops to A (or to 0.0).
  "dup"  read: nZ + nA == k + 1, so the median is the LAST A (or the last Z). A B counted twice takes a zero-filled sample's place: the
               median rises to B.
A group holds as many reads of either kind as it takes for every position of the read to carry a B in one of them (two loss reads, three
dup reads from five samples on; reads of two samples show a doubled B in the MAD; a doubled sample of a one-sample read leaves the
selection's domain -- more samples counted than the read has -- and is not claimed). sentinel_flags() evaluates the property from the class
counts alone.

Everything is generated from integers (splitmix64, as tests/ksmall_vectors.py); CRCS pins the bytes of every group.
Nothing here computes a statistic with the product: the expected values are the oracle's (orc_median / orc_madf)."""
import functools
import math
import zlib

import numpy as np

from ksmall_vectors import splitmix64, bits  # noqa: F401  (bits: re-exported for the tests)

SCALE1 = (2048.0, 0.0, 2048.0)   # digitisation == range: scale 1.0, pA = code + offset


class Group:
    """Reads of one engine (one pa window): raws[i] int16, cals[i] = (digitisation, offset, range), ids[i]; meta[i] free-form."""
    def __init__(self, name, pa, k1):
        self.name, self.pa, self.k1 = name, pa, k1   # k1: a k = 1 model, one base and one op per read (reads below 12 samples)
        self.raws, self.cals, self.ids, self.meta = [], [], [], []

    def add(self, id_, raw, cal, **meta):
        raw = np.asarray(raw)
        assert raw.size > 0 and raw.min() >= -32768 and raw.max() <= 32767, id_
        self.raws.append(np.ascontiguousarray(raw.astype(np.int16, copy=False))); self.cals.append(tuple(float(x) for x in cal)); self.ids.append(id_); self.meta.append(meta)
        return len(self.ids) - 1

    def __len__(self):
        return len(self.ids)

    def reversed(self):
        g = Group(self.name + "_reversed", self.pa, self.k1)
        g.raws, g.cals, g.ids, g.meta = self.raws[::-1], self.cals[::-1], self.ids[::-1], self.meta[::-1]
        return g

    def begs(self):
        return np.concatenate([[0], np.cumsum([r.size for r in self.raws])]).astype(np.int64)

    def crc(self):
        c = 0
        for r, cal in zip(self.raws, self.cals):
            c = zlib.crc32(r.tobytes(), c)
            c = zlib.crc32(np.array(cal, np.float64).tobytes(), c)
        return c & 0xFFFFFFFF

    def sample_limit(self):
        """Every read carries the same bases, so each k-mer gets one event per read: above the read count (twice, for two submits) no
        k-mer completes and no read behind it is skipped (PG_STAT_SKIP would make its statistics NaN)."""
        return 2 * len(self) + 16


def batch_of(g):
    """As _batch_of of tests/test_ksmall_golden.py: 12 bases and 12 one-sample matches per read, reads back to back in one signal buffer;
    with g.k1 one base and one op (reads shorter than 12 samples)."""
    from poregen_amd.engine import Batch
    n = len(g)
    nb = 1 if g.k1 else 12
    sig_off = g.begs().astype(np.uint64)
    cal = np.array(g.cals, np.float64)
    seq = np.tile(np.frombuffer(b"A" if g.k1 else b"ACGTTGCAAGCT", np.uint8), n)
    steps = np.arange(n + 1, dtype=np.uint64) * np.uint64(nb)
    return Batch(n_reads=n, sig=np.concatenate(g.raws), sig_off=sig_off, digitisation=np.ascontiguousarray(cal[:, 0]), offset=np.ascontiguousarray(cal[:, 1]),
                 range=np.ascontiguousarray(cal[:, 2]), query_start=np.zeros(n, np.int32), target_start=np.zeros(n, np.int32),
                 target_end=np.full(n, nb, np.int32), seq=seq, seq_off=steps, op_n=np.ones(nb * n, np.uint32), op_t=np.zeros(nb * n, np.uint8), op_off=steps.copy()).validate_host()


def engine_params(g, **kw):
    from poregen_amd.engine import GmoveParams, generate_kmers
    k = 1 if g.k1 else 5
    return GmoveParams(kmers=generate_kmers(k), kmer_size=k, scaling=1, sample_limit=g.sample_limit(), min_dur=1, max_dur=70, pa_min=g.pa[0], pa_max=g.pa[1], **kw)


def pa_zero_filled(raw, cal, pa):
    """gmove.cpp:751-760 as ksmall_vectors.pa_zero_filled, with the read's own calibration and the group's window."""
    dig, off, rng = cal
    x = (raw.astype(np.float64) + off) * (rng / dig)
    x[(x < pa[0]) | (x > pa[1])] = 0.0
    return x


def oracle_medmad(raw, cal, pa):
    """(median, madf) of the oracle on the zero-filled pA vector."""
    import orc
    L = orc.lib()
    x = pa_zero_filled(raw, cal, pa)
    med = L.orc_median(x.ctypes.data, x.size)
    return med, L.orc_madf(x.ctypes.data, x.size, med)


@functools.lru_cache(maxsize=None)
def _expected(name):
    g = GROUPS[name]()
    med, mad = np.empty(len(g)), np.empty(len(g))
    for i, (raw, cal) in enumerate(zip(g.raws, g.cals)):
        m, d = oracle_medmad(raw, cal, g.pa)
        med[i], mad[i] = m, (d if d > 1.0 else 1.0)
    return med.view(np.uint64), mad.view(np.uint64)


def expected(g):
    """The 64 bits of the expected median and MAD (= max(madf, 1.0)) of every read; computed once per group and process."""
    base = g.name[:-len("_reversed")] if g.name.endswith("_reversed") else g.name
    med, mad = _expected(base)
    return (med[::-1], mad[::-1]) if base != g.name else (med, mad)


# ---- sentinel reads ---------------------------------------------------------------------------------------------------------------
def class_medmad(L, nA, nB, vA, vB):
    """Median and MAD (clamped) of nZ = L - nA - nB zeros, nA values vA and nB values vB (0 < vA < vB), from the counts alone."""
    nZ = L - nA - nB
    if nZ < 0 or nA < 0 or nB < 0:
        return None          # more samples counted than the read has: outside the selection's domain
    k = L // 2
    med = 0.0 if k < nZ else (vA if k < nZ + nA else vB)
    if L == 1:
        return med, 1.0
    need = k
    for dev, cnt in sorted([(abs(0.0 - med), nZ), (abs(vA - med), nA), (abs(vB - med), nB)]):
        if need < cnt:
            mad = dev * 1.4826
            return med, (mad if mad > 1.0 else 1.0)
        need -= cnt
    raise AssertionError


def sentinel_flags(L, nA, nB, vA, vB):
    """{(class, change): does it move (median, MAD)} for class in "AB" and change in ("lost", "twice"): a lost in-range sample
    becomes a zero-filled one, a sample counted twice takes a zero-filled one's place. O(1) per perturbation."""
    base = class_medmad(L, nA, nB, vA, vB)
    out = {}
    for c, (dA, dB) in (("A", (1, 0)), ("B", (0, 1))):
        out[c, "lost"] = (nA if c == "A" else nB) > 0 and class_medmad(L, nA - dA, nB - dB, vA, vB) != base
        t = class_medmad(L, nA + dA, nB + dB, vA, vB)
        out[c, "twice"] = (nA if c == "A" else nB) > 0 and t is not None and t != base
    return out


def sentinel_group(L, seed, cA, cB, cZ):
    """[(kind, part, raw)]: the loss and dup reads of one geometry; cZ: the out-of-range codes to draw from (cycled)."""
    k = L // 2
    perm = np.argsort(splitmix64(seed, L), kind="stable")
    out = []
    for kind, nB in (("loss", L - k), ("dup", L - k - 1)):
        if nB <= 0:
            continue            # one or two samples: the loss reads carry the dup property (or nothing can), see the module docstring
        parts = -(-L // nB)
        for j in range(parts):
            s = min(j * nB, L - nB)
            raw = np.full(L, cA, np.int64)
            raw[perm[s:s + nB]] = cB
            rest = np.concatenate([perm[:s], perm[s + nB:]])
            nz = 1 if rest.size else 0       # one zero-filled sample (where there is room): nZ = L - in-range is then not zero by accident
            if L >= 64:
                nz = min(rest.size, 3)
            for q in range(nz):
                raw[rest[q]] = cZ[(j + q) % len(cZ)]
            out.append((kind, j, raw))
    return out


def sentinel_counts(raw, cA, cB):
    return int(np.count_nonzero(raw == cA)), int(np.count_nonzero(raw == cB))


def uncovered_positions(reads, cA, cB, vA, vB, need_twice=True):
    """Positions of a sentinel group at which a lost (a doubled) sample moves no read's (median, MAD): ([lost], [twice])."""
    L = reads[0].size
    lost, twice = np.zeros(L, bool), np.zeros(L, bool)
    for raw in reads:
        nA, nB = sentinel_counts(raw, cA, cB)
        f = sentinel_flags(L, nA, nB, vA, vB)
        for c, code in (("A", cA), ("B", cB)):
            if f[c, "lost"]: lost |= raw == code
            if f[c, "twice"]: twice |= raw == code
    return np.flatnonzero(~lost), (np.flatnonzero(~twice) if need_twice else np.zeros(0, np.int64))


# ---- A. streaming geometry, main launch ---------------------------------------------------------------------------------------------
A_PA = (40.0, 180.0)               # with SCALE1: c_lo = 40, span = 141
A_CODES = dict(cA=100, cB=120, cZ=(300, 10, -32768, 32767, 181, 39))   # above / below the window, the int16 ends, the codes next to it
A_NVEC = [1, 63, 64, 65, 511, 512, 513, 1024, 1025]


def a_geometries():
    """(head, tail, n_vec, L, tag): beg mod 8, end mod 8, whole 16-byte vectors between them, samples."""
    out = []
    for h in range(8):
        for t in range(8):
            if t != h:
                out.append((h, t, 0, (t - h) % 8, "lt8"))            # fewer than 8 samples: no whole vector
            if h >= 1 and t >= h:
                out.append((h, t, 0, 8 - h + t, "straddle"))          # 8 .. 14 samples around one boundary: still none (va >= vb)
            for nv in A_NVEC:
                out.append((h, t, nv, (8 - h) % 8 + 8 * nv + t, "nv%d" % nv))
    return out


def _place(g, cur, head, cB, tag):
    """A padding read in front of the next read so that it begins at `head` mod 8: 1 .. 8 samples of the sentinel's B (counted into the
    read behind or in front of it, they move its median)."""
    p = (head - cur) % 8 or 8
    g.add("pad_" + tag, np.full(p, cB), SCALE1, pad=True)
    return cur + p


@functools.lru_cache(maxsize=None)
def group_a():
    g = Group("A", A_PA, k1=True)
    cur = 0
    for gi, (h, t, nv, L, tag) in enumerate(a_geometries()):
        for kind, part, raw in sentinel_group(L, 7000 + gi, **A_CODES):
            gid = "h%d_t%d_%s" % (h, t, tag)
            cur = _place(g, cur, h, A_CODES["cB"], gid)
            assert cur % 8 == h and (cur + L) % 8 == t
            g.add("%s_%s%d" % (gid, kind, part), raw, SCALE1, pad=False, geom=gid, head=h, tail=t, n_vec=nv, kind=kind)
            cur += L
    g.add("pad_end", np.full(8, A_CODES["cB"]), SCALE1, pad=True)
    return g


# ---- calibrations that give a wanted interval ---------------------------------------------------------------------------------------
def cal_for(c_lo, span, pa):
    """A calibration under which the in-range codes are exactly [c_lo, c_lo + span): scale = window / (span - 1/2), the bounds a quarter
    code away from the nearest code (far above any rounding). test_stats_cases_host asserts it through pgt_plan."""
    s = (pa[1] - pa[0]) / (span - 0.5)
    off = pa[0] / s - c_lo + 0.25
    return (8192.0, off, s * 8192.0)


def counted_read(counts, n_extra, extra_codes, seed):
    """A read from {code: count} plus n_extra samples cycled from extra_codes, in a seeded order."""
    v = [np.full(n, c, np.int64) for c, n in counts.items()]
    v.append(np.array([extra_codes[i % len(extra_codes)] for i in range(n_extra)], np.int64))
    v = np.concatenate(v)
    return v[np.argsort(splitmix64(seed, v.size), kind="stable")]


# ---- B. interval and bin edges ------------------------------------------------------------------------------------------------------
B_PA = (1000.0, 1999.5)            # scale 1.0 gives 1000 codes; every other span by the read's own scale
B_SPANS = [1, 2, 15, 16, 17, 1000, 1023, 1024, 1025, 2047, 2048, 2049, 65536]
B_L = 301


def _outside(c_lo, span):
    """codes just outside [c_lo, c_lo + span) and far from it, as far as int16 has them"""
    cand = [c_lo - 1, c_lo + span, c_lo - 2, c_lo + span + 1, -32768, 32767, c_lo - 700, c_lo + span + 700]
    return [c for c in cand if -32768 <= c <= 32767 and not (c_lo <= c < c_lo + span)]


def _edge_pair(g, tag, c_lo, span, binA, binB, cZ, seed, L=B_L, **meta):
    """a loss and a dup read over the bins binA <= binB of [c_lo, c_lo + span); cZ: out-of-range codes (none: an interval of all codes)"""
    cal = cal_for(c_lo, span, g.pa)
    k = L // 2
    for kind, nB in (("loss", L - k), ("dup", L - k - 1)):
        nZ = min(len(cZ), 8)
        nlow = L - nB - nZ                   # loss: nZ + nlow == k; dup: k + 1
        counts = {c_lo + binB: nB}
        if binA != binB: counts[c_lo + binA] = nlow
        else: nZ += nlow
        if nZ and not cZ:                    # every code is in range: the lowest code plays the zero-filled class's part
            counts[c_lo] = counts.get(c_lo, 0) + nZ; nZ = 0
        g.add("%s_%s" % (tag, kind), counted_read(counts, nZ, cZ, seed), cal, c_lo=c_lo, span=span, kind=kind, **meta)


@functools.lru_cache(maxsize=None)
def group_b():
    g = Group("B", B_PA, k1=True)
    for i, span in enumerate(B_SPANS):           # the histogram's first and last bin carry the two classes, the codes next to them the rest
        c_lo = -32768 if span == 65536 else -(span // 2) + 100
        _edge_pair(g, "span%d" % span, c_lo, span, 0, span - 1, _outside(c_lo, span), 100 + i)
    # intervals touching either end of int16: code - c_lo modulo 2^16 of a sample at the opposite end equals span
    _edge_pair(g, "top_of_int16", 32768 - 1000, 1000, 0, 999, [-32768], 201)
    _edge_pair(g, "bottom_of_int16", -32768, 1000, 0, 999, [32767], 202)
    # the median's bin: the first one, either side of the first lane's last bin, the last one
    c_lo, span = 4000, 1000
    for b in (0, 15, 16, 999):
        _edge_pair(g, "median_bin%d" % b, c_lo, span, max(b - 1, 0), b, [c_lo - 1, c_lo - 300], 300 + b)
    # ... and in the last, partly valid lane (bins 992 .. 1007 of which 992 .. 999 exist): 250 samples just above the window land in the
    # real bins 1000 .. 1023 (and in the lane's running sum), 50 below it on the dummy bins; the median is the first sample of bin 995
    counts = {c_lo + 995: 150, c_lo + 996: 50, c_lo + 997: 50, c_lo + 998: 50, c_lo + 999: 50}
    for j in range(50): counts[c_lo + (j * 19) % 990] = counts.get(c_lo + (j * 19) % 990, 0) + 1
    above = [c_lo + 1000 + j for j in range(24)]
    raw = counted_read(counts, 250, above, 401)
    raw = np.concatenate([raw, np.full(50, c_lo - 5)])
    g.add("median_in_last_lane", raw[np.argsort(splitmix64(402, raw.size), kind="stable")], cal_for(c_lo, span, g.pa), c_lo=c_lo, span=span)
    # short reads, and one without an in-range sample
    cal = cal_for(c_lo, span, g.pa)
    for j, r in enumerate([[c_lo + 5], [c_lo - 1], [c_lo + 5, c_lo + 900], [c_lo + 900, c_lo - 1], [c_lo + 7, c_lo + 5, c_lo + 6], [c_lo - 1, c_lo + 999, c_lo + 1000]]):
        g.add("short%d_%d" % (len(r), j), r, cal, c_lo=c_lo, span=span)
    g.add("all_out_of_range", counted_read({}, 77, _outside(c_lo, span), 403), cal, c_lo=c_lo, span=span)
    return g


BZ_PA = (-50.0, 60.0)              # zero inside the window (tests/test_select_host.py, mode 4)


@functools.lru_cache(maxsize=None)
def group_bz():
    """pA = code - 500: codes 450 .. 560 in range, z0 = 50 negative ones; the zero-filled class sorts between code 499 and code 500."""
    g = Group("BZ", BZ_PA, k1=True)
    cal = (2048.0, -500.0, 2048.0)
    L, k = 201, 100
    neg, pos, out = [455, 470, 499], [500, 501, 540, 560], [300, 449, 561, 900]
    def read(n_neg, n_zero, seed):
        counts = {}
        for j in range(n_neg): counts[neg[j % 3]] = counts.get(neg[j % 3], 0) + 1
        for j in range(L - n_neg - n_zero): counts[pos[j % 4]] = counts.get(pos[j % 4], 0) + 1
        return counted_read(counts, n_zero, out, seed)
    for tag, n_neg, n_zero in (("median_is_zero_filled", 60, 80), ("median_first_zero_filled", k, 50), ("median_last_zero_filled", 51, 50),
                               ("median_last_negative", k + 1, 50), ("median_first_non_negative", 40, 60)):
        g.add(tag, read(n_neg, n_zero, 500 + n_neg), cal, c_lo=450, span=111, z0=50)
    # z0 at 0 and at span: the interval is cut off by the end of int16
    cal0 = (2048.0, 32768.0 + 10.0, 2048.0)          # code -32768 is pA 10: c_lo = -32768, span 51, no negative value
    g.add("z0_is_0", counted_read({-32768: 60, -32760: 41, -32718: 50}, 50, [-32717, 0, 32767], 601), cal0, c_lo=-32768, span=51, z0=0)
    cal1 = (2048.0, -32767.0 - 10.0, 2048.0)         # code 32767 is pA -10: c_lo = 32727, span 41, every value negative
    g.add("z0_is_span", counted_read({32767: 60, 32750: 41, 32727: 50}, 50, [32726, 0, -32768], 602), cal1, c_lo=32727, span=41, z0=41)
    return g


# ---- C. the rare lists ---------------------------------------------------------------------------------------------------------------
C_WIDE, C_HUGE, C_PLAIN = 130, 130, 140


@functools.lru_cache(maxsize=None)
def group_c():
    """400 reads of 100 .. 300 samples, plain / wide / huge in turn (the list of the rare reads fills from both ends at once): 130 wide
    ones (more than the 64 workers of a first batch) and 130 huge ones (more than PG_HUGE_BLOCKS) make every worker reuse its histogram.
    The samples of a read are spread over its own interval: counts left from the previous read change nV, hence nZ, median and MAD."""
    g = Group("C", B_PA, k1=False)
    wide = [1025, 2048, 2047, 1026] + [1025 + (j * 389) % 1024 for j in range(C_WIDE - 4)]
    huge = [65536, 2049, 65535, 65536, 2050] + [2049 + (j * 7919) % 63488 for j in range(C_HUGE - 5)]
    plain = [1024, 1, 1000, 17] + [1 + (j * 97) % 1024 for j in range(C_PLAIN - 4)]
    n = 0
    for j in range(max(C_WIDE, C_HUGE, C_PLAIN)):
        for kind, spans in (("plain", plain), ("wide", wide), ("huge", huge)):
            if j >= len(spans):
                continue
            span = spans[j]
            L = 100 + int(splitmix64(900 + n, 1)[0] % np.uint64(201))
            c_lo = -32768 if span == 65536 else -32768 + int(splitmix64(901 + n, 1)[0] % np.uint64(65536 - span + 1))
            u = splitmix64(10000 + n, L)
            raw = c_lo + (u % np.uint64(span)).astype(np.int64)
            raw[0], raw[L - 1] = c_lo, c_lo + span - 1                     # both ends of the interval occur
            out = _outside(c_lo, span)
            for q in range(min(len(out), 5)):
                raw[1 + q * (L // 7)] = out[q]
            g.add("%s%d_span%d" % (kind, j, span), raw, cal_for(c_lo, span, g.pa), c_lo=c_lo, span=span, kind=kind)
            n += 1
    return g


# ---- D. slices of long reads ---------------------------------------------------------------------------------------------------------
D_SLICE = 16384                    # PG_LONG_SLICE; reads above PG_LONG_MIN = 32768 samples are cut
D_LENGTHS = [2 * D_SLICE + x for x in (1, 7, 8, 9, 15, 16, 17)]
D_HEADS = [0, 1, 7]


def d_slices(L):
    """(number of slices, slice length) as pg_long_geometry; 1 slice: not split"""
    if L <= 2 * D_SLICE:
        return 1, L
    sl = D_SLICE
    while -(-L // sl) > 1024:
        sl *= 2
    return -(-L // sl), sl


def _long_group(name, specs):
    g = Group(name, A_PA, k1=True)
    cur = 0
    for gi, (h, L) in enumerate(specs):
        gid = "L%d_h%d" % (L, h)
        for kind, part, raw in sentinel_group(L, 8000 + gi, **A_CODES):
            cur = _place(g, cur, h, A_CODES["cB"], gid)
            g.add("%s_%s%d" % (gid, kind, part), raw, SCALE1, pad=False, geom=gid, head=h, kind=kind, slices=d_slices(L)[0])
            cur += L
    g.add("pad_end", np.full(8, A_CODES["cB"]), SCALE1, pad=True)
    return g


@functools.lru_cache(maxsize=None)
def group_d():
    return _long_group("D", [(h, L) for L in D_LENGTHS for h in D_HEADS] + [(0, 32768), (3, 32768), (0, 32769), (5, 32769)])


D_GIANT = [1024 * D_SLICE, 1024 * D_SLICE + 1]      # 1024 slices of 16384; 513 slices of 32768 (the slice is doubled)


def giant_risk(L):
    """Positions of a giant read that a wrong slice could lose or double: 16 samples on either side of every multiple of 16384 (every slice
    boundary of both slice lengths), the first and the last 64."""
    edges = np.arange(0, L + D_SLICE, D_SLICE, dtype=np.int64)
    p = (edges[:, None] + np.arange(-16, 16, dtype=np.int64)[None, :]).ravel()
    p = np.concatenate([p, np.arange(64), np.arange(L - 64, L)])
    return np.unique(p[(p >= 0) & (p < L)])


def giant_pair(L, seed, cA, cB, cZ):
    """One loss and one dup read (a full group of 16.7 M-sample reads costs the oracle ten seconds): both carry B's at giant_risk(L), the
    rest of the B's on a seeded affine walk over the read. The per-position property of whole groups is group D's."""
    k = L // 2
    risk = giant_risk(L)
    mult = 2 * int(splitmix64(seed, 1)[0] % np.uint64(L // 4)) + 1
    while math.gcd(mult, L) != 1:
        mult += 2
    walk = (np.arange(L, dtype=np.int64) * mult + seed) % L
    out = []
    for kind, nB in (("loss", L - k), ("dup", L - k - 1)):
        is_b = np.zeros(L, bool); is_b[risk] = True
        fill = walk[~is_b[walk]]
        is_b[fill[:nB - risk.size]] = True
        raw = np.where(is_b, np.int16(cB), np.int16(cA)).astype(np.int16)
        raw[fill[nB - risk.size:nB - risk.size + 3]] = cZ[:3]
        out.append((kind, 0, raw))
    return out


@functools.lru_cache(maxsize=None)
def group_d_giant():
    g = Group("D_giant", A_PA, k1=True)
    cur = 0
    for gi, (h, L) in enumerate([(3, D_GIANT[0]), (6, D_GIANT[1])]):
        gid = "L%d_h%d" % (L, h)
        for kind, part, raw in giant_pair(L, 8100 + gi, **A_CODES):
            cur = _place(g, cur, h, A_CODES["cB"], gid)
            g.add("%s_%s%d" % (gid, kind, part), raw, SCALE1, pad=False, geom=gid, head=h, kind=kind, slices=d_slices(L)[0])
            cur += L
    g.add("pad_end", np.full(8, A_CODES["cB"]), SCALE1, pad=True)
    return g


# ---- E. the selection paths ----------------------------------------------------------------------------------------------------------
class Rng:
    """splitmix64 stream: integers, and doubles made of them by exact operations (no libm)"""
    def __init__(self, seed):
        self.seed, self.i = seed, 0

    def u64(self, n=1):
        v = splitmix64(self.seed * 1000003 + self.i, n); self.i += n
        return v

    def below(self, n):
        return int(self.u64()[0] % np.uint64(n))

    def choice(self, seq):
        return seq[self.below(len(seq))]

    def unit(self):
        return float(self.u64()[0] >> np.uint64(11)) * 2.0 ** -53

    def uniform(self, lo, hi):
        return lo + (hi - lo) * self.unit()

    def normal_codes(self, mean, sd, n):
        u = self.u64(n)
        s4 = ((u & np.uint64(0xFFFF)) + ((u >> np.uint64(16)) & np.uint64(0xFFFF)) + ((u >> np.uint64(32)) & np.uint64(0xFFFF)) + (u >> np.uint64(48))).astype(np.int64)
        return int(mean) + (((s4 - 131070) * int(sd * 64)) // (37837 * 64))     # four 16-bit uniforms: sd 37837

    def mask(self, n, per_mille):
        return (self.u64(n) % np.uint64(1000)).astype(np.int64) < per_mille


E_N = 250
E_LENGTHS = [1, 2, 3, 4, 5, 7, 16, 100, 1000, 4000]
E_WINDOWS = {"w40_180": (40.0, 180.0), "w100_180": (100.0, 180.0), "w_50_60": (-50.0, 60.0), "w_shifted": (-37.5, 262.25), "w0_0": (0.0, 0.0), "w_narrow": (77.0, 123.0)}
# family -> window; "fuzz<m>" / "sym<m>": mode m of test_fuzz_bit_exact / test_symmetric_fast_path_is_exact_whenever_it_applies (tests/test_select_host.py)
E_FAMILIES = {"fuzz0": "w40_180", "fuzz1": "w40_180", "fuzz2": "w40_180", "fuzz3": "w100_180", "fuzz4": "w_50_60", "fuzz5": "w40_180", "fuzz6": "w_shifted", "fuzz7": "w0_0",
              "sym0": "w40_180", "sym1": "w40_180", "sym2": "w40_180", "sym3": "w40_180", "sym4": "w_50_60", "sym5": "w40_180", "sym6": "w40_180", "sym7": "w_narrow",
              "sym8": "w40_180", "sym9": "w40_180", "directed": "w40_180"}
# families in which the symmetric path cannot apply (nothing is in range / the guard refuses the calibration) or always does
E_ONE_SIDED = {"fuzz7": "the window [0, 0] holds one value", "sym8": "|offset| beyond pg_sym_guard", "directed": "calibrations beyond pg_sym_guard"}


def _e_read(fam, rng):
    kind, mode = fam[:-1], int(fam[-1])
    n = rng.choice(E_LENGTHS if kind == "fuzz" else E_LENGTHS[1:])
    dig = rng.choice([2048.0, 8192.0]); rg = rng.uniform(200.0, 1500.0)
    off = float(rng.below(600) - 300)
    sds = [1, 5, 50, 300, 3000] if kind == "fuzz" else [1, 5, 50, 300]
    # the centre follows the calibration (the ported generators draw it from 300 .. 1500 codes whatever the scale, which leaves most
    # reads outside [40, 180] pA): 60 .. 160 pA, so that reads with in-range samples, and a median among them, are the rule
    centre = rng.uniform(60.0, 160.0) / (rg / dig) - off
    if rng.below(5) == 0: centre = rng.uniform(300.0, 1500.0)
    raw = np.clip(rng.normal_codes(centre, rng.choice(sds), n), -32768, 32767)
    spike = lambda per_mille: np.where(rng.mask(n, per_mille), rng.below(65535) - 32768, raw)
    if kind == "fuzz":
        if mode == 1: raw = spike(300)
        if mode == 2: raw = np.full(n, raw[0])
        if mode == 5: off = rng.uniform(-300.0, 300.0)
        if mode == 6: off = float(-500 - rng.below(2500))
    else:
        if mode == 1: raw = spike(50)
        if mode == 2: raw = spike(450)
        if mode == 3: off = rng.uniform(-300.0, 300.0)
        if mode == 5: rg = math.ldexp(rng.uniform(1.0, 2.0), rng.below(61) - 30)           # tiny / huge scales: the guard decides
        if mode == 6: raw = np.clip(raw[0] + (rng.u64(n) % np.uint64(3)).astype(np.int64) - 1, -32768, 32767)   # three adjacent codes
        if mode == 8: off = rng.uniform(-1e13, 1e13); rg = 1e14
        if mode == 9: raw = np.sort(raw)[:: rng.choice([1, -1])].copy()
    return raw, (dig, off, rg)


def _coarse_cal(log2_off):
    """|offset| = 2^log2_off >= 2^53: code + offset is rounded to a multiple of 2^(log2_off - 52), so that many adjacent codes share one
    pA; the scale puts all of them at ~110 pA. pg_sym_guard refuses the offset (sym == 0): stats_select_fast runs first. Every code
    is in range (the huge list)."""
    off = math.ldexp(1.0, log2_off)
    return (1.0, off, 110.0 / off)


def e_directed():
    """[(tag, raw, cal)] aimed at stats_select_fast's refusals (pg_kernels.hip); whichever path answers, the result must be the oracle's.
      equal_neighbours  the median's code and the code below it have the same pA (the first test after the median search)
      tied_successor    the median's code is the lower one of a pair of equal pA, the code below it differs: candidate t = 0 of the up
                        side ties with t = 1 (own_tie), so the first qualifying candidate is not `sure`
      lane0 / coarse    16, 64 and 1024 codes per pA value: the integer model of the candidate window (deviations spaced one scale apart)
                        is off by more than the 15 codes the window reaches, so the first qualifying candidate sits at lane 0 of its
                        window, or no candidate of a side qualifies and the window does not reach the side's last code
      one_sided         all samples at the interval's lowest (highest) codes: the down (up) side is empty or qualifies nowhere"""
    out = []
    rng = Rng(4242)
    for j in range(40):
        lg = [53, 53, 54, 57, 59, 63][j % 6]
        step = 1 << (lg - 52)
        cal = _coarse_cal(lg)
        n = [16, 100, 1000, 4000, 7][j % 5]
        centre = rng.below(40000) - 20000
        raw = np.clip(rng.normal_codes(centre, [1, 3, 40, 600][j % 4], n), -32768, 32767)
        out.append(("coarse%d_%d" % (step, j), raw, cal))
    cal = _coarse_cal(53)          # pairs: code + 2^53 is rounded to even (ties to the even significand)
    for j, m in enumerate([100, 101, 102, 103, -7, -8]):
        out.append(("pair_median_at_%d" % m, counted_read({m - 3: 20, m - 1: 25, m: 30, m + 1: 25, m + 2: 21}, 0, [0], 4300 + j), cal))
    for j, (lo, n_lo, hi, n_hi) in enumerate([(-32768, 100, -32767, 1), (32767, 100, 32766, 1), (-32768, 60, 32767, 59), (-32768, 59, 32767, 60)]):
        out.append(("one_sided%d" % j, counted_read({lo: n_lo, hi: n_hi}, 0, [0], 4400 + j), _coarse_cal(53 + j % 2)))
        out.append(("one_sided_fine%d" % j, counted_read({lo: n_lo, hi: n_hi}, 0, [0], 4500 + j), (1.0, 1.5e12 + 0.5 * j, 110.0 / 1.5e12)))   # distinct pA per code, guard refuses
    return out


@functools.lru_cache(maxsize=None)
def groups_e():
    """{window: Group}; meta family = the generator family of each read"""
    gs = {w: Group("E_" + w, pa, k1=True) for w, pa in E_WINDOWS.items()}
    for fi, (fam, w) in enumerate(E_FAMILIES.items()):
        if fam == "directed":
            for tag, raw, cal in e_directed():
                gs[w].add("directed_" + tag, raw, cal, family=fam)
            continue
        rng = Rng(500 + fi)
        for t in range(E_N):
            raw, cal = _e_read(fam, rng)
            gs[w].add("%s_%d" % (fam, t), raw, cal, family=fam)
    return gs


GROUPS = {"A": group_a, "B": group_b, "BZ": group_bz, "C": group_c, "D": group_d, "D_giant": group_d_giant}
for _w in E_WINDOWS:
    GROUPS["E_" + _w] = (lambda w: lambda: groups_e()[w])(_w)

# zlib.crc32 over every read's samples and calibration, in order: the generators above produce the same bytes on every numpy
CRCS = {
    "A": 0x4d359a31,
    "B": 0x263eac59,
    "BZ": 0x276a0e09,
    "C": 0xa19b2c8f,
    "D": 0x478bbe01,
    "D_giant": 0x0728262c,
    "E_w40_180": 0x856764e2,
    "E_w100_180": 0xbb1c4a60,
    "E_w_50_60": 0x87e21eb2,
    "E_w_shifted": 0x851205a1,
    "E_w0_0": 0x40f517e0,
    "E_w_narrow": 0x46d1064d,
}
