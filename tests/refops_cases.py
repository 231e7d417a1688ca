"""Shared by the tests of the projection onto the reference (pg_refops.h, pg_mvops_project, `reform --to_ref`, `gmove --reform --ref`):
reads and CIGARs that sit on the edges of the rule and of the kernels' shapes, batches of them laid out as the ABI takes them, and a
writer of MAPPED SAM / BAM records with mv / ns / ts tags whose reference is derived from the reads. Nothing here calls the product."""
import struct
import zlib

import numpy as np

import refops_ref as R
from poregen_amd import synth

P = 4096  # the library's piece (asserted against pg_mvops_piece by the tests that use it)


class Case:
    """One read: ops in signal order, query_start, the expansion's status, CIGAR words, 0-based pos."""

    def __init__(self, label, o, words, qs=100, status=0, pos=1000):
        self.label, self.o, self.words, self.qs, self.status, self.pos = label, [int(x) for x in o], [int(w) for w in words], int(qs), int(status), int(pos)

    def ref(self, rna=False):
        return R.project(self.o, self.qs, self.status, self.words, self.pos, rna)


def _query(words):
    return sum(w >> 4 for w in words if (w & 15) in (0, 1, 4, 7, 8))


def _ops(rng, n):
    return rng.integers(5, 200, n).tolist()


def from_text(rng, label, cigar, **kw):
    w = R.words_of(cigar)
    return Case(label, _ops(rng, _query(w)), w, **kw)


def random_words(rng, n_words, big=False):
    """n_words words: M runs with I / D / N / = / X between them, a clip at either end now and then."""
    out = []
    for i in range(n_words):
        if i == 0 and n_words > 2 and rng.random() < 0.5:
            out.append(int(rng.integers(1, 30)) << 4 | 4)
        elif i == n_words - 1 and n_words > 2 and rng.random() < 0.5:
            out.append(int(rng.integers(1, 30)) << 4 | 4)
        elif i % 2 == 0:
            out.append(int(rng.integers(1, 3000 if big and rng.random() < 0.1 else 40)) << 4 | int(rng.choice([0, 0, 0, 7, 8])))
        else:
            out.append(int(rng.integers(1, 80 if rng.random() < 0.1 else 4)) << 4 | int(rng.choice([1, 2, 2, 1, 3])))
    return out


def edit_words(rng, L, rate=0.05):
    """A CIGAR over L bases as an aligner writes it: M runs, about `rate` of the bases next to an I, a D or inside a clip."""
    out, left = [], L
    if rng.random() < rate * 4 and left > 20:
        n = int(rng.integers(1, 10)); out.append(n << 4 | 4); left -= n
    tail = int(rng.integers(1, 10)) if rng.random() < rate * 4 and left > 20 else 0
    left -= tail
    while True:                      # M runs with an I or a D between them; the last word in front of the trailing clip is an M
        m = min(left, int(rng.geometric(rate)))
        out.append(m << 4 | 0); left -= m
        if left == 1:
            out[-1] += 1 << 4; left = 0
        if left == 0:
            break
        if rng.random() < 0.5:
            n = min(left - 1, int(rng.integers(1, 4)))
            out.append(n << 4 | 1); left -= n
        else:
            out.append(int(rng.integers(1, 4)) << 4 | 2)
    if tail:
        out.append(tail << 4 | 4)
    assert _query(out) == L and all(w >> 4 for w in out)
    return out


def edge_cases(seed=1):
    rng = np.random.default_rng(seed)
    c = []
    for n in (1, 63, 64, 65, 129):
        w = random_words(rng, n, big=n > 1)
        c.append(Case(f"words{n}", _ops(rng, _query(w)), w))
    c.append(from_text(rng, "clean200", "200M"))
    c.append(from_text(rng, "clean10000", "10000M"))
    for m in (1, 63, 64, 65, P - 1, P, P + 1):
        c.append(from_text(rng, f"m{m}", f"{m}M"))
        c.append(from_text(rng, f"m{m}_between", f"5S{m}M2D3M1I2M"))
    c.append(from_text(rng, "m_across_piece_edge", f"{P - 100}M1D200M2I{P}M"))
    for i in (1, 64, 70):
        c.append(from_text(rng, f"i{i}", f"10M{i}I10M"))
    c.append(from_text(rng, "i_3_before_piece_edge", f"{P - 3}M10I50M"))
    c.append(from_text(rng, "i_17_at_piece_edge", f"{P}M17I5M"))
    c.append(from_text(rng, "i_longer_than_a_piece", f"10M{P + 904}I10M"))
    c.append(from_text(rng, "i_long_from_base_0", f"{2 * P + 1}I3M"))
    for s in (0, 1, P, 5000):
        c.append(from_text(rng, f"lead_s{s}", f"{s}S30M" if s else "30M"))
    c.append(from_text(rng, "two_leading_s", "3S2H4S30M"))
    c.append(from_text(rng, "trailing_s", "30M7S"))
    c.append(from_text(rng, "trailing_s_long", f"30M{P + 5}S"))
    c.append(from_text(rng, "h_both_ends", "3H5S20M4S2H"))
    c.append(from_text(rng, "s_in_the_middle", "5M3S5M"))
    c.append(from_text(rng, "leading_i", "3I10M"))
    c.append(from_text(rng, "leading_d", "2D10M"))
    c.append(from_text(rng, "s_then_d", "4S2D10M"))
    c.append(from_text(rng, "i_next_to_d", "5M2I3D5M"))
    c.append(from_text(rng, "d_next_to_i", "5M3D2I5M"))
    c.append(from_text(rng, "d_at_piece_edge", f"{P}M2D10M"))
    c.append(from_text(rng, "trailing_d", "10M4D"))
    c.append(from_text(rng, "trailing_d_at_piece_edge", f"{P}M4D"))
    c.append(from_text(rng, "other_ops", "5=2X3N1P4M2=1I3X"))
    c.append(Case("zero_length_words", _ops(rng, 8), [n << 4 | op for n, op in ((0, 4), (0, 0), (0, 1), (0, 2), (0, 3), (0, 5), (0, 6), (0, 7), (0, 8), (5, 0), (0, 4), (0, 2), (0, 1), (3, 0), (0, 0))]))
    c.append(Case("zero_length_m_in_front_of_s", _ops(rng, 9), [0 << 4 | 0, 4 << 4 | 4, 5 << 4 | 0]))   # the S is still a leading clip
    c.append(from_text(rng, "only_s_and_i", "3S4I2S"))
    c.append(from_text(rng, "only_s", "12S"))
    c.append(from_text(rng, "pos0", "20M2D3M", pos=0))
    c.append(from_text(rng, "l1_m", "1M"))
    c.append(from_text(rng, "l1_i", "1I"))
    c.append(from_text(rng, "l1_s", "1S"))
    c.append(Case("l0_d", [], R.words_of("3D")))
    c.append(Case("l0_h", [], R.words_of("5H")))
    c.append(Case("wraps", [0xfffffff0, 0x30, 0xffffffff, 7, 0x80000000, 0x80000001, 9], R.words_of("2S2I3M"), qs=0x7ffffff0, pos=0x7ffffffe))
    c.append(Case("big_d", _ops(rng, 4), [2 << 4 | 0, 0xfffffff << 4 | 2, 0xfffffff << 4 | 3, 2 << 4 | 0] + [0xfffffff << 4 | 2] * 15, pos=5))
    # refusals
    c.append(Case("no_cigar", _ops(rng, 10), []))
    c.append(from_text(rng, "ok_between_refused", "4M1D6M"))
    c.append(Case("too_short", _ops(rng, 10), R.words_of("4M1D5M")))
    c.append(Case("too_long", _ops(rng, 10), R.words_of("4M1I6M")))
    c.append(Case("too_long_by_2_to_the_32", _ops(rng, 10), [0xfffffff << 4 | 0] * 16 + [16 << 4 | 0, 10 << 4 | 0]))  # 16 (2^28 - 1) + 16 + 10 = 2^32 + 10
    c.append(Case("op9", _ops(rng, 10), [4 << 4 | 0, 0 << 4 | 9, 6 << 4 | 0]))
    c.append(Case("op15", _ops(rng, 10), [10 << 4 | 0, 3 << 4 | 15]))
    c.append(Case("short_and_op9", _ops(rng, 10), [4 << 4 | 0, 6 << 4 | 9]))                             # the length decides first
    c.append(Case("expansion_refused", [], R.words_of("10M"), status=3, qs=0))
    c.append(Case("expansion_refused_no_cigar", [], [], status=1, qs=17))
    c.append(from_text(rng, "ok_behind_refused", f"2S{P + 3}M1I4M"))
    return c


def random_batch(n, seed=3):
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        L = int(rng.integers(1, 700)) if i % 50 else int(rng.integers(P, 3 * P))
        out.append(Case(f"rand{i}", _ops(rng, L), edit_words(rng, L), qs=int(rng.integers(0, 5000)), pos=int(rng.integers(0, 1 << 20))))
    return out


def layout(cases, cigar_lead=0):
    """The ABI's arrays of a batch: op_n, op_off, query_start, status (the ops to project) and cigar, cigar_off, pos. cigar_lead words that
    belong to no read lie in front."""
    o = [x for c in cases for x in c.o]
    w = [0xfffffff0 | 9] * cigar_lead + [x for c in cases for x in c.words]
    return dict(op_n=np.array(o, np.uint64).astype(np.uint32), op_off=np.cumsum([0] + [len(c.o) for c in cases]).astype(np.uint64),
                query_start=np.array([c.qs for c in cases], np.int64).astype(np.int32), status=np.array([c.status for c in cases], np.uint32),
                cigar=np.array(w, np.uint64).astype(np.uint32), cigar_off=np.cumsum([cigar_lead] + [len(c.words) for c in cases]).astype(np.uint64),
                pos=np.array([c.pos for c in cases], np.int64).astype(np.int32))


def expected(cases, rna=False):
    refs = [c.ref(rna) for c in cases]
    ops = [x for f in refs for x in f.ops]
    i32 = lambda name: np.array([getattr(f, name) for f in refs], np.int64).astype(np.int32)
    return dict(status=np.array([f.status for f in refs], np.uint32), op_n=np.array([v for v, _ in ops], np.uint64).astype(np.uint32),
                op_t=np.array([t for _, t in ops], np.uint8), op_off=np.cumsum([0] + [len(f.ops) for f in refs]).astype(np.uint64),
                query_start=i32("query_start"), query_end=i32("query_end"), target_start=i32("target_start"), target_end=i32("target_end"),
                ref_len=np.array([f.ref_len for f in refs], np.uint32), n_match=np.array([f.n_match for f in refs], np.uint32))


# ---- mapped SAM / BAM with move tables: the reference is derived from the reads -------------------------------------------------------

class MappedSet:
    """synth.make_batch reads, a CIGAR drawn for each, and contigs built from the reads: a read's slice is its M bases plus random bases
    for D, embedded at pos between random flanks. Records of other kinds (unmapped, reverse strand, secondary, supplementary) can be
    mixed in; they carry names the signal file does not hold."""

    def __init__(self, kind, seed, n_reads=300, rate=0.05, contigs=3, missing_contig=False, mix=False, refuse_at=None, read_len=4000):
        rng = np.random.default_rng(seed + 1000)
        b = synth.make_batch(n_reads, kind=kind, seed=seed, read_len=read_len)
        b.target_start = np.zeros_like(b.target_start)
        self.b, self.rna = b, kind == "rna004"
        names = [f"ctg{i}" for i in range(contigs)] + (["ctgX"] if missing_contig else [])
        parts = {n: [self._rand(rng, 50)] for n in names}
        at = {n: 50 for n in names}
        self.recs = []                                       # dicts: name, flag, rname, pos (0-based), words, seq (str), r (index into b or None)
        for r in range(b.n_reads):
            seq = synth.seq_string(b, r)
            words = edit_words(rng, len(seq), rate)
            if refuse_at == r:
                words = words + [1 << 4 | 0]                  # one base more than SEQ has: status 6
            sl, q = [], 0
            for w in words:
                n, op = w >> 4, w & 15
                if op == 0:
                    sl.append(seq[q:q + n])
                if op == 2:
                    sl.append(self._rand(rng, n))
                if op in (0, 1, 4):
                    q += n
            sl = "".join(sl)
            ctg = names[r % len(names)]
            gap = self._rand(rng, int(rng.integers(0, 30)))
            parts[ctg] += [gap, sl]; pos = at[ctg] + len(gap); at[ctg] = pos + len(sl)
            if mix and r % 40 == 7:
                self.recs.append(dict(name=f"u{r}", flag=4, rname="*", pos=-1, words=[], seq=seq, r=r))
            if mix and r % 40 == 11:
                self.recs.append(dict(name=f"v{r}", flag=0x10, rname=ctg, pos=pos, words=words, seq=seq, r=r))
            if mix and r % 40 == 13:
                self.recs.append(dict(name=f"s{r}", flag=0x100, rname=ctg, pos=pos, words=words, seq=seq, r=r))
            if mix and r % 40 == 17:
                self.recs.append(dict(name=f"p{r}", flag=0x800, rname=ctg, pos=pos, words=words, seq=seq, r=r))
            if mix and r % 40 == 19:
                self.recs.append(dict(name=f"w{r}", flag=0, rname="*", pos=-1, words=[], seq=seq, r=r))   # flag 0 and no reference name
            self.recs.append(dict(name=f"r{r}", flag=0, rname=ctg, pos=pos, words=words, seq=seq, r=r))
        self.contigs = [(n, "".join(parts[n]) + self._rand(rng, 50)) for n in names]
        self.in_fasta = [c for c in self.contigs if c[0] != "ctgX"]
        self.n_skipped = sum(1 for x in self.recs if not (x["flag"] & 0x900) and ((x["flag"] & 0x14) or x["rname"] == "*"))

    @staticmethod
    def _rand(rng, n):
        return synth.BASES[rng.integers(0, 4, n)].tobytes().decode()

    def _mv(self, r, stride):
        d = self.b.op_n[int(self.b.op_off[r]):int(self.b.op_off[r + 1])]
        mv = [stride]
        for x in d:
            mv += [1] + [0] * (int(x) // stride - 1)
        return mv

    def _ns(self, r, trim):
        return int(self.b.sig_off[r + 1] - self.b.sig_off[r]) + trim

    def with_lead(self, trim, seed=9):
        """The batch with `trim` more samples in front of every read's signal: what a record with ts = trim is basecalled from."""
        import dataclasses
        rng = np.random.default_rng(seed)
        b = self.b
        parts = []
        for r in range(b.n_reads):
            parts += [rng.integers(300, 1500, trim).astype(np.int16), b.sig[int(b.sig_off[r]):int(b.sig_off[r + 1])]]
        return dataclasses.replace(b, sig=np.concatenate(parts), sig_off=(b.sig_off + np.arange(b.n_reads + 1, dtype=np.uint64) * np.uint64(trim)).astype(np.uint64))

    def write_fasta(self, path, width=60):
        with open(path, "w") as f:
            for n, s in self.in_fasta:
                f.write(f">{n} synthetic\n")
                for i in range(0, len(s), width):
                    f.write(s[i:i + width] + "\n")

    def write_sam(self, path, stride=5, trim=0):
        with open(path, "w") as f:
            f.write("@HD\tVN:1.6\tSO:unknown\n")
            for n, s in self.contigs:
                f.write(f"@SQ\tSN:{n}\tLN:{len(s)}\n")
            f.write("@PG\tID:synthetic\n")
            for x in self.recs:
                mv = ",".join(str(v) for v in self._mv(x["r"], stride))
                f.write(f"{x['name']}\t{x['flag']}\t{x['rname']}\t{x['pos'] + 1}\t60\t{R.text_of(x['words'])}\t*\t0\t0\t{x['seq']}\t*\tmv:B:c,{mv}\tqs:i:10\t"
                        f"ns:i:{self._ns(x['r'], trim)}\tts:i:{trim}\n")

    def write_bam(self, path, stride=5, trim=0, block_bytes=3000):
        code = {c: i for i, c in enumerate("=ACMGRSVTWYHKDBN")}
        text = b"@HD\tVN:1.6\tSO:unknown\n" + b"".join(f"@SQ\tSN:{n}\tLN:{len(s)}\n".encode() for n, s in self.contigs)
        raw = bytearray(b"BAM\x01" + struct.pack("<i", len(text)) + text + struct.pack("<i", len(self.contigs)))
        tid = {}
        for i, (n, s) in enumerate(self.contigs):
            raw += struct.pack("<i", len(n) + 1) + n.encode() + b"\x00" + struct.pack("<i", len(s)); tid[n] = i
        for x in self.recs:
            mv, seq = self._mv(x["r"], stride), x["seq"]
            name = x["name"].encode() + b"\x00"
            packed = bytearray((len(seq) + 1) // 2)
            for i, ch in enumerate(seq):
                packed[i >> 1] |= code.get(ch, 15) << (4 if i % 2 == 0 else 0)
            tags = (b"mvBc" + struct.pack("<i", len(mv)) + struct.pack(f"<{len(mv)}b", *mv) + b"qsC" + struct.pack("<B", 10)
                    + b"nsI" + struct.pack("<I", self._ns(x["r"], trim)) + b"tsI" + struct.pack("<I", trim))
            body = (struct.pack("<iiBBHHHiiii", tid.get(x["rname"], -1), x["pos"], len(name), 60, 4680, len(x["words"]), x["flag"], len(seq), -1, -1, 0) + name
                    + b"".join(struct.pack("<I", w) for w in x["words"]) + bytes(packed) + b"\xff" * len(seq) + tags)
            raw += struct.pack("<i", len(body)) + body
        with open(path, "wb") as f:
            def block(data: bytes):
                c = zlib.compressobj(6, zlib.DEFLATED, -15)
                comp = c.compress(data) + c.flush()
                f.write(b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff\x06\x00BC\x02\x00" + struct.pack("<H", 18 + len(comp) + 8 - 1) + comp
                        + struct.pack("<II", zlib.crc32(data) & 0xffffffff, len(data)))
            for o in range(0, len(raw), block_bytes):
                block(bytes(raw[o:o + block_bytes]))
            block(b"")

    def expected_paf(self, stride=5, trim=0):
        """The PAF of `reform -c -k 1 --stride 0 --to_ref [--rna]` by tests/mvops_ref.py and tests/refops_ref.py."""
        import kfreq_reads_cases as K
        import mvops_ref as MV
        lens = dict((n, len(s)) for n, s in self.contigs)
        out = []
        for x in self.recs:
            if x["flag"] & 0x900 or x["flag"] & 0x14 or x["rname"] == "*":
                continue
            e = MV.expand(self._mv(x["r"], stride)[1:], stride, self._ns(x["r"], trim), trim, K.codes_of(x["seq"].encode()), x["flag"], MV.RNA if self.rna else 0)
            p = R.project(e.ops, e.query_start, e.status, x["words"], x["pos"], self.rna)
            assert p.status == 0, (x["name"], p.status)
            out.append(R.paf_line(x["name"], self._ns(x["r"], trim), p, x["rname"], lens[x["rname"]]))
        return "".join(out)
