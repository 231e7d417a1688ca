"""Shared by the command tests of the signal-to-reference model loop (`gmove --reform --ref --realign`, `fit --ref`, `realign --ref`): a
refops_cases.MappedSet -- mapped records with about 5 % I / D / S in their CIGARs, contigs built from the reads -- whose signal is planted
from a 5-mer model's levels over the k-mers the REFERENCE spells, under boundaries jittered off the move table's stride; the files of the
run; and the expected refined PAF printed from the Python rounds (mvops_ref -> refops_ref -> realigngap_ref). Nothing here calls the
product."""
import numpy as np

import fit_ref as R
import fitgap_ref as G
import kfreq_reads_cases as K
import mvops_ref as MV
import realigngap_ref as RG
import refops_cases as X
import refops_ref as XR
from poregen_amd import synth

K5 = 5
DUR = (5, 70)


def kmers(k):
    out = [""]
    for _ in range(k):
        out = [p + c for p in out for c in "ACGT"]
    return out


class RefRealignSet:
    """ms: a MappedSet whose records lie forward on ms.contigs (StrandedSet.b is one too). The signal of every taken record is replaced
    in `full` (the batch the signal files are written from) before anything is written."""

    def __init__(self, d, ms, seed, trim=0, band=10, min_len=3, min_events=20, m=0):
        rng = np.random.default_rng(7000 + seed)
        self.d, self.ms, self.rna, self.trim = d, ms, ms.rna, trim
        self.band, self.min_len, self.min_events, self.m = band, min_len, min_events, m
        lv = 60000 + 80 * rng.permutation(1024)                            # 60 .. 141.9 pA, all different
        self.model = d / "k5.model"
        self.model.write_text("kmer\tlevel_mean\tlevel_stdv\n" + "".join(f"{km}\t{lv[i] / 1000:.3f}\t2.000\n" for i, km in enumerate(kmers(K5))))
        self.levels = R.parse_model(self.model.read_text())[1]
        self.full = ms.with_lead(trim) if trim else ms.b
        self.full.sig = np.array(self.full.sig, np.int16)                   # (writable, and the MappedSet's own when there is no lead)
        self.contigs = dict(ms.in_fasta)
        self.lens = dict((n, len(s)) for n, s in ms.contigs)
        self.taken = [x for x in ms.recs if not (x["flag"] & 0x914) and x["rname"] != "*"]
        self.proj = {}
        for x in self.taken:
            self._plant(rng, x)

    def projected(self, x):
        """(Projected, slice, ns) of a record: its expansion carried through its CIGAR, and its slice of the FASTA ("" for a contig it lacks)"""
        if x["name"] not in self.proj:
            ns = self.ms._ns(x["r"], self.trim)
            e = MV.expand(self.ms._mv(x["r"], 5)[1:], 5, ns, self.trim, K.codes_of(x["seq"].encode()), x["flag"], MV.RNA if self.rna else 0)
            p = XR.project(e.ops, e.query_start, e.status, x["words"], x["pos"], self.rna)
            assert p.status == 0, (x["name"], p.status)
            lo = min(p.target_start, p.target_end)
            self.proj[x["name"]] = (p, self.contigs.get(x["rname"], "")[lo:lo + p.ref_len] if x["rname"] in self.contigs else "", ns)
        return self.proj[x["name"]]

    def signal(self, x):
        so = self.full.sig_off
        return self.full.sig[int(so[x["r"]]):int(so[x["r"] + 1])]

    def _plant(self, rng, x):
        p, sl, ns = self.projected(x)
        ops, types = [v for v, _ in p.ops], [t for _, t in p.ops]
        starts, cols = G.layout(ops, types, p.query_start)
        if len(sl) != cols[-1]:
            return
        H = list(starts)                                                   # where the levels change: off the stride by up to 2 samples
        for e in range(1, len(ops)):
            if types[e - 1] == 0 and types[e] == 0:
                H[e] = max(min(starts[e] + int(rng.integers(-2, 3)), starts[e + 1] - 1), H[e - 1] + 1)
        sig = self.signal(x)
        a, b = float(rng.uniform(300, 600)), float(rng.uniform(0.004, 0.008))
        for j, kmer, _, _ in G.pairing(sl, ops, types, p.query_start, K5, self.m, self.rna):
            s0, s1 = H[j], min(H[j + 1], len(sig))
            if s1 > s0 and all(c in "ACGT" for c in kmer):
                sig[s0:s1] = np.rint(a + b * self.levels[R.slot_of(kmer)]).astype(np.int64) + rng.integers(-3, 4, s1 - s0)

    def write(self):
        """s.slow5 (the oracle reads it), s.blow5, s.fastq (the basecalled reads), map.sam, map.bam, ref.fa"""
        pre = str(self.d / "s")
        synth.write_files(self.full, pre)
        synth.write_blow5(self.full, pre + ".blow5")
        self.ms.write_sam(self.d / "map.sam", trim=self.trim); self.ms.write_bam(self.d / "map.bam", trim=self.trim, block_bytes=3000)
        self.ms.write_fasta(self.d / "ref.fa")
        return self

    def rounds(self, x, n_rounds, band=None):
        p, sl, ns = self.projected(x)
        ops, types = [v for v, _ in p.ops], [t for _, t in p.ops]
        key = ("rounds", x["name"], n_rounds, band)
        if key not in self.proj:
            self.proj[key] = RG.rounds(sl, ops, types, p.query_start, [int(v) for v in self.signal(x)], self.levels, K5, self.m, self.rna, DUR[0], DUR[1], self.min_events,
                                       self.band if band is None else band, self.min_len, n_rounds)
        return self.proj[key]

    def refined_paf(self, n_rounds, band=None):
        """The PAF `reform -c -k 1 --stride 0 --to_ref` prints, with the durations the Python rounds leave"""
        import copy
        out = []
        for x in self.taken:
            p, sl, ns = self.projected(x)
            q = copy.copy(p)
            q.ops = list(zip(self.rounds(x, n_rounds, band)[-1][4][0], [t for _, t in p.ops]))
            out.append(XR.paf_line(x["name"], ns, q, x["rname"], self.lens[x["rname"]]))
        return "".join(out)

    def plain_paf(self):
        return "".join(XR.paf_line(x["name"], self.projected(x)[2], self.projected(x)[0], x["rname"], self.lens[x["rname"]]) for x in self.taken)

    def check_conditions(self):
        """At least half of the records are ok in round 1, and each of those has a boundary moved."""
        first = [self.rounds(x, 1)[0] for x in self.taken]
        ok = [r for r in first if r[0] == R.OK]
        assert 2 * len(ok) >= len(self.taken) > 0, (len(ok), len(self.taken))
        assert all(r[4][2] >= 1 for r in ok)
        return len(ok)
