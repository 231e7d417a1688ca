"""The rule of `poregen simulate` (csrc/pg_sim.h) restated in Python integers, independently of the C++: Philox4x32-10, the dwell and the
sample arithmetic, the walk of one read, the command's read drawing and its stride rounding. The three Philox known answers are those of
the Random123 distribution's test vectors; the worked read below was computed by hand-checkable steps from this file alone."""
from dataclasses import dataclass

M32 = 0xffffffff
OK, TOO_SHORT, BAD_BASE, NO_LEVEL = 0, 1, 2, 3
STREAM_READ, STREAM_DWELL, STREAM_SAMPLE = 0, 1, 2

# (counter, key, output)
PHILOX_KAT = [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((M32, M32, M32, M32), (M32, M32), (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


def philox(ctr, key):
    c0, c1, c2, c3 = ctr
    k0, k1 = key
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & M32, (p0 >> 32) ^ c3 ^ k1, p0 & M32
        k0, k1 = (k0 + 0x9E3779B9) & M32, (k1 + 0xBB67AE85) & M32
    return c0, c1, c2, c3


def draw(seed, read, stream, i):
    return philox((i, stream, read & M32, (read >> 32) & M32), (seed & M32, (seed >> 32) & M32))


def q_of(digitisation, range_e4):
    return (digitisation * 10 * 2 ** 32 + range_e4 // 2) // range_e4


@dataclass
class Rule:
    k: int
    m: int = 0
    rna: bool = False
    seed: int = 0
    digitisation: int = 8192
    range_e4: int = 14676100
    offset: int = 10
    off_spread: int = 0
    spread_pct: int = 50
    lead: int = 0
    lead_level: int = 0
    lead_stdv: int = 0

    @property
    def Q(self):
        return q_of(self.digitisation, self.range_e4)

    def kw(self):
        """The keywords of engine.SignalSimulator / engine.sim_walk."""
        return dict(sig_move_offset=self.m, rna=self.rna, seed=self.seed, digitisation=self.digitisation, range_e4=self.range_e4, offset=self.offset, off_spread=self.off_spread,
                    spread_pct=self.spread_pct, lead=self.lead, lead_level=self.lead_level, lead_stdv=self.lead_stdv)


def rule_ok(R):
    return (1 <= R.k <= 9 and 0 <= R.m <= 64 and 1 <= R.digitisation <= 2 ** 16 and R.range_e4 >= 1 and q_of(R.digitisation, R.range_e4) < 2 ** 40 and abs(R.offset) <= 2 ** 20
            and 0 <= R.off_spread <= 2 ** 16 and 0 <= R.spread_pct <= 100 and 0 <= R.lead <= 2 ** 20 and 0 <= R.lead_level < 2 ** 18 and 0 <= R.lead_stdv < 2 ** 18)


def off_r(R, read):
    return R.offset - R.off_spread + ((draw(R.seed, read, STREAM_READ, 0)[0] * (2 * R.off_spread + 1)) >> 32)


def dwell(R, read, e, D):
    w = D * R.spread_pct // 100
    lo, hi = max(1, D - w), D + w
    return lo + ((draw(R.seed, read, STREAM_DWELL, e)[0] * (hi - lo + 1)) >> 32)


def noise(x):
    return sum((w >> s) & 0xff for w in x[:3] for s in (0, 8, 16, 24)) - 1530


def sample(R, read, j, l, s, off):
    G = noise(draw(R.seed, read, STREAM_SAMPLE, j))
    v = l + ((s * G + 128) // 256)           # Python's // is the floor
    t = (v * R.Q + 2 ** 31) >> 32            # and its >> is arithmetic
    return max(-32768, min(32767, t - off))


BASES = {"A": 0, "C": 1, "G": 2, "T": 3, "U": 3}


def slot_of(kmer):
    s = 0
    for c in kmer:
        if c not in BASES:
            return -1
        s = s * 4 + BASES[c]
    return s


def event_slots(R, seq):
    """The slot of every event, or the status that refuses the read."""
    lb = len(seq)
    if lb < R.k:
        return TOO_SHORT
    if any(c not in BASES for c in seq):
        return BAD_BASE
    out = []
    for e in range(lb):
        i = min(max(e - R.m, 0), lb - R.k)
        first = lb - i - R.k if R.rna else i
        out.append(slot_of(seq[first:first + R.k]))
    return out


def walk(R, levels, stdvs, dwells, seq, read):
    """(status, ops, samples, off_r) of one read; seq is a str."""
    off = off_r(R, read)
    slots = event_slots(R, seq)
    if isinstance(slots, int):
        return slots, [], [], off
    if any(not levels[s] for s in slots):
        return NO_LEVEL, [], [], off
    ops = [dwell(R, read, e, int(dwells[s])) for e, s in enumerate(slots)]
    sig = [sample(R, read, j, R.lead_level, R.lead_stdv, off) for j in range(R.lead)]
    j = R.lead
    for s, n in zip(slots, ops):
        for _ in range(n):
            sig.append(sample(R, read, j, int(levels[s]), int(stdvs[s]), off))
            j += 1
    return OK, ops, sig, off


def pick(seed, read, total, read_len, rna):
    """The command's read drawing: (position over the concatenated contigs, length before the cut at the contig's end, reverse strand)."""
    x = draw(seed, read, STREAM_READ, 1)
    u = (x[0] << 32) | x[1]
    lo, hi = read_len // 2, read_len + read_len // 2
    return (u * total) >> 64, lo + ((x[2] * (hi - lo + 1)) >> 32), (not rna) and bool(x[3] & 1)


def round_stride(B, lead, stride):
    return stride * ((B - lead + stride // 2) // stride)


def round_half_up_text(text, mult):
    """A decimal text times mult, to the nearest integer with halves up, exactly."""
    from fractions import Fraction
    import math
    return math.floor(Fraction(text) * mult + Fraction(1, 2))


# ---- one worked read: k = 2, six bases, read number 3, seed 7; every slot's level is 60000 + 1000 slot, stdv 1500 + 10 slot, dwell 4 + slot % 3
WORKED = dict(rule=Rule(k=2, m=1, seed=7, digitisation=8192, range_e4=14676100, offset=12, off_spread=3, spread_pct=50, lead=2, lead_level=75000, lead_stdv=1800),
              levels=[60000 + 1000 * s for s in range(16)], stdvs=[1500 + 10 * s for s in range(16)], dwells=[4 + s % 3 for s in range(16)], seq="GATTAC", read=3)
WORKED_SLOTS = [8, 8, 3, 15, 12, 1]            # event 0 is clamped onto the first k-mer, GA; then GA AT TT TA AC
WORKED_OFF_R = 13
WORKED_OPS = [9, 4, 4, 5, 2, 7]
WORKED_FIRST_SAMPLES = [410, 409, 357, 369, 359, 352, 362, 366, 365, 363]   # two of the lead, then eight of event 0
WORKED_N_SAMPLES = 33
