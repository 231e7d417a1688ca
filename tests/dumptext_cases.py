"""Batches of dump files placed on the seams of the dump-text parser (pg_dumptext.hip): 16-byte lanes, 1 KiB wave tiles,
4 KiB workgroups, file boundaries, declined files among strict ones, and the sizes at which the one-workgroup scans change their step.
A batch is (bytes, file_off, [file bytes]). Lane, tile and workgroup come from the library (pgt_dumptext_levels), never from literals.
tests/test_dumptext_host.py checks the placement claims and runs the files through oracle/model_oracle; tests/test_gpu_dumptext_edges.py
runs the batches on the device against tests/dumptext_ref.py."""
import ctypes as C
import functools
import os
import random

from dump_cases import ODD_FILES
from dumptext_ref import fmt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def hosttest():
    L = C.CDLL(os.environ.get("PG_HOSTTEST_SO") or os.path.join(ROOT, "poregen_amd", "_pg_hosttest.so"))
    L.pgt_dumptext_field.argtypes = [C.c_char_p, C.c_uint64, C.c_uint64, C.POINTER(C.c_int64), C.POINTER(C.c_int)]
    L.pgt_dumptext_field.restype = C.c_int
    return L


@functools.lru_cache(maxsize=None)
def levels():
    """(lane, tile, workgroup, min field) bytes of the kernels"""
    out = (C.c_uint32 * 4)()
    hosttest().pgt_dumptext_levels(out)
    return tuple(int(x) for x in out)


LANE, TILE, WG, MIN_FIELD = levels()
MAX_FIELD = 19                                     # "-39999999.99999999;"
F19 = b"-39999999.99999999"                        # the longest field and the shortest, without their separator
F11 = b"0.00000001"
EDGES = (TILE, WG, 2 * WG)


def batch(files):
    files = [bytes(f) for f in files]
    off = [0]
    for f in files:
        off.append(off[-1] + len(f))
    return b"".join(files), off, files


def pad_ok(L):
    return L == 0 or MIN_FIELD <= L <= MAX_FIELD or L >= 2 * MIN_FIELD


def _field(length, rng, sep):
    """one field of `length` bytes with its separator: an integer part below 1000 (zeros lead where the length asks for more digits), so
    that the values of a file stay within the reduction's spread; never a zero"""
    neg = length == MAX_FIELD or (length > MIN_FIELD and rng.random() < 0.4)
    nd = length - 10 - (1 if neg else 0)
    ip = rng.randrange(0, min(10**nd, 1000))
    return b"%s%0*d.%08d%s" % (b"-" if neg else b"", nd, ip, rng.randrange(1, 10**8), sep)


@functools.lru_cache(maxsize=None)
def pad(L, seed=0, ev=5):
    """one strict file of exactly L bytes (device-strict: small spread, no negative zero), in events of `ev` values"""
    assert pad_ok(L), f"no strict file has {L} bytes"          # 1..10, 20 and 21: fields are 11..19 bytes long
    if L == 0:
        return b""
    rng = random.Random(L * 7919 + seed)
    most = L // MIN_FIELD
    n = rng.randint(max(-(-L // MAX_FIELD), most * 3 // 4), most)
    lens, extra = [MIN_FIELD] * n, L - n * MIN_FIELD
    while extra:
        j = rng.randrange(n)
        if lens[j] < MAX_FIELD:
            add = rng.randint(1, min(MAX_FIELD - lens[j], extra))
            lens[j] += add; extra -= add
    out = [_field(l, rng, b";" if i == n - 1 or rng.randrange(ev) == 0 else b",") for i, l in enumerate(lens)]
    text = b"".join(out)
    assert len(text) == L
    return text


TAIL = pad(2 * TILE + 5, seed=99)                  # behind every probe: ranks behind it are checked as well


def fronts(offset):
    """strict files that fill exactly `offset` bytes: two where the size allows it, so that the probe's file is not the batch's first"""
    if offset == 0:
        return []
    for a in (35, 24, 13, 47):
        if offset - a > 0 and pad_ok(offset - a):
            return [pad(a, seed=1), pad(offset - a, seed=2)]
    assert pad_ok(offset), f"nothing fills {offset} bytes"
    return [pad(offset, seed=2)]


def at(offset, thing, lead=b""):
    """A batch in which `thing` begins at byte `offset`. thing: a list of files, which follow the front files; or bytes, the rest of a file
    whose first bytes are `lead` (the probe is then lead's file, which begins at offset - len(lead)). The fixed tail file comes last."""
    if isinstance(thing, (bytes, bytearray)):
        files = fronts(offset - len(lead)) + [lead + bytes(thing)]
    else:
        files = fronts(offset) + list(thing)
    return batch(files + [TAIL])


# ---- A: a field across an edge -------------------------------------------------------------------------------------------------------
A_LEAD = {F19: b"-39999999.50000000,-39999990.12345678,", F11: b"1.25000000,0.50000000,"}   # values next to the probe's: no spread
A_MORE = {F19: b"-39999998.00000000,-39999999.99999999;", F11: b"0.00000002,3.00000000;"}


def family_a():
    """[(batch, byte of the probe's separator)]: the 19-byte and the 11-byte field with the separator at E + d, d = -1 .. 19, once as the
    last field of the file and once in the middle of an event"""
    out = []
    for E in EDGES:
        for d in range(-1, 20):
            for f in (F19, F11):
                sep = E + d
                begin = sep - len(f)
                out.append((at(begin, f + b";", A_LEAD[f]), sep))
                out.append((at(begin, f + b"," + A_MORE[f], A_LEAD[f]), sep))
    return out


# ---- B: a file boundary across an edge -------------------------------------------------------------------------------------------------
B_NEXT = ([b"1.00000000;"], [b"-1.00000000,2.00000000;"], [b"", b"7.50000000,8.25000000;9.00000000;"])


def family_b():
    """[(batch, boundary byte, files behind the boundary)]"""
    return [(at(E + d, nxt), E + d, len(nxt)) for E in EDGES for d in range(-17, 18) for nxt in B_NEXT]


# ---- C: many files in a lane and in a wave ---------------------------------------------------------------------------------------------
def run_of(n, length):
    """n single-value files of `length` bytes, all values distinct"""
    nd = length - 10
    return [b"%0*d.%08d;" % (nd, (i * 7 + 1) % min(10**nd, 1000), 10**7 + i * 4099) for i in range(n)]


def family_c():
    S1, S2 = b"4.00000000,5.50000000;6.25000000;", b"-2.00000000,3.00000000,1.75000000;"
    out = []
    for length in (11, 12, 16):
        out.append(batch(run_of(200, length)))                             # 16-byte files from byte 0: a boundary on every lane edge
        out.append(at(TILE - 5 * length - 3, run_of(200, length)))         # ... and through a tile edge, off the lanes
        out.append(at(WG - LANE * 3, run_of(200, length)))                 # lane-aligned in front of a workgroup edge
    for r in (1, 2, 63, 64, 65):
        e = [b""] * r
        out += [batch(e + [S1, S2]), batch([S1] + e + [S2]), batch([S1, S2] + e), at(TILE - 11, [S1] + e + [S2])]
    out.append(batch([b""] * 5))                                           # n = 0 with five files
    out.append(batch([b"3.14159265;"]))
    return out


# ---- D: never in front of the file -----------------------------------------------------------------------------------------------------
D_PAIRS = [  # (first file: host, it does not end in ';'; second file; what the second must come to: units, or None for host)
    (b"1.00000000,12345", b"6.00000000;", [6 * 10**8]),
    (b"1.00000000,-", b"1.00000000;", [10**8]),
    (b"1.00000000,1.5", b".00000000;", None),
    (b"1.00000000,3999999", b"9.00000000;", [9 * 10**8]),
]


def family_d():
    """[(batch, boundary byte, index of the pair)]: the boundary at all 16 lane residues, and once exactly on a tile edge"""
    out = []
    for i, (first, second, _) in enumerate(D_PAIRS):
        for boundary in [WG - 3 * LANE + r for r in range(LANE)] + [TILE]:
            out.append((at(boundary - len(first), [first, second]), boundary, i))
    return out


# ---- E: declined files among strict ones -----------------------------------------------------------------------------------------------
def _fields(k, seed):
    rng = random.Random(seed)
    return [_field(rng.randrange(MIN_FIELD, 15), rng, b";" if rng.randrange(4) == 0 else b",") for _ in range(k)]


def declined(kind, k, seed=0):
    """a file outside the strict grammar that carries k separators (`;;`: k + 1)"""
    f = _fields(k if kind != "no_final" else k + 1, seed + k)
    f[-1] = f[-1][:-1] + b";"
    m = len(f) // 2
    if kind == "stray":
        f[m] = f[m][:3] + b"x" + f[m][4:]
    elif kind == "dec7":
        f[m] = b"2.5000000" + f[m][-1:]
    elif kind == "dec9":
        f[m] = b"2.500000001" + f[m][-1:]
    elif kind == "int9":
        f[m] = b"123456789.00000000" + f[m][-1:]
    elif kind == "4e7":
        f[m] = b"40000000.00000000" + f[m][-1:]
    elif kind == "plus":
        f[m] = b"+1.5" + f[m][-1:]
    elif kind == "semisemi":
        f[m] = f[m][:-1] + b";;"
    elif kind == "lead_comma":
        f = [b","] + f[1:]
    elif kind == "no_final":
        f[-1] = f[-1][:-1]
    else:
        raise ValueError(kind)
    return b"".join(f)


E_KINDS = ("stray", "dec7", "dec9", "int9", "4e7", "plus", "semisemi", "lead_comma", "no_final")
E_SEPS = (1, 70, 700)


def family_e():
    out = []
    for i, kind in enumerate(E_KINDS):
        for k in E_SEPS:
            s1, s2 = pad(700 + 37 * i + k % 7, seed=3), TAIL
            d1, d2 = declined(kind, k), declined(E_KINDS[(i + 4) % len(E_KINDS)], k, seed=5)
            out += [batch([s1, d1, s2]), batch([s1, d1, d2, s2]), batch([d1, s1, s2]), batch([s1, s2, d1])]
    odd = [c.encode() for _, c, _ in ODD_FILES]
    out += [batch(odd), batch(odd[::-1]), batch(odd[5:] + odd[:5])]
    return out


# ---- F: values -------------------------------------------------------------------------------------------------------------------------
def spread_file(n, dev, seed):
    """n values: the first two at the origin (100.0; the origin whether the first value is kept or not), one exactly `dev` units from it"""
    rng = random.Random(seed)
    O = 10**10
    u = [O, O] + [O + rng.randrange(-10**6, 10**6) for _ in range(n - 3)]
    u.insert(2 + rng.randrange(n - 2), O + dev)
    text = []
    for i, x in enumerate(u):
        text.append(fmt(x) + (b";" if i == n - 1 or i % 6 == 5 else b","))
    return b"".join(text)


def family_f():
    D = 1 << 40
    files = [
        b"39999999.99999999,39999999.99999998,39999999.99999990;39999999.99999999;",
        b"-39999999.99999999,-39999999.99999998;-39999999.99999990,-39999999.99999999;",
        b"0.00000000,0.00000001,-0.00000001,0.00000000;0.00000001;",
        b"00000000.00000001,00000001.00000000,00000012.50000000;",
        b"1.00000000,012345678.00000000;",                              # nine digits behind a leading zero: host
        b"1.00000000,-0.00000000,0.00000000;",                          # the middle values are (0, 0): host
        b"-0.00000000,-0.00000001,0.00000001;",                         # (-1, +1) when the negative zero is dropped: device
        b"-0.00000000,0.00000000,0.00000000;",                          # a negative zero that tail drops, a zero median: host all the same
        b"1.00000000,-00.00000000,0.00000000;",
        b"5.00000000,-0.00000000,2.00000000;3.25000000;",               # a negative zero away from the median: device
        b"-0.00000001,-0.00000000,-0.00000002,0.00000003,-0.00000004;",
    ]
    for n in (40, 5000):
        for dev in (D - 1, D, -(D - 1), -D):
            files.append(spread_file(n, dev, n + (dev > 0)))
    return [batch(files), batch(files[::-1] + [TAIL])]


# ---- G: events -------------------------------------------------------------------------------------------------------------------------
def events_file(n_events, per, seed):
    rng = random.Random(seed)
    return b"".join(b",".join(fmt(rng.randrange(-5 * 10**9, 5 * 10**9)) for _ in range(per)) + b";" for _ in range(n_events))


def family_g():
    files = [events_file(300, 1, 1), events_file(1, 3000, 2)] + [events_file(n, 3, n) for n in (255, 256, 257, 511, 512, 513)]
    return [batch([pad(50, seed=4), f, TAIL]) for f in files] + [batch(files)]


# ---- H: batch sizes ----------------------------------------------------------------------------------------------------------------------
def small_files(n, seed):
    """n files, each empty or of 11 bytes"""
    rng = random.Random(seed)
    return [b"%d.%08d;" % (rng.randrange(10), rng.randrange(10**8)) if rng.random() < 0.6 else b"" for _ in range(n)]


def family_h():
    out = []
    for size in (LANE, TILE, WG):
        for n in (size - 1, size, size + 1):
            out.append(batch([pad(n, seed=6)] if n < 100 else [pad(46, seed=6), pad(n - 46, seed=7)]))
    for n_files in (255, 256, 257, 1023, 1024, 1025):
        out.append(batch(small_files(n_files, n_files)))
    return out


@functools.lru_cache(maxsize=None)
def big_batch():
    """just over 1024 tiles (1 MiB + 2 tiles): k_dt_scan takes two tiles per thread. A few large files, 300 small ones, and one declined
    file behind the 1 MiB mark."""
    total = 1024 * TILE + 2 * TILE
    large = [pad(250000 + i, seed=10 + i, ev=9) for i in range(4)]
    small = [pad(MIN_FIELD + i % 9 if i % 3 else 22 + i % 40, seed=i) for i in range(300)]
    bad = declined("dec7", 70, seed=8)
    last = pad(600, seed=9)
    used = sum(map(len, large)) + sum(map(len, small)) + len(bad) + len(last)
    mid = pad(total - used, seed=11)
    b = batch(large[:2] + small[:150] + large[2:] + small[150:] + [mid, bad, last])
    assert len(b[0]) == total and b[1][-3] > 1024 * TILE
    return b


FAMILIES = {
    "A": lambda: [b for b, _ in family_a()],
    "B": lambda: [b for b, _, _ in family_b()],
    "C": family_c,
    "D": lambda: [b for b, _, _ in family_d()],
    "E": family_e,
    "F": family_f,
    "G": family_g,
    "H": family_h,
}


@functools.lru_cache(maxsize=None)
def family(name):
    return tuple(FAMILIES[name]())


def representative(name):
    """one batch of the family for the runs that repeat it in other memory (device bytes, unaligned views)"""
    f = family(name)
    pick = {"A": 2 * (21 * 2 + 4 * 2 + 0) + 1,      # workgroup edge, d = 3, the 19-byte field in the middle of an event
            "B": 3 * 12 + 2,                         # tile edge, d = -5, an empty file and a strict one behind the boundary
            "C": 1,                                  # 200 files of 11 bytes through a tile edge
            "D": 3 * (LANE + 1) + LANE,              # 3999999 | 9.00000000; with the boundary on a tile edge
            "E": 4 * 2 + 1,                          # 700 separators in two declined files between strict ones
            "F": 0, "G": len(f) - 1, "H": len(f) - 1}[name]
    return f[pick]
