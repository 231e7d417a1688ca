"""The f1_score kernels (poregen_amd/csrc/pg_f1.hip) at their edges on the MI355X: the 16-byte spans and 4 KiB tiles of the byte
walk, the 8-step / 2048-step cuts of the merge path, the 32 MiB / 2^20-pair pieces, the refusals across those boundaries and values
near 2^62. Every expected count comes from tests/f1_ref.py (one signal point at a time) or from a derivation beside the case."""
import functools
import os
import subprocess

import numpy as np
import pytest

import f1_cases
import f1_ref as R
from poregen_amd import synth
from poregen_amd.engine import AlignmentScorer, PgError, f1_counts

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "bin", "poregen")
TILE, CHUNK, UNIT, UNIT_PAIRS = 4096, 2048, 32 << 20, 1 << 20  # kTile, kChunk, kUnit, kUnitPairs of pg_f1.hip
ERR_EMPTY, ERR_ENDS_DIGIT, ERR_NON_ASCII, ERR_COUNT, ERR_NO_POINTS = 1, 2, 3, 4, 5

# a pair here is (ss1, sig1, ref1, ss2, sig2, ref2): bytes and ints, side 2's ref with base_shift added


def from_si(ss1, si1, ss2, si2, base_shift=0):
    a, b = [R.py_int(v) for v in si1.split(",")], [R.py_int(v) for v in si2.split(",")]
    return (ss1, a[0], a[2], ss2, b[0], b[2] + base_shift)


def pack(pairs):
    ss = b"".join(p[0] + p[3] for p in pairs)
    lens = np.array([len(s) for p in pairs for s in (p[0], p[3])], np.uint64)
    off = np.concatenate([np.zeros(1, np.uint64), np.cumsum(lens, dtype=np.uint64)])
    sig = np.array([v for p in pairs for v in (p[1], p[4])], np.int64)
    ref = np.array([v for p in pairs for v in (p[2], p[5])], np.int64)
    return np.frombuffer(ss, np.uint8), off, sig, ref


@functools.lru_cache(maxsize=None)
def expanded(ss, sig, ref, direction):
    return R.expand(ss, sig, ref, direction)


def want_one(p, rna=False, threshold=0, region=None):
    d = -1 if rna else 1
    return R.compare(expanded(p[0], p[1], p[2], d), expanded(p[3], p[4], p[5], d), threshold, region)


def want(pairs, **kw):
    return np.array([want_one(p, **kw) for p in pairs], np.int64).reshape(-1, 4)


def on_device(ss, shift=0):
    """the bytes as a CUDA tensor that starts `shift` bytes into its allocation"""
    import torch
    buf = torch.zeros(ss.size + 16, dtype=torch.uint8, device="cuda")
    view = buf[shift:shift + ss.size]
    view.copy_(torch.from_numpy(np.array(ss)))
    return view


def score(sc, batch, device=False, shift=0):
    """per-pair counts of one batch on scorer sc; the totals must be their sums"""
    ss, off, sig, ref = batch
    sc.submit(on_device(ss, shift) if device else ss, off, sig, ref)
    got = sc.finish()
    pairs = got.pairs.astype(np.int64)
    assert np.array_equal(got.totals.astype(np.int64), pairs.sum(0))
    return pairs


def check(pairs, device=False, shift=0, sc=None, **kw):
    own = sc is None
    sc = sc or AlignmentScorer(**kw)
    try:
        got = score(sc, pack(pairs), device, shift)
    finally:
        if own:
            sc.close()
    exp = want(pairs, **kw)
    bad = np.nonzero((got != exp).any(1))[0]
    assert bad.size == 0, f"{bad.size} pairs differ, first {bad[0]}: {pairs[bad[0]]} got {got[bad[0]]} want {exp[bad[0]]}"


@pytest.fixture
def scorer():
    made = []

    def make(**kw):
        made.append(AlignmentScorer(**kw))
        return made[-1]
    yield make
    for sc in made:
        sc.close()


# ---- 1. the quirk table ---------------------------------------------------------------------------------------------------------------

def lib_kw(kw):
    return {k: v for k, v in kw.items() if k != "base_shift"}


@pytest.mark.parametrize("device", [False, True], ids=["host", "cuda"])
def test_quirk_table_per_row(device):
    for name, ss1, si1, ss2, si2, kw, exp in f1_cases.QUIRKS:
        batch = pack([from_si(ss1, si1, ss2, si2, kw.get("base_shift", 0))])
        ss = on_device(batch[0]) if device else batch[0]
        got = f1_counts(ss, *batch[1:], **lib_kw(kw))
        assert [int(v) for v in got.pairs[0]] == exp, name
        assert [int(v) for v in got.totals] == exp, name


def option_groups():
    groups = {}
    for row in f1_cases.QUIRKS:
        groups.setdefault(tuple(sorted(row[5].items())), []).append(row)
    return list(groups.items())


@pytest.mark.parametrize("device", [False, True], ids=["host", "cuda"])
def test_quirk_table_one_batch_per_option_set(device):
    # the rows side by side in one batch: a row's neighbours must not change it
    for opts, rows in option_groups():
        kw = dict(opts)
        pairs = [from_si(r[1], r[2], r[3], r[4], kw.get("base_shift", 0)) for r in rows]
        sc = AlignmentScorer(**lib_kw(kw))
        try:
            got = score(sc, pack(pairs), device)
        finally:
            sc.close()
        assert got.tolist() == [r[6] for r in rows], [r[0] for r in rows]


GROUPS = option_groups()


@pytest.mark.parametrize("opts,rows", GROUPS, ids=["-".join(f"{k}={v}" for k, v in o) or "default" for o, _ in GROUPS])
def test_quirk_table_cli(tmp_path, opts, rows):
    """The rows of one option set as the reads of a SAM pair and of a BAM pair. Every record spans chr1:0-1000, so --region keeps the
    records unless its END is 0 (pysam's fetch keeps pos < END), and then filters points on r1 + 1."""
    kw = dict(opts)
    recs1 = [dict(name=r[0], ss=r[1], si=r[2], cigar="1000M") for r in rows]
    recs2 = [dict(name=r[0], ss=r[3], si=r[4], cigar="1000M") for r in reversed(rows)]
    args = ["--read_limit", 0, "--threshold", kw.get("threshold", 0), f"--base_shift={kw.get('base_shift', 0)}"]
    if kw.get("rna"):
        args.append("--rna")
    reg = kw.get("region")
    if reg:
        args += ["--region", f"chr1:{reg[0]}-{reg[1]}"]
    tot = np.sum([r[6] for r in rows], 0) if not reg or reg[1] > 0 else np.zeros(4, int)
    line = b"TP\tFP\tTN\tFN\t%d\t%d\t%d\t%d" % tuple(int(v) for v in tot)
    for fmt, writer in (("sam", synth.write_alignment_sam), ("bam", synth.write_alignment_bam)):
        a, b = tmp_path / f"1.{fmt}", tmp_path / f"2.{fmt}"
        writer(str(a), recs1)
        writer(str(b), recs2)
        if fmt == "sam":
            exp = R.run(str(a), str(b), read_limit=0, base_shift=kw.get("base_shift", 0), rna=kw.get("rna", False),
                        threshold=kw.get("threshold", 0), region=f"chr1:{reg[0]}-{reg[1]}" if reg else None)
            assert exp.split(b"\n")[0] == line
        r = subprocess.run([BIN, "f1_score", str(a), str(b)] + [str(v) for v in args], capture_output=True)
        assert r.returncode == 0, r.stderr
        assert r.stdout == exp, fmt


# ---- 2. exhaustive small strings ------------------------------------------------------------------------------------------------------

SMALL = [s for s in f1_cases.small_strings() if f1_cases.maps_a_point(s)]

SMALL_CONFIGS = [  # sig1, sig2, ref1, ref2, rna, threshold, region
    (0, 0, 5, 5, False, 0, None), (0, 1, 5, 5, False, 0, None), (2, 0, 5, 6, False, 1, None), (0, 4, 5, 5, False, 0, None),
    (0, 0, -3, -3, False, 0, None), (0, 1, -2, -3, False, 1, None), (0, 0, 2, 2, True, 0, None), (2, 0, 1, 2, True, 1, None),
    (0, 0, 5, 5, False, -1, None), (0, 1, 0, 0, True, -1, None), (0, 0, -3, -2, False, 0, (0, 2)), (0, 4, 3, 2, True, 1, (-1, 1)),
]


@pytest.mark.parametrize("cfg", SMALL_CONFIGS, ids=[f"{i}" for i in range(len(SMALL_CONFIGS))])
def test_every_pair_of_small_strings(cfg):
    assert len(SMALL) == 84
    s1, s2, r1, r2, rna, thr, reg = cfg
    pairs = [(a, s1, r1, b, s2, r2) for a in SMALL for b in SMALL]
    check(pairs, device=cfg[0] == 2, rna=rna, threshold=thr, region=reg)


def test_sampled_longer_strings():
    rng = np.random.default_rng(20261017)
    tokens = [str(c).encode() + bytes([k]) for c in (0, 1, 3, 10, 999) for k in b",IDX"]
    pairs = []
    while len(pairs) < 3000:
        a, b = (b"".join(tokens[i] for i in rng.integers(0, len(tokens), int(rng.integers(3, 6)))) for _ in range(2))
        if f1_cases.maps_a_point(a) and f1_cases.maps_a_point(b):
            pairs.append((a, int(rng.integers(0, 6)), int(rng.integers(-5, 6)), b, int(rng.integers(0, 6)), int(rng.integers(-5, 6))))
    check(pairs, threshold=1)
    check(pairs, device=True, rna=True, threshold=0, region=(-3, 4))


# ---- 3. every alignment against spans and tiles -----------------------------------------------------------------------------------------

# multi-digit counts, a count behind 40 / 41 zeros (a digit run of more than two spans), I / D / X, a zero count, short tokens
PROBE = (b"12,3I" + b"0" * 40 + b"7,2D0,1,5X10,1I", 3, 100, b"9," + b"0" * 41 + b"4I3,1D11,2,0I7,", 0, 101)


def filler(total):
    """a pair of `total` ss bytes: "1," x 1000 against "2," tokens, led by one "10," when the rest is odd"""
    rest = total - 2000
    assert rest >= 5
    ss2 = (b"10," if rest % 2 else b"") + b"2," * ((rest - (3 if rest % 2 else 0)) // 2)
    assert 2000 + len(ss2) == total
    return (b"1," * 1000, 0, 7, ss2, 5, 9)


def test_probe_at_every_offset_around_a_tile_edge(scorer):
    sc = scorer(threshold=1)
    probe = want([PROBE], threshold=1)[0]
    assert probe.sum() > 0 and (probe > 0).sum() >= 3
    for start in range(TILE - 48, TILE + 49):
        pairs = [filler(start), PROBE]
        got = score(sc, pack(pairs))
        assert np.array_equal(got[1], probe), (start, got[1], probe)
        assert np.array_equal(got[0], want(pairs[:1], threshold=1)[0]), start


@pytest.mark.parametrize("shift", [1, 7, 15])
def test_probe_on_an_unaligned_device_view(scorer, shift):
    # a tensor view that starts inside an allocation: walk_span loads its bytes one by one
    sc = scorer(rna=True)
    probe = want([PROBE], rna=True)[0]
    for start in (TILE - 48, TILE - 17, TILE - 16, TILE - 15, TILE - 1, TILE, TILE + 1, TILE + 16, TILE + 33):
        pairs = [filler(start), PROBE, filler(start + 3)]
        got = score(sc, pack(pairs), device=True, shift=shift)
        assert np.array_equal(got, want(pairs, rna=True)), (start, got)
        assert np.array_equal(got[1], probe)


# ---- 4. merge-path and chunk edges ----------------------------------------------------------------------------------------------------

def random_side(n_ops, rng):
    """n_ops tokens: counts 0..3, mostly ',', with I, D and X; at least one point"""
    kinds = rng.choice(np.frombuffer(b",,,,,,,IDX", np.uint8), n_ops)
    cnt = rng.integers(0, 4, n_ops)
    if not ((cnt > 0) & ((kinds == ord(",")) | (kinds == ord("I")))).any():
        kinds[0], cnt[0] = ord(","), 2
    return b"".join(str(int(c)).encode() + bytes([k]) for c, k in zip(cnt, kinds))


def n_points(ss):
    return R.expand(ss, 0, 0, 1)[1].size


@pytest.mark.parametrize("total", [7, 8, 9, 2047, 2048, 2049, 4096, 4097])
def test_op_count_totals(total):
    rng = np.random.default_rng(total)
    pairs = []
    for na in (total // 2, 1, total - 1):
        a, b = random_side(na, rng), random_side(total - na, rng)
        if na == 1:
            a = str(max(1, n_points(b) - 1)).encode() + b","
        if total - na == 1:
            b = str(max(1, n_points(a) - 1)).encode() + b"I"
        pairs += [(a, 0, 3, b, 0, 3), (a, 2, 3, b, 0, 4)]
    check(pairs, threshold=1)
    check(pairs, device=True, rna=True, region=(-50, 1))


def test_ties_at_the_chunk_boundary():
    # Which side a cut takes first on a tie cannot change the counts: the interval between two tied boundaries is empty, and a thread
    # that starts inside a tie group walks the rest of it before its first non-empty interval. What these pairs catch is a cut that
    # loses or repeats a step (a chunk count rounded down fails here).
    # "1," / "3," then "2," on both sides: from merged position 3 on, positions (2k + 1, 2k + 2) hold the two sides' boundaries at the
    # same signal point, so a tie sits on every thread's cut (multiples of 8) and on the chunk's (2047, 2048)
    a, b = b"1," + b"2," * 1500, b"3," + b"2," * 1500
    # the same boundaries on both sides: ties at positions (2k, 2k + 1)
    c = b"2," * 1500
    # side 1's ops 1020..1029 map no point: with the op behind them they are 11 boundaries at point 1020, merged positions 2040..2050
    z = b"1," * 1020 + b"0,0I0D0X0," * 2 + b"1," * 500
    pairs = [(a, 0, 5, b, 0, 4), (b, 0, 5, a, 0, 6), (c, 0, 5, c, 0, 5), (z, 0, 5, b"1," * 1500, 0, 5), (b"1," * 1500, 0, 5, z, 0, 5)]
    check(pairs)
    check(pairs, device=True, threshold=1)


def test_window_clamped_at_its_start_and_end():
    long_, short = b"1," * 3000, b"1,1I2,1D" * 25
    pairs = [
        (long_, 0, 10, short, 2500, 2510),   # 2500 ops of side 1 before the window: the first chunk is boundaries clamped to 0
        (short, 2500, 2510, long_, 0, 10),   # ... of side 2
        (long_, 0, 10, short, 100, 110),     # about 2800 ops of side 1 past the window end, clamped to its length
        (short, 100, 110, long_, 0, 10),
        (long_, 0, 10, long_, 2999, 3009),   # a window of one point behind 2999 ops
        (long_, 2999, 3009, long_, 0, 10),
    ]
    check(pairs)
    check(pairs, device=True, rna=True, threshold=3000)


def typed_batch(types, idx):
    """the pairs types[i] for i in idx as one batch"""
    idx = np.asarray(idx)
    blobs = [t[0] + t[3] for t in types]
    ss = np.frombuffer(b"".join([blobs[i] for i in idx]), np.uint8)
    lens = np.empty(2 * idx.size, np.uint64)
    sig, ref = np.empty(2 * idx.size, np.int64), np.empty(2 * idx.size, np.int64)
    for side, (s, g, r) in enumerate(((0, 1, 2), (3, 4, 5))):
        lens[side::2] = np.array([len(t[s]) for t in types], np.uint64)[idx]
        sig[side::2] = np.array([t[g] for t in types], np.int64)[idx]
        ref[side::2] = np.array([t[r] for t in types], np.int64)[idx]
    return ss, np.concatenate([np.zeros(1, np.uint64), np.cumsum(lens, dtype=np.uint64)]), sig, ref


TINY = [(b"1,", 0, 5, b"1,", 0, 5), (b"2I", 0, 5, b"1,1,", 0, 5), (b"1,1D1,", 0, 5, b"3,", 0, 5), (b"3,", 0, 1, b"3,", 1, 1),
        (b"0,2,", 0, 10, b"1I1,", 0, 11)]
BIG = [(b"1,2," * 550, 0, 5, b"2,1," * 550, 1, 5),             # 2200 ops: two chunks
       (b"1,1I" * 1050, 3, 9, b"1,1,1D" * 700, 0, 8)]          # 4200 ops: three chunks


@pytest.fixture(scope="module")
def type_counts():
    types = TINY + BIG
    exp = want(types)
    assert len({tuple(r) for r in exp}) == len(types)  # no two types answer alike
    exp.setflags(write=False)
    return exp


@pytest.mark.parametrize("n", [1023, 1024, 1025, 2049])
def test_chunk_offsets_across_the_scan_carry(n, type_counts):
    rng = np.random.default_rng(n)
    idx = rng.choice(len(TINY) + len(BIG), n, p=[0.19] * 5 + [0.03, 0.02])
    idx[[0, n - 1]] = 5, 6                      # multi-chunk pairs at both ends ...
    idx[np.arange(1021, min(1027, n))] = (6, 5, 0, 6, 1, 5)[:min(1027, n) - 1021]  # ... and around the scan's block of 1024
    sc = AlignmentScorer()
    try:
        got = score(sc, typed_batch(TINY + BIG, idx))
    finally:
        sc.close()
    assert np.array_equal(got, type_counts[idx])


# ---- 5. piece edges ---------------------------------------------------------------------------------------------------------------------

def test_more_pairs_than_one_piece_takes(type_counts):
    n = UNIT_PAIRS + 3
    idx = np.arange(n) % len(TINY)
    assert idx[UNIT_PAIRS - 1] != idx[UNIT_PAIRS]
    sc = AlignmentScorer()
    try:
        got = score(sc, typed_batch(TINY, idx))
        assert np.array_equal(got, type_counts[idx])
        # the same scorer on a smaller batch afterwards
        small = np.arange(1000)[::-1] % len(TINY)
        assert np.array_equal(score(sc, typed_batch(TINY, small)), type_counts[small])
    finally:
        sc.close()


@pytest.fixture(scope="module")
def huge_pair():
    """One pair of more than 32 MiB: 8.6 M one-digit ops per side. Its expectation comes from f1_ref.expand_ops on the very count and
    kind arrays the bytes are written from (a one-digit op is the bytes '0' + count, kind), so no 17 MB string is parsed in Python."""
    rng = np.random.default_rng(32)
    n = 8_600_000
    sides = []
    for p_ins, hi in ((0.03, 2), (0.05, 3)):
        cnt = rng.integers(1, hi, n).astype(np.int64)
        r = rng.random(n)
        kind = np.where(r < p_ins, ord("I"), np.where(r < 2 * p_ins, ord("D"), ord(","))).astype(np.int64)
        kind[-1] = ord(",")
        ss = np.empty((n, 2), np.uint8)
        ss[:, 0], ss[:, 1] = 48 + cnt, kind
        sides.append((ss.reshape(-1), cnt, kind))
    (ss1, c1, k1), (ss2, c2, k2) = sides
    assert ss1.size + ss2.size > UNIT
    exp = R.compare(R.expand_ops(c1, k1, 0, 1000, 1), R.expand_ops(c2, k2, 40, 998, 1), 2, None)
    assert (exp > 0).all()
    before, after = [TINY[1], TINY[3]], [TINY[2], TINY[4], TINY[0]]
    bb, ba = pack(before), pack(after)
    ss = np.concatenate([bb[0], ss1, ss2, ba[0]])
    mid = np.array([ss1.size, ss1.size + ss2.size], np.uint64) + bb[1][-1]
    off = np.concatenate([bb[1], mid, ba[1][1:] + mid[-1]])
    sig = np.concatenate([bb[2], [0, 40], ba[2]])
    ref = np.concatenate([bb[3], [1000, 998], ba[3]])
    expect = np.concatenate([want(before, threshold=2), exp[None], want(after, threshold=2)])
    expect.setflags(write=False)
    return (ss, off, sig, ref), expect


@pytest.mark.parametrize("device", [False, True], ids=["host", "cuda"])
def test_one_pair_larger_than_a_piece(huge_pair, device):
    batch, expect = huge_pair
    sc = AlignmentScorer(threshold=2)
    try:
        assert np.array_equal(score(sc, batch, device), expect)
        # the same scorer on a smaller batch afterwards, as a fresh scorer answers it
        pairs = [PROBE, TINY[3], filler(TILE + 1)]
        assert np.array_equal(score(sc, pack(pairs), device), want(pairs, threshold=2))
    finally:
        sc.close()


# ---- 6. refusals across boundaries ------------------------------------------------------------------------------------------------------

GOOD = [TINY[2], PROBE, TINY[1]]


def refused(sc, batch, pair, code, side, device=False):
    """the batch is refused with that pair, code and side; then the same scorer answers a good batch"""
    ss, off, sig, ref = batch
    sc.submit(on_device(ss) if device else ss, off, sig, ref)
    with pytest.raises(PgError) as e:
        sc.finish()
    r = sc.last_result
    assert (int(r.err_pair), int(r.err_code), int(r.err_side)) == (pair, code, side), str(e.value)
    assert f"pair {pair}, file {side + 1}" in str(e.value)
    assert np.array_equal(score(sc, pack(GOOD)), want(GOOD))


def test_the_earlier_of_two_offending_pairs_is_reported(scorer):
    sc = scorer()
    # pair 1 (bytes from 5000, the second tile) maps no point: the highest code; pair 3 (the third tile) is empty: the lowest code
    pairs = [filler(5000), (b"5D", 0, 1, b"2,", 0, 1), filler(5001), (b"", 0, 1, b"2,", 0, 1), TINY[0]]
    refused(sc, pack(pairs), 1, ERR_NO_POINTS, 0)
    refused(sc, pack(pairs), 1, ERR_NO_POINTS, 0, device=True)
    refused(sc, pack(pairs[2:] + pairs[:2]), 1, ERR_EMPTY, 0)
    # within one pair: the lower code first, whichever side has it; then file 1 before file 2
    for ss1, ss2, code, side in ((b"4294967296,", b"3,4", ERR_ENDS_DIGIT, 1), (b"3,4", b"", ERR_EMPTY, 1), (b"5D", b"5D", ERR_NO_POINTS, 0),
                                (b"3,\xc3\xa9,", b"3,\xc3\xa9,", ERR_NON_ASCII, 0), (b"2,", b"0,0I3D", ERR_NO_POINTS, 1)):
        refused(sc, pack([filler(TILE + 5), TINY[0], (ss1, 0, 1, ss2, 0, 1), TINY[1]]), 2, code, side)


def test_every_small_string_without_a_point_is_refused(scorer):
    sc = scorer()
    none = [s for s in f1_cases.small_strings() if not f1_cases.maps_a_point(s)]
    assert len(none) == 72
    for i, s in enumerate(none):
        with pytest.raises(R.F1Error):
            R.pair_counts(s, "0,0,0,0", b"1,", "0,0,0,0")
        side = i & 1
        bad = (b"1,", 0, 0, s, 0, 0) if side else (s, 0, 0, b"1,", 0, 0)
        sc.submit(*pack([TINY[0]] * (i % 3) + [bad, TINY[1]]))
        with pytest.raises(PgError):
            sc.finish()
        r = sc.last_result
        assert (int(r.err_pair), int(r.err_code), int(r.err_side)) == (i % 3, ERR_NO_POINTS, side), s
    assert np.array_equal(score(sc, pack(GOOD)), want(GOOD))


def test_offending_pair_in_the_second_piece(scorer, type_counts):
    sc = scorer()
    n, bad = UNIT_PAIRS + 8, UNIT_PAIRS + 5
    idx = np.arange(n) % len(TINY)
    ss, off, sig, ref = typed_batch(TINY, idx)
    assert TINY[idx[bad]][0] == b"2I"
    ss = ss.copy()
    ss[int(off[2 * bad]) + 1] = ord("5")  # "25": ends in a digit
    refused(sc, (ss, off, sig, ref), bad, ERR_ENDS_DIGIT, 0)


@pytest.mark.parametrize("at", range(4090, 4103))
def test_offending_byte_around_a_tile_edge(scorer, at):
    sc = scorer()
    # a byte outside ASCII at piece offset `at`
    refused(sc, pack([filler(at - 2), (b"1,\xe9" + b"1,", 0, 1, b"2,", 0, 1), TINY[0]]), 1, ERR_NON_ASCII, 0)
    refused(sc, pack([filler(at - 4), (b"2,", 0, 1, b"1,\xe9" + b"1,", 0, 1)]), 1, ERR_NON_ASCII, 1)
    # a count of 2^32 whose first digit is at `at`, alone and behind zeros that begin there
    refused(sc, pack([filler(at), (b"4294967296,", 0, 1, b"2,", 0, 1), TINY[0]]), 1, ERR_COUNT, 0)
    refused(sc, pack([filler(at - 4), (b"2,", 0, 1, b"2," + b"0" * 20 + b"4294967296I", 0, 1), TINY[0]]), 1, ERR_COUNT, 1, device=True)
    # 2^32 - 1 there is accepted. By hand: side 1 maps 2^32 - 1 points to ref 5, side 2 three points from signal 7 to ref 5:
    # the window is those three points
    pairs = [filler(at), (b"4294967295,", 0, 5, b"3,", 7, 5), TINY[3]]
    got = score(sc, pack(pairs))
    assert got[1].tolist() == [3, 0, 0, 0]
    assert np.array_equal(got[[0, 2]], want([pairs[0], pairs[2]]))
    # 4294967295D: no point, so the restatement can follow it
    pairs = [filler(at), (b"1,4294967295D2,", 0, 5, b"1,2,", 0, 5 + 4294967295), (b"00004294967295D2,", 0, 5, b"2,", 0, 4294967300)]
    assert pairs[2][5] == 5 + 4294967295
    check(pairs, sc=sc)
    check(pairs, sc=sc, device=True)


# ---- 7. large magnitudes ----------------------------------------------------------------------------------------------------------------

LARGE = f1_cases.LARGE


@pytest.mark.parametrize("case", range(len(LARGE)))
def test_large_magnitudes(case):
    p, rna, thr, reg = LARGE[case]
    exp = R.pair_counts_py(*p, rna, thr, reg)
    for device in (False, True):
        batch = pack([TINY[0], p, TINY[1]])
        got = f1_counts(on_device(batch[0]) if device else batch[0], *batch[1:], rna=rna, threshold=thr, region=reg)
        assert [int(v) for v in got.pairs[1]] == exp, (got.pairs[1], exp)
