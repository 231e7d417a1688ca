"""k_events' geometry for the direct ranking with both slot tables in LDS (k <= 5, <= 1024 slots) at its edges: 16 consecutive ops per
thread, 256 threads per tile of 4096 ops, four tiles per workgroup; a group whose reads leave the straight-line form goes through the
per-event or the per-op form. Every case goes through the C ABI with a sample limit no k-mer reaches, so that every slot the kernel wrote
shows in the result, and equals the CPU oracle bit for bit. (The op counts and the halves of a workgroup are those at which a geometry of
two groups per thread -- tiles tq and tq + 2, tools/probe/r07_events_two_groups.patch, DESIGN 3.9 -- has its seams as well.)"""
import numpy as np
import pytest

from helpers import assert_result_equals_oracle, oracle_for
from poregen_amd import synth
from poregen_amd.engine import Batch, GmoveEngine, GmoveParams, PgError, generate_kmers

pytestmark = pytest.mark.gpu

TILE, GROUP, TBL = 4096, 16, 128   # PG_SORT_TILE, ops per group, PG_EV_TBL
LIMIT = 1000000                    # no k-mer ever completes


def build(reads, seed, long_op=()):
    """reads: (match ops, RNA-oriented, with an insertion) per read; op lengths 3 .. 80 samples on both sides of the duration window
    [5, 70] of the cases below. long_op: reads whose third op gets 2^24 samples."""
    rng = np.random.default_rng(seed)
    sig, sig_off, seq, seq_off, op_n, op_t, op_off, ts, te = [], [0], [], [0], [], [], [0], [], []
    for r, (nm, rna, indel) in enumerate(reads):
        n = rng.integers(3, 81, nm).tolist(); t = [0] * nm
        if r in long_op:
            n[2] = 1 << 24
        if indel:
            n.insert(2, int(rng.integers(3, 9))); t.insert(2, 1)
        L = sum(n) + int(rng.integers(1, 5))
        sig.append(rng.integers(700, 1100, L).astype(np.int16)); sig_off.append(sig_off[-1] + L)
        bases = rng.integers(0, 4, nm)                   # a read without ops: an empty target range, skipped for every k
        seq.append(synth.BASES[bases[::-1]] if rna else synth.BASES[bases]); seq_off.append(seq_off[-1] + bases.size)
        op_n += n; op_t += t; op_off.append(op_off[-1] + len(n))
        ts.append(bases.size if rna else 0); te.append(0 if rna else bases.size)
    m = len(reads)
    return Batch(n_reads=m, sig=np.concatenate(sig), sig_off=np.asarray(sig_off, np.uint64), digitisation=np.full(m, 2048.0),
                 offset=np.full(m, -240.0), range=np.full(m, 281.0), query_start=np.zeros(m, np.int32), target_start=np.asarray(ts, np.int32),
                 target_end=np.asarray(te, np.int32), seq=np.concatenate(seq).astype(np.uint8), seq_off=np.asarray(seq_off, np.uint64),
                 op_n=np.asarray(op_n, np.uint32), op_t=np.asarray(op_t, np.uint8), op_off=np.asarray(op_off, np.uint64)).validate_host()


def run(b, kmers, **p):
    eng = GmoveEngine(GmoveParams(kmers=kmers, **p))
    try:
        eng.submit(b)
        return eng.finish()
    finally:
        eng.close()


def check(b, **p):
    kmers = generate_kmers(p["kmer_size"], rna=p["rna"])
    o = oracle_for(kmers, **p)
    rcs = o.run_batch(b)
    assert min(rcs) >= 0 and max(rcs) <= 1, "the generator must stay inside the reference's defined behaviour"
    assert_result_equals_oracle(run(b, kmers, **p), o, check_text_slots=2, sample_limit=LIMIT)


def plain_reads(n_ops, seed):
    """RNA-oriented direct reads of 30 .. 400 ops, n_ops in all; no read starts at a multiple of the tile, so a read spans every tile edge,
    every seam between a thread's two groups (multiples of 8192) and every workgroup edge (16384) the batch has"""
    rng = np.random.default_rng(seed)
    reads, at = [], 0
    while at < n_ops:
        n = min(int(rng.integers(30, 401)), n_ops - at)
        if (at + n) % TILE == 0 and at + n < n_ops:
            n += 1
        reads.append((n, True, False)); at += n
    starts = np.cumsum([0] + [n for n, _, _ in reads])[1:-1]
    assert at == n_ops and not np.any(starts % TILE == 0)
    return reads


@pytest.mark.parametrize("n_ops", [1, 15, 16, 17, 4095, 4096, 4097, 8191, 8193, 16383, 16384, 16385, 2 * 16384 + 1])
def test_op_counts_at_group_tile_and_workgroup_edges(n_ops):
    """The headline's shape (RNA, k = 5, one orientation, the window of an event its own op: the straight-line form) where a group, a
    tile, a pair of tiles or a second workgroup begins or ends one op early, exactly, or one op late."""
    b = build(plain_reads(n_ops, 1000 + n_ops), 2000 + n_ops)
    assert int(b.op_off[-1]) == n_ops
    check(b, kmer_size=5, rna=True, scaling=1, sample_limit=LIMIT, kmer_pick_margin=0, min_dur=5, max_dur=70)


def every_form_reads(rna, seed, without_ops=True):
    """Ten tiles (three workgroups) of reads that send groups through every form, in both halves of a workgroup: boundaries between
    direct reads of opposite orientation (with --rna only: the per-event form), reads of three and four ops
    back to back (three reads in a group: per-op form), reads without ops (and so without bases: the reference skips a read of fewer
    bases than k and is undefined on one that has none for k = 1 -- not with k = 1 then), reads with an insertion (k_walk's events passed through)
    next to direct ones, and stretches of six-op reads that put more than 128 reads into a tile (per-op form for the whole tile)."""
    rng = np.random.default_rng(seed)
    reads, at, it = [], 0, 0
    crowded = {1 * TILE + 700, 3 * TILE - 300, 6 * TILE + 100}   # stretches in tiles 1 (first half), 2 / 3 (second half: across a tile edge), 6 (second half)
    while at < 10 * TILE:
        if any(c <= at < c + 400 for c in crowded):
            c = next(c for c in crowded if c <= at < c + 400); crowded.discard(c)
            for _ in range(200):
                reads.append((6, rna and len(reads) % 2 == 0, False)); at += 6
            continue
        u = it % 9; it += 1
        n = int(rng.integers(40, 130))
        reads.append((n, rna and len(reads) % 2 == 0, u == 4)); at += n + (u == 4)
        if u == 2:
            reads += [(3, rna, False), (4, rna, False)]; at += 7
        if u == 6 and without_ops:
            reads.append((0, rna, False))
    return reads


def forms_seen(b, reads):
    """which (form, half of the workgroup) pairs the batch really holds, from its op_off alone -- the kernel's own rules restated"""
    off = b.op_off.astype(np.int64); n_ops = int(off[-1])
    with_ops = np.flatnonzero(np.diff(off) > 0)
    start = off[with_ops]; rna = np.array([reads[r][1] for r in with_ops]); direct = np.array([not reads[r][2] for r in with_ops])
    seen = set()
    over = set()
    for t in range((n_ops + TILE - 1) // TILE):
        lo, hi = t * TILE, min(t * TILE + TILE + GROUP, n_ops)
        first = int(np.searchsorted(off, lo, side="right")) - 1            # reads from the owner of the tile's first op on, with or without ops
        if int(np.searchsorted(off[:-1], hi, side="left")) - first > TBL:
            over.add(t); seen.add(("over", (t % 4) // 2))
    for g in range(0, n_ops, GROUP):
        t = g // TILE
        if t in over:
            continue
        a = int(np.searchsorted(start, g, side="right")) - 1
        inside = np.flatnonzero((start > g) & (start < g + GROUP))
        if inside.size >= 2:
            seen.add(("more", (t % 4) // 2))
        elif inside.size == 1 and direct[a] and direct[inside[0]] and rna[a] != rna[inside[0]]:
            seen.add(("mixed", (t % 4) // 2))
        if not direct[a] or (inside.size and not direct[inside[0]]):
            seen.add(("generic", (t % 4) // 2))
    return seen


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("rna", [False, True], ids=["dna", "rna"])
@pytest.mark.parametrize("k", [1, 2, 3, 4, 5])
def test_every_form_of_a_group_in_both_halves_of_a_workgroup(k, rna, offset):
    """sig_move_offset 1 takes every group out of the straight-line form: the window of an event is that of the next op"""
    reads = every_form_reads(rna, 300 + k, without_ops=k > 1)
    b = build(reads, 400 + k)
    want = {(f, h) for f in ("over", "more", "generic") + (("mixed",) if rna else ()) for h in (0, 1)}
    assert want <= forms_seen(b, reads), want - forms_seen(b, reads)
    assert any(n == 0 for n, _, _ in reads) == (k > 1)
    check(b, kmer_size=k, rna=rna, scaling=1, sample_limit=LIMIT, kmer_pick_margin=0, min_dur=5, max_dur=70, sig_move_offset=offset)


@pytest.mark.parametrize("bad,named", [((95,), 95), ((30, 95), 30)], ids=["in_the_second_half", "in_both_halves"])
def test_an_op_of_2_to_the_24_samples_names_the_lowest_read(bad, named):
    """read 30 lies in tile 0, read 95 in tile 2 (the workgroup's second half): the lowest failing read is reported"""
    reads = [(100, True, False)] * 120
    b = build(reads, 77, long_op=bad)
    assert int(b.op_off[30]) // TILE == 0 and int(b.op_off[95]) // TILE == 2
    kmers = generate_kmers(5, rna=True)
    with pytest.raises(PgError) as ei:
        run(b, kmers, kmer_size=5, rna=True, scaling=1, sample_limit=LIMIT, kmer_pick_margin=0, min_dur=5, max_dur=70)
    assert ei.value.status == -3 and f"read {named} of the batch" in ei.value.text, ei.value.text
