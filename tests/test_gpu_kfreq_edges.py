"""`poregen kmer_freq` on a FASTQ, on the MI355X (pg_kfreq_submit, kernels k_kf_lines and k_kf_count with its seam): the dense counts and
the odd keys and counts against tests/kfreq_ref.py, exactly, on the inputs of tests/kfreq_text_cases.py -- line ends, line starts, N and
lines of about k bytes around span and tile edges, units of odd length read in place (every second one unaligned), views off a 16-byte
boundary, a small stream cut everywhere and delivered byte by byte, units shorter than k, more than 256 tiles and a full unit, more odd
windows than a workgroup stages, homopolymers, page-locked input and NUL bytes. DESIGN.md 9.3 says which gap each test closes."""
import numpy as np
import pytest

import kfreq_ref as R
import kfreq_text_cases as T
from kfreq_fasta_cases import assert_result, rand_seq

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def counters():
    """One counter per k for the whole module: creating one allocates the odd-key list."""
    from poregen_amd.engine import KmerCounter
    made = {}

    def get(k):
        if k not in made:
            made[k] = KmerCounter(k)
        return made[k]
    yield get
    for kc in made.values():
        kc.close()


@pytest.fixture
def capped(monkeypatch):
    """A counter of its own whose odd list, and with it the unit, holds `cap` entries (PGKFREQ_ODD_CAP is read when it is created)."""
    from poregen_amd.engine import KmerCounter
    made = []

    def get(k, cap):
        monkeypatch.setenv("PGKFREQ_ODD_CAP", str(cap))
        made.append(KmerCounter(k))
        return made[-1]
    yield get
    for kc in made:
        kc.close()


def run(kc, data, cuts=()):
    at = 0
    for c in list(cuts) + [len(data)]:
        kc.submit(data[at:c]); at = c
    return kc.finish()


def on_device(data):
    import torch
    return torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()


def same(a, b):
    return np.array_equal(a.counts, b.counts) and a.odd_keys == b.odd_keys and np.array_equal(a.odd_counts, b.odd_counts)


@pytest.mark.parametrize("what", T.KINDS)
@pytest.mark.parametrize("k", T.K)
def test_span_and_tile_edges(counters, k, what):
    rng = np.random.default_rng(1000 * T.KINDS.index(what) + k)
    for data in (T.edge_stream(rng, k, 2 * T.SPAN, what), T.edge_stream(rng, k, T.TILE, what, reach=300)):
        assert_result(run(counters(k), data), R.count(data, k), k)


@pytest.mark.parametrize("k", (6, 7))
def test_edges_in_units_of_odd_length_read_in_place(capped, k):
    kc = capped(k, 2 * T.TILE + 1)            # units of 65 537 bytes of one device tensor: every second one starts off a 16-byte boundary
    rng = np.random.default_rng(50 + k)
    for what in T.KINDS:
        for data in (T.edge_stream(rng, k, 2 * T.SPAN, what), T.edge_stream(rng, k, T.TILE, what, reach=300)):
            t = on_device(data)
            assert t.data_ptr() % 16 == 0
            kc.submit(t)
            assert_result(kc.finish(), R.count(data, k), k)


@pytest.mark.parametrize("k", (5, 9))
def test_device_views_off_a_16_byte_boundary(counters, k):
    import torch
    rng = np.random.default_rng(60 + k)
    cases = []
    for what in T.KINDS:                        # three tiles and a bit; "n" and "seq_start" end inside a sequence line, whose next byte would count
        data = T.edge_stream(rng, k, T.TILE, what, reach=300)[:3 * T.TILE + 50]
        cases.append((data, R.count(data, k)))
    assert [T.line_index(d, len(d) - 1) % 4 == 1 for d, _ in cases] == [False, True, True, False]
    for off in range(1, 16):
        data, want = cases[off % 4]
        box = torch.full((len(data) + 64,), ord("T"), dtype=torch.uint8, device="cuda")      # poison: a newline in front, letters behind
        box[:off] = 10
        box[off:off + len(data)] = on_device(data)
        assert (box.data_ptr() + off) % 16 == off
        kc = counters(k)
        kc.submit(box[off:off + len(data)])
        assert_result(kc.finish(), want, k)


SMALL_NAMES = ("closed", "seq_open", "qual_open")


@pytest.mark.parametrize("name", SMALL_NAMES)
@pytest.mark.parametrize("k", T.K)
def test_small_whole_and_byte_by_byte(counters, k, name):
    data = T.SMALLS[SMALL_NAMES.index(name)]
    kc = counters(k)
    whole = run(kc, data)
    assert_result(whole, R.count(data, k), k)
    assert len(data) > 64 and same(run(kc, data, range(1, len(data))), whole)     # more units in flight than snapshots are kept


@pytest.mark.parametrize("name", SMALL_NAMES)
@pytest.mark.parametrize("k", T.K)
def test_small_one_cut_at_every_offset(counters, k, name):
    data = T.SMALLS[SMALL_NAMES.index(name)]
    kc = counters(k)
    whole = run(kc, data)
    assert_result(whole, R.count(data, k), k)
    for cut in range(len(data) + 1):
        assert same(run(kc, data, [cut]), whole), cut


@pytest.mark.parametrize("k", (7, 9, 12))
def test_small_in_units_shorter_than_k(capped, k):
    kc = capped(k, 5)
    for data in T.SMALLS:
        want = R.count(data, k)
        assert_result(run(kc, data), want, k)                 # host bytes, staged five at a time
        kc.submit(on_device(data))
        assert_result(kc.finish(), want, k)


@pytest.fixture(scope="module")
def two_units():
    """16 MiB and two tiles, and an offset inside a sequence line near its middle."""
    data = T.tiles_stream(np.random.default_rng(78), T.UNIT + 2 * T.TILE)
    at = data.rfind(b"\n", 0, len(data) // 2) + 1                  # a line start near the middle; from there to a sequence line of 40 bytes
    i = T.line_index(data, at)
    while i % 4 != 1 or data.find(b"\n", at) - at < 40:
        at, i = data.find(b"\n", at) + 1, i + 1
    cut = at + 20
    assert T.line_index(data, cut) % 4 == 1 and b"\n" not in data[cut - 20:cut + 20]
    assert data[:T.UNIT].count(b"\n") and data[T.UNIT:].count(b"\n")
    return data, cut


@pytest.mark.parametrize("k", (6, 9))
def test_more_than_256_tiles_and_a_full_unit(counters, two_units, k):
    data, cut = two_units
    want = R.count(data, k)
    kc = counters(k)
    kc.submit(on_device(data))                               # one piece: 512 tiles in front of the last workgroups, then a second unit
    assert_result(kc.finish(), want, k)
    assert_result(run(kc, data, [cut]), want, k)             # host bytes in two pieces cut inside a sequence line


@pytest.mark.parametrize("k", (5, 9, 12))
def test_more_odd_windows_than_a_workgroup_stages(counters, capped, k):
    rng = np.random.default_rng(70 + k)
    data = T.dirty(rng, 3000)
    want = R.count(data, k)
    assert len(data) < T.TILE and sum(n for key, n in want.items() if not set(key) <= set(b"ACGT")) > 2 * T.levels()[5]
    assert_result(run(counters(k), data), want, k)
    data = T.dirty(rng, 5000)                                # a list of 1000 entries: drained between the units, keys merged across drains
    assert_result(run(capped(k, 1000), data), R.count(data, k), k)


@pytest.mark.parametrize("k", T.K)
def test_homopolymers(counters, k):
    rng = np.random.default_rng(80 + k)
    pad = b"@" + b"A" * (T.SPAN - 40)                         # the line starts 38 bytes in front of a span edge
    wave = 64 * T.SPAN
    lines = (b"A" * (T.TILE + 300),                                                   # poly-A across a tile edge
             b"A" * (wave - 90) + rand_seq(rng, wave + 100),                          # wave 0: one code in every open run; wave 1: many
             rand_seq(rng, wave - 90) + b"C" * (wave + 100),
             (b"AC" * T.TILE)[:T.TILE + 301], (b"AC" * T.SPAN)[:3 * T.SPAN + 5])      # runs of one window each
    for seq in lines:
        data = T.one_line(seq, pad)
        assert_result(run(counters(k), data), R.count(data, k), k)
    r = run(counters(k), T.one_line(lines[0], pad))
    assert int(r.counts[0]) == T.TILE + 300 - k + 1 == int(r.counts.sum()) and not r.odd_keys


@pytest.mark.parametrize("k", (5, 9))
def test_page_locked_input(counters, k):
    import torch
    rng = np.random.default_rng(90 + k)
    data = T.edge_stream(rng, k, T.TILE, "short", reach=300) + T.dirty(rng, 2000)
    kc = counters(k)
    plain = run(kc, data)
    assert_result(plain, R.count(data, k), k)
    pinned = torch.frombuffer(bytearray(data), dtype=torch.uint8).pin_memory()
    assert pinned.is_pinned()
    view = pinned.numpy()
    at = 0
    for c in (len(data) // 3 | 1, 2 * len(data) // 3 | 1, len(data)):      # three pieces cut at odd offsets
        kc.submit(view[at:c])
        view[at:c] = ord("N")                                                # the caller's buffer is its own again once submit returns
        at = c
    assert same(kc.finish(), plain)


@pytest.mark.parametrize("k", (5, 9))
def test_nul_at_tile_edges_and_unit_seams(counters, k):
    from poregen_amd import _abi
    from poregen_amd.engine import PgError
    kc = counters(k)
    base = T.one_line(rand_seq(np.random.default_rng(k), 2 * T.TILE), b"@" + b"A" * (T.SPAN - 40))
    want = R.count(base, k)
    assert T.line_index(base, T.TILE) == 1 and T.line_index(base, 3 * T.TILE - 1) == 3
    for edge in (T.TILE, 3 * T.TILE):                        # a tile edge inside the sequence line, one inside the quality line
        for at in (edge - 1, edge):
            data = base[:at] + b"\0" + base[at + 1:]
            for cuts in ((), (at,), (at + 1,)):              # the NUL inside a unit, as a unit's first byte and as its last
                if edge == T.TILE:
                    with pytest.raises(PgError) as ei:
                        run(kc, data, cuts)
                    assert ei.value.status == _abi.PG_ERR_INPUT
                    assert_result(run(kc, T.SMALL), R.count(T.SMALL, k), k)      # usable afterwards
                else:
                    assert_result(run(kc, data, cuts), want, k)
