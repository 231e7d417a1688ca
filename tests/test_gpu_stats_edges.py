"""k_read_plan, k_read_stats and the rare workers (poregen_amd/csrc/pg_kernels.hip) on the reads of tests/stats_cases.py, in which every
sample decides: the device's median and MAD of every read (GmoveEngine.device_view(): d_med / d_mad) against the oracle's, all 64 bits.
What each group reaches, and that the cases are what they claim, is shown without a GPU in tests/test_stats_cases_host.py."""
import numpy as np
import pytest

import stats_cases as S

pytestmark = pytest.mark.gpu


class _A:
    def __init__(self, ptr, n): self.__cuda_array_interface__ = {"shape": (n,), "typestr": "<i8", "data": (int(ptr), False), "version": 2}


def _device_stats(eng, n):
    import torch
    v = eng.device_view()
    return (torch.as_tensor(_A(v.d_med, n), device="cuda").cpu().numpy().view(np.uint64), torch.as_tensor(_A(v.d_mad, n), device="cuda").cpu().numpy().view(np.uint64))


def _assert_equal(g, med, mad, what):
    emed, emad = S.expected(g)
    bad = np.flatnonzero((med != emed) | (mad != emad))
    assert bad.size == 0, (what, "%d of %d reads differ" % (bad.size, len(g)),
                           [(g.ids[i], "%016x %016x" % (med[i], mad[i]), "expected %016x %016x" % (emed[i], emad[i])) for i in bad[:6]])


def _run(groups, **kw):
    """one engine, the groups submitted one after the other; -> kernel_stats()"""
    from poregen_amd.engine import GmoveEngine
    eng = GmoveEngine(S.engine_params(groups[0], **kw))
    try:
        for g in groups:
            eng.submit(S.batch_of(g))
            eng.sync()
            med, mad = _device_stats(eng, len(g))
            _assert_equal(g, med, mad, (g.name, kw))
        return eng.kernel_stats()
    finally:
        eng.close()


@pytest.mark.parametrize("mode", ["default", "one_stream"])
def test_streaming_geometries_every_sample_decides(mode):
    """Group A, the main launch (1024-bin path): every head (beg mod 8) x tail (end mod 8) x number of whole 16-byte vectors -- none (fewer
    than 8 samples; 8 .. 14 around one boundary: va >= vb), 1, 63 / 64 / 65 (one row of 64 lanes), 511 / 512 / 513 (one pass of eight
    rows), 1024 / 1025 (a third pass of one vector) -- as loss and dup sentinel reads between padding reads of B's."""
    _run([S.group_a()], overlap=(False if mode == "one_stream" else None))


@pytest.mark.parametrize("narrow", [False, True], ids=["win15", "narrow"])
def test_interval_and_bin_edges(narrow):
    """Group B: spans 1 .. 1024 (main launch), 1025 .. 2048 (wide list), 2049 and 65536 (huge list) with the classes on the first and last
    bin and the codes next to the interval; intervals touching either end of int16 (the modulo-2^16 difference of stats_bin8 equals span);
    the median's bin at 0, 15, 16, span - 1 and in the last, partly valid lane beside 250 samples in the bins behind span; reads of 1, 2, 3
    samples; no in-range sample. Group BZ: zero inside the window, the median in, and on either side of, the zero-filled class; z0 == 0, z0 == span."""
    _run([S.group_b()], debug_narrow=narrow)
    _run([S.group_bz()], debug_narrow=narrow)


@pytest.mark.parametrize("vehicle", ["own_launch", "scan_chained", "len_partials"])
def test_rare_lists_reuse_their_histograms(vehicle, monkeypatch):
    """Group C, then the same reads in reverse order on the same engine (lists and counters left by the first batch): 130 wide and 130 huge
    reads, so that each of the 64 (then 130) wide workers and of the PG_HUGE_BLOCKS huge workers bins several reads into one histogram.
    The three launches the workers ride in: k_read_stats_rare (two streams, the default; profiling would switch the second stream off, so the
    launch is not named there), k_scan_chained<true> (one stream: the sample-offset scan, no k_read_stats_rare launch is recorded) and
    k_len_partials<true> (one stream, PGMOVE_DENSE_MIN=0: the chunk sums' launch is recorded, k_read_stats_rare is not)."""
    kw = {}
    if vehicle != "own_launch":
        kw = dict(overlap=False, profile=True)
    if vehicle == "len_partials":
        monkeypatch.setenv("PGMOVE_DENSE_MIN", "0")
    else:
        monkeypatch.delenv("PGMOVE_DENSE_MIN", raising=False)
    g = S.group_c()
    st = _run([g, g.reversed()], **kw)
    if vehicle == "scan_chained":
        assert st["scan_ev_len"][0] == 2 and "k_read_stats_rare" not in st and "len_partials" not in st, st
    if vehicle == "len_partials":
        assert st["len_partials"][0] == 2 and "k_read_stats_rare" not in st and "scan_ev_len" not in st, st
    if vehicle != "own_launch":
        assert st["k_read_stats"][0] == 2, st


@pytest.mark.parametrize("mode", ["default", "one_stream", "no_split", "few_helpers"])
def test_slices_of_long_reads(mode, monkeypatch):
    """Group D: sentinel reads of 2 * 16384 + {1, 7, 8, 9, 15, 16, 17} samples at beg mod 8 of 0, 1, 7 -- the last slice takes the va >= vb
    branch or holds one vector --, 32768 (not split) and 32769; split over helper waves, by one wave each, and with room for some helpers only."""
    g = S.group_d()
    long_reads = sum(1 for m in g.meta if not m.get("pad") and m["slices"] > 1)
    want = sum(m["slices"] - 1 for m in g.meta if not m.get("pad"))
    assert long_reads > 100 and want > 200
    monkeypatch.delenv("PGMOVE_NO_LONG_SPLIT", raising=False); monkeypatch.delenv("PGMOVE_LONG_HELPERS", raising=False)
    if mode == "no_split":
        monkeypatch.setenv("PGMOVE_NO_LONG_SPLIT", "1")
    if mode == "few_helpers":
        monkeypatch.setenv("PGMOVE_LONG_HELPERS", str(want // 3))
    st = _run([g], overlap=(False if mode == "one_stream" else None))
    split = st.get("long_reads_split", (0, 0.0))[0]
    if mode == "no_split":
        assert split == 0
    elif mode == "few_helpers":
        assert 1 <= split < long_reads and st["long_helpers_short_batches"][0] == 1, st
    else:
        assert split == long_reads and st.get("long_helpers_short_batches", (0, 0.0))[0] == 0, st


def test_reads_of_1024_slices_and_of_doubled_slices():
    """1024 * 16384 samples: 1024 slices, the most pg_long_geometry hands out; one sample more: 513 slices of 32768. A loss and a dup read each,
    B's on either side of every slice boundary (the per-position groups are test_slices_of_long_reads')."""
    g = S.group_d_giant()
    st = _run([g])
    assert st.get("long_reads_split", (0, 0.0))[0] == sum(1 for m in g.meta if not m.get("pad")), st


@pytest.mark.parametrize("narrow", [False, True], ids=["win15", "narrow"])
@pytest.mark.parametrize("window", sorted(S.E_WINDOWS))
def test_selection_paths(window, narrow):
    """Group E: the generator families of tests/test_select_host.py as reads of one engine per pa window, the calibration differing from
    read to read; stats_select_sym where it applies, stats_select_fast and stats_select behind it (debug_narrow: the general search alone)."""
    _run([S.groups_e()[window]], debug_narrow=narrow)
